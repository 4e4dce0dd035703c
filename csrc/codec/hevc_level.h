// H.265 level selection (Annex A, Main tier): the lowest level whose picture size
// (MaxLumaPs), sample rate (MaxLumaSr) and decoded picture buffer (A.4.2 MaxDpbSize)
// hold a w x h session. Host only; shared by the parameter sets and the configuration check.
#pragma once

namespace sk {
namespace hevc {

// A.4.2: pictures a DPB of a level with MaxLumaPs `max_ps` holds at picture size `ps` (maxDpbPicBuf 6).
inline int max_dpb_size(double ps, double max_ps) {
    if (ps <= max_ps / 4) return 16;
    if (ps <= max_ps / 2) return 12;
    if (ps <= 3 * max_ps / 4) return 8;
    return 6;
}

// general_level_idc for a w x h picture at `fps`; dpb_pics > 0: the level must also hold that
// many pictures (the current one included), -1 when none does. dpb_pics == 0: sample rate and
// size only, level 6.2 when nothing fits.
inline int level_idc_for(int w, int h, float fps, int dpb_pics) {
    const double ps = (double)w * h, sr = ps * (fps > 0 ? fps : 60.0);
    struct L { int idc; double ps, sr; };
    static const L levels[] = {{30, 36864, 552960},          {60, 122880, 3686400},
                               {63, 245760, 7372800},        {90, 552960, 16588800},
                               {93, 983040, 33177600},       {120, 2228224, 66846720},
                               {123, 2228224, 133693440},    {150, 8912896, 267386880},
                               {153, 8912896, 534773760},    {156, 8912896, 1069547520},
                               {180, 35651584, 1069547520},  {183, 35651584, 2139095040},
                               {186, 35651584, 4278190080.0}};
    for (const L& l : levels)
        if (ps <= l.ps && sr <= l.sr && (dpb_pics <= 0 || dpb_pics <= max_dpb_size(ps, l.ps))) return l.idc;
    return dpb_pics > 0 ? -1 : 186;
}

}  // namespace hevc
}  // namespace sk
