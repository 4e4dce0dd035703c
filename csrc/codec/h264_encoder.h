// Session-level H.264 encoder interface: configuration, geometry, per-stripe
// control state (damage / paint-over / keyframe decisions) and the frame plan
// handed to an execution backend (CPU reference or the HIP pipeline).
//
// Stripe semantics mirror the pixelflux contract used by the reference server
// (selkies.py:2919-2964 CaptureSettings; client demux selkies-core.js:2925-3032):
//  * striped mode: every stripe is an independent H.264 stream (own SPS/PPS,
//    own IDR) emitted as a 0x04 packet [type|key|frame_id|y|w|h] + Annex-B;
//    undamaged stripes emit nothing.
//  * full-frame mode (encoder "x264enc"): one picture whose slices are the
//    stripes, emitted as a single 0x04 packet with y = 0.
#pragma once
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
#include <vector>
#include <string>
#include "h264_core.h"
#include "ratecontrol.h"
#include "ltr.h"
#include "hevc_level.h"
#include "av1_geo.h"

namespace sk {
namespace h264 {

struct EncoderConfig {
    int width = 1920;
    int height = 1080;
    int stripe_height = 64;      // pixels, multiple of 16
    int fullframe = 0;
    int full_range = 0;          // h264_fullcolor
    int qp = 25;                 // h264_crf mapped to a constant QP
    int paint_qp = 18;           // h264_paintover_crf
    int use_paint_over = 1;
    int paint_over_trigger = 15;
    int paint_over_burst = 5;
    int streaming_mode = 0;
    int damage_threshold = 10;
    int damage_duration = 20;
    int me_range = 64;           // max |mv| in integer pixels
    int me_iters = 24;           // diamond refinement iterations
    int scenecut = 1;
    float fps = 60.f;
    int deblock = 2;             // in-loop deblocking (idc 2: inside each slice): 0 off (x264 ultrafast), 1 on,
                                 // 2 automatic: the slices coded at QP >= kAutoDeblockQp (slice_deblock)
    int me_full = 1;             // +-16 exhaustive MFMA search candidate (dirty MBs of P slices)
    int shared_copy = 0;         // HIP: uploads on the device's shared copy stream (in submit order)
    int num_refs = 1;            // reference frames per stream (sliding-window DPB): 1, or 2 for the
                                 // previous-but-one picture as a second P reference (blinking/toggling UI)
    int src_width = 0;           // K2: capture size when it differs from width x height (0 = same);
    int src_height = 0;          //     the frame is resampled (bilinear) inside the K1 conversion
    int codec = 0;               // 0 = H.264, 1 = HEVC (hevc_encoder.h: same front end, full frame), 2 = AV1
    int tile_cols_log2 = -1;     // AV1 tiles (av1_encoder.h): -1 = automatic
    int tile_rows_log2 = -1;
    int rc_mode = RC_CQP;        // K10 rate control (ratecontrol.h): CQP, CRF (qp = CRF value), CBR
    int bitrate_kbps = 0;        // CBR target
    int vbv_ms = 0;              // CBR buffer (ratecontrol.h rc_init): 0 = 1.5 frame intervals
    int aq_strength = 0;         // MB-level adaptive QP strength, Q4 (16 = 1.0; 0 = off): h264_mb.h aq_offset
    int subpel = 1;              // quarter-pel refinement of P vectors (K4c, H.264 and HEVC); AV1 keeps integer vectors
    int intra4x4 = 0;            // H.264 I slices may code MBs as I_NxN (nine 4x4 modes) where cheaper; off
                                 // by default like x264's ultrafast preset (partitions none)
    int ltr_slots = 0;           // long-term reference cache (ltr.h): pictures kept per stream for content that comes
                                 // back (window switches); 0 = off, 1..8 (AV1: 1..7); H.264: excludes num_refs > 1
    int av1_intra_inter = 0;     // AV1: blocks of an inter frame whose inter coding left a residual are also tried as
                                 // intra blocks (luma palettes included, av1_core.h); the other codecs ignore it
    int av1_chroma_palette = 0;  // AV1: exact chroma palettes of 2..8 (U, V) pairs on intra blocks, where luma palettes may
                                 // occur (key frames; inter frames with av1_intra_inter); the other codecs ignore it
    int av1_cfl = 0;             // AV1: chroma from luma (UV_CFL_PRED) on intra blocks, where it costs less by RD than the
                                 // chroma coding standing (key frames; inter frames with av1_intra_inter); the other
                                 // codecs ignore it
    int av1_palette_cluster = 0; // AV1: luma palettes of clustered colours with a residual on intra blocks whose source
                                 // luma holds more than 8 values (anti-aliased text), where luma palettes may occur; the
                                 // other codecs ignore it
};

// Long-term cache slots in force (the three codecs share this configuration and the front end).
inline int ltr_slots_of(const EncoderConfig& c) {
    const int cap = c.codec == 2 ? ltr::kLtrAv1MaxSlots : ltr::kLtrMaxSlots;
    return c.ltr_slots > 0 ? (c.ltr_slots < cap ? c.ltr_slots : cap) : 0;
}

// The four AV1 tool options from a session's API values (> 0: on), after c.codec is set: the other
// codecs run with all of them off.
inline void set_av1_tools(EncoderConfig& c, int intra_inter, int chroma_palette, int cfl, int palette_cluster) {
    const bool av1 = c.codec == 2;
    c.av1_intra_inter = av1 && intra_inter > 0 ? 1 : 0;
    c.av1_chroma_palette = av1 && chroma_palette > 0 ? 1 : 0;
    c.av1_cfl = av1 && cfl > 0 ? 1 : 0;
    c.av1_palette_cluster = av1 && palette_cluster > 0 ? 1 : 0;
}

// HEVC cache expiry age in pictures (ltr.h ltr_expire): SK_HEVC_LTR_MAX_AGE=<n>, clipped to
// 2..32768 (tests exercise expiry at small sizes); read once when an encoder is built.
inline int ltr_max_age_env() {
    const char* e = getenv("SK_HEVC_LTR_MAX_AGE");
    return e && e[0] ? ltr::ltr_clip_max_age(atoi(e)) : ltr::kLtrMaxAge;
}

// The session's cache (ltr.h LtrConfig), for both back ends: the one place a codec maps to a mode.
inline ltr::LtrConfig ltr_config_of(const EncoderConfig& c) {
    ltr::LtrConfig l = {};
    l.slots = ltr_slots_of(c);
    if (!l.slots) return l;
    l.mode = c.codec == 2 ? ltr::LTR_BUFMAP : c.codec == 1 ? ltr::LTR_RPS : ltr::LTR_SECOND_REF;
    if (l.mode == ltr::LTR_BUFMAP)   // front-end slices in one tile row, the cache's decision unit
        l.unit_slices = av1::tile_row_units(c.width, c.height, c.tile_cols_log2, c.tile_rows_log2) / (c.stripe_height / 16);
    l.max_age = ltr_max_age_env();
    return l;
}

// Why a configuration cannot run the long-term cache (nullptr: it can, or the cache is off).
inline const char* ltr_config_error(const EncoderConfig& c) {
    if (c.ltr_slots <= 0) return nullptr;
    if (c.codec == 2) {   // AV1: a decoder owns eight buffers, one of them holds the previous picture
        if (c.ltr_slots > ltr::kLtrAv1MaxSlots)
            return "ltr_slots must be 0 (off) or 1..7 for AV1: the decoder's eight reference buffers hold the "
                   "previous picture and the cached ones";
        if (c.stripe_height <= 0 ||
            (av1::tile_row_units(c.width, c.height, c.tile_cols_log2, c.tile_rows_log2) * 16) % c.stripe_height)
            return "ltr_slots: the AV1 tile height must be a multiple of stripe_height (a tile row predicts from "
                   "one picture)";
        return nullptr;
    }
    if (c.ltr_slots > ltr::kLtrMaxSlots) return "ltr_slots must be 0 (off) or 1..8";
    if (c.codec == 1) {   // HEVC: current picture + previous picture + slots within some level's MaxDpbSize (A.4.2)
        if (hevc::level_idc_for((c.width + 15) & ~15, (c.height + 15) & ~15, c.fps, 2 + c.ltr_slots) < 0)
            return "ltr_slots: no H.265 level holds this picture size with that many long-term pictures (MaxDpbSize)";
        return nullptr;
    }
    if (c.num_refs > 1)
        return "ltr_slots > 0 cannot be combined with num_refs > 1: the cached picture takes the second reference "
               "list position";
    // the largest stream's DPB (one short-term picture + the slots) must fit level 5.2 (Table A-1 MaxDpbMbs)
    const int sh = c.fullframe ? c.height : (c.height < c.stripe_height ? c.height : c.stripe_height);
    if ((long)(1 + c.ltr_slots) * ((c.width + 15) / 16) * ((sh + 15) / 16) > 184320)
        return "ltr_slots: the decoded picture buffer would exceed H.264 level 5.2 (MaxDpbMbs)";
    return nullptr;
}

struct Geometry {
    int W = 0, H = 0, mb_w = 0, mb_h = 0, rows_per_slice = 0, num_slices = 0;
    int stride_y = 0, stride_c = 0, plane_h_y = 0, plane_h_c = 0;
    int fullframe = 0, stripe_height = 0;
    void init(const EncoderConfig& c) {
        W = c.width;
        H = c.height;
        fullframe = c.fullframe;
        stripe_height = c.stripe_height;
        mb_w = (W + 15) / 16;
        mb_h = (H + 15) / 16;
        rows_per_slice = c.stripe_height / 16;
        if (rows_per_slice < 1) rows_per_slice = 1;
        num_slices = (mb_h + rows_per_slice - 1) / rows_per_slice;
        stride_y = mb_w * 16;
        stride_c = mb_w * 8;
        plane_h_y = mb_h * 16;
        plane_h_c = mb_h * 8;
    }
    int slice_first_row(int s) const { return s * rows_per_slice; }
    int slice_rows(int s) const {
        int r = mb_h - s * rows_per_slice;
        return r < rows_per_slice ? r : rows_per_slice;
    }
    int slice_pix_y(int s) const { return s * rows_per_slice * 16; }
    int slice_pix_h(int s) const {
        int y0 = slice_pix_y(s);
        int y1 = y0 + slice_rows(s) * 16;
        if (y1 > H) y1 = H;
        return y1 - y0;
    }
    int num_mbs() const { return mb_w * mb_h; }
};

// Per-slice work item for one frame (POD, copied to device memory as is).
enum SliceAction : int32_t { ACT_NONE = 0, ACT_P = 1, ACT_I = 2, ACT_SKIPALL = 3 };
struct SliceTask {
    int32_t action;        // SliceAction requested by the controller
    int32_t qp;
    int32_t first_row;     // MB rows of the slice
    int32_t num_rows;
    int32_t pic_row0;      // first MB row of the picture this slice belongs to
    int32_t pic_rows;      // MB rows of that picture (MC clamp bounds)
    int32_t frame_num;     // frame_num if coded as P (or non-IDR I)
    int32_t idr_pic_id;    // idr_pic_id if coded as IDR
    int32_t allow_scenecut;
    int32_t idr_on_intra;  // striped mode: an I decision makes the stripe an IDR
    int32_t final_action;  // written by the backend (scene-cut may turn P into I)
    int32_t num_refs;      // P: reference pictures available to this slice (1..EncoderConfig::num_refs)
};
static_assert(sizeof(SliceTask) == 48, "SliceTask layout");

// K5 parallel key frames. An I slice of a stripe wider than kIntraSubMbs macroblocks is
// coded as sub-slices of kIntraSubMbs MBs each (consecutive in raster order, so most
// start mid-row: first_mb_in_slice at any MB). The reference's encoders split pictures
// the same way (num-slices 4, legacy/gstwebrtc_app.py:504, 538, 663). Since
// kIntraSubMbs < mb_w, no MB has its top neighbour in its own sub-slice: a sub-slice
// predicts from its left neighbours only, its reconstruction chain is at most
// kIntraSubMbs MBs long, and the sub-slices of a stripe are independent (one wave
// each on the GPU, k_code_intra_sub). With in-loop deblocking (disable_deblocking_filter_idc
// 2) the filter keeps off the sub-slice edges and restarts the QP_Y chain at each
// sub-slice (h264_deblock.h, k_deblock_prep / k_deblock_edges); Intra4x4 blocks see no
// top or top-right neighbour outside their sub-slice (k_code_intra_sub's I_NxN path).
constexpr int kIntraSubMbs = 40;
// Automatic deblocking (EncoderConfig::deblock = 2): a slice is filtered when it is coded
// at QP >= 34 - CBR under a tight budget, where the 4x4 / 16x16 block edges become
// visible - and left unfiltered at the CRF-25 default, as x264's ultrafast preset
// (legacy/gstwebrtc_app.py:637). Per slice, in its disable_deblocking_filter_idc (2 or 1):
// the stripes of one frame run at different (dithered) QPs.
constexpr int kAutoDeblockQp = 34;
SK_HD bool slice_deblock(int deblock, const SliceTask& t) {
    return deblock == 1 || (deblock == 2 && t.qp >= kAutoDeblockQp);
}
SK_HD bool intra_split(const SliceTask& t, int mb_w, int deblock, int intra4x4) {
    (void)deblock;
    (void)intra4x4;
    return t.final_action == ACT_I && mb_w > kIntraSubMbs;
}
// Sub-slices of a split I slice; nmb = its MBs.
SK_HD int intra_sub_count(int nmb) { return (nmb + kIntraSubMbs - 1) / kIntraSubMbs; }
// Upper bound of the NALs one stripe's slice can need (the GPU's per-stripe NAL slots).
SK_HD int max_nals_per_slice(int rows_per_slice, int mb_w) {
    return mb_w > kIntraSubMbs ? intra_sub_count(rows_per_slice * mb_w) : 1;
}

// K10: slices whose QP the rate controller sets: coded, and not a paint-over refresh
// (CRF; under CBR the refresh is budgeted like any other slice)
SK_HD bool rc_slice_adjustable(const SliceTask& t, int plan_qp, int mode = 1) {
    return (t.final_action == ACT_P || t.final_action == ACT_I) && (t.qp == plan_qp || mode == 2);
}

// Upper bound of the slice QPs (SliceTask::qp) of a frame that is planned under rate mode
// `mode` with QP `qp` and paint-over QP `paint_qp` (the configured values or their set_qp
// overrides, whichever apply to that frame). plan_stripe gives every slice one of the
// two. CQP: rc_apply leaves them. CRF: a slice at `qp` moves to rc_clamp_qp of
// rc_frame_qpf's base_qp + [-3, +6] (base_qp is `qp`; a whole QP, so rc_dither_qp adds
// nothing; H.264's qp_min can lift it), a paint-over slice keeps paint_qp. CBR: the
// controller and the guard's second pass (rc_redo) reach every QP up to 51, so no bound
// below that holds: 51. The HIP back end leaves its deblocking kernels out of a frame
// whose bound is below kAutoDeblockQp (deblock = 2).
SK_HD int max_slice_qp(int mode, int qp, int paint_qp) {
    if (mode == RC_CQP) return sk_max(qp, paint_qp);
    if (mode == RC_CRF) return sk_max(sk_clip(qp + 6, rc_qp_min_for(0), 51), paint_qp);
    return 51;
}

struct StripeState {
    int frame_num = 0;     // next frame_num
    int idr_pic_id = 0;
    bool need_idr = true;
    int static_frames = 0;
    int dirty_streak = 0;
    int hot_left = 0;
    int paint_left = 0;
    bool painted = true;   // nothing to paint before the first change
    int refs = 0;          // pictures in the decoder's DPB for this stream (sliding window)
    int subpel_hits = 0;   // MBs of this stripe's last frame given a fractional vector (K4c)
    int subpel_prev = 0;   // the same count one frame earlier: the adaptive refinement gate
};

// Controller knobs as a POD, so the same plan code runs on the host (CPU
// backend) and inside the HIP graph (k_plan), bit-for-bit the same decisions.
struct PlanConfig {
    int32_t fullframe, scenecut, use_paint_over, paint_over_trigger, paint_over_burst;
    int32_t damage_threshold, damage_duration, streaming_mode, qp, paint_qp, num_refs;
    int32_t ltr_slots;   // > 0: a stripe's scene-cut I slice stays a non-IDR picture (the cache survives it)
};
inline PlanConfig plan_config(const EncoderConfig& c) {
    return PlanConfig{c.fullframe, c.scenecut, c.use_paint_over, c.paint_over_trigger, c.paint_over_burst,
                      c.damage_threshold, c.damage_duration, c.streaming_mode, c.qp, c.paint_qp,
                      c.num_refs > 1 ? 2 : 1, ltr_slots_of(c)};
}
constexpr int kFrameNumMask = (1 << 16) - 1;  // log2_max_frame_num = 16 (h264_syntax.h)

// One stripe's decision for this frame; `pic` is the picture state (full-frame mode).
SK_HD void plan_stripe(const PlanConfig& c, StripeState& st, const StripeState& pic, bool d,
                              int first_row, int num_rows, int mb_h, SliceTask& t) {
    const bool ff = c.fullframe != 0;
    t = SliceTask{};
    t.first_row = first_row;
    t.num_rows = num_rows;
    t.pic_row0 = ff ? 0 : first_row;
    t.pic_rows = ff ? mb_h : num_rows;
    t.allow_scenecut = c.scenecut;
    t.idr_on_intra = (ff || c.ltr_slots > 0) ? 0 : 1;
    if (d) {
        st.static_frames = 0;
        st.dirty_streak++;
        st.painted = false;
        st.paint_left = 0;
        if (st.dirty_streak >= c.damage_threshold) st.hot_left = c.damage_duration;
    } else {
        st.static_frames++;
        st.dirty_streak = 0;
        if (st.hot_left > 0) st.hot_left--;
        if (c.use_paint_over && !st.painted && st.static_frames >= c.paint_over_trigger && st.hot_left == 0) {
            st.painted = true;
            st.paint_left = c.paint_over_burst;
        }
    }
    bool paint = false;
    if (!d && st.paint_left > 0) {
        paint = true;
        st.paint_left--;
    }
    t.qp = paint ? c.paint_qp : c.qp;
    const bool need_idr = ff ? pic.need_idr : st.need_idr;
    if (need_idr) {  // a keyframe counts as a change for paint-over purposes
        st.painted = false;
        st.static_frames = 0;
        t.action = ACT_I;
        t.allow_scenecut = 0;
    } else if (d || paint || st.hot_left > 0 || c.streaming_mode) {
        t.action = ACT_P;
    } else {
        t.action = ff ? ACT_SKIPALL : ACT_NONE;
    }
    if (ff) {
        t.frame_num = need_idr ? 0 : pic.frame_num;
        t.idr_pic_id = pic.idr_pic_id;
        if (need_idr) t.idr_on_intra = 1;
    } else {
        if (need_idr) t.idr_on_intra = 1;
        t.frame_num = st.frame_num;
        t.idr_pic_id = st.idr_pic_id;
    }
    const int refs = ff ? pic.refs : st.refs;
    t.num_refs = refs < 1 ? 1 : (refs < c.num_refs ? refs : c.num_refs);
    t.final_action = t.action;
}

// Striped mode: stripe state after its slice was coded with `final_action`.
// `idr`: an I slice was an IDR picture (always, unless the long-term cache keeps it a non-IDR I picture,
// whose frame_num advances as for P).
SK_HD void commit_stripe(StripeState& st, int final_action, int max_refs, bool idr = true) {
    if (final_action == ACT_I && idr) {
        st.frame_num = 1;
        st.idr_pic_id = (st.idr_pic_id + 1) & 0xffff;
        st.need_idr = false;
        st.refs = 1;
    } else if (final_action == ACT_P || final_action == ACT_I) {
        st.frame_num = (st.frame_num + 1) & kFrameNumMask;
        st.refs = st.refs + 1 < max_refs ? st.refs + 1 : max_refs;
    }
}

// Full-frame mode: picture state after a picture (IDR iff every slice was an IDR slice).
SK_HD void commit_picture(StripeState& pic, bool idr, int max_refs) {
    if (idr) {
        pic.frame_num = 1;
        pic.idr_pic_id = (pic.idr_pic_id + 1) & 0xffff;
        pic.need_idr = false;
        pic.refs = 1;
    } else {
        pic.frame_num = (pic.frame_num + 1) & kFrameNumMask;
        pic.refs = pic.refs + 1 < max_refs ? pic.refs + 1 : max_refs;
    }
}

// ---- long-term cache (ltr.h) over a stream's SliceTasks: slices [s0, s1) of one decoder ----
// Whether a gated frame takes slice t's zero-vector SADs: the slices planned as P; LTR_BUFMAP:
// every slice, the tile row is the unit and its clean slices count too.
SK_HD bool ltr_slice_compared(const ltr::LtrConfig& c, const SliceTask& t) {
    return c.mode == ltr::LTR_BUFMAP || t.action == ACT_P;
}

// The stream's decision for one frame, between planning and motion search. `dirty`: changed
// macroblocks of the stream; `gated`: `sad` ([slice][kLtrSadCols]) holds this frame's sums
// of the compared slices. Fills lt[s0..s1) and gives a matched H.264 slice its second reference.
SK_HD void ltr_stream_decide(const ltr::LtrConfig& c, ltr::LtrState& st, SliceTask* tasks, int s0, int s1, int dirty,
                             int mb_w, bool gated, uint32_t* sad, ltr::LtrTask* lt) {
    bool key = false, anyp = false;
    int rows = 0;
    for (int s = s0; s < s1; s++) {
        key |= tasks[s].action == ACT_I;
        anyp |= tasks[s].action == ACT_P;
        rows += tasks[s].num_rows;
    }
    if (c.mode == ltr::LTR_RPS) ltr::ltr_expire(c.slots, st, tasks[s0].frame_num, c.max_age);
    if (c.mode == ltr::LTR_BUFMAP && gated)   // one sum per tile row, so its slices match the same slot
        ltr::ltr_sum_units(c.slots, st.valid, s0, s1, c.unit_slices, sad);
    ltr::ltr_decide(c.slots, st, dirty, rows * mb_w, anyp && !key, tasks[s0].frame_num, kFrameNumMask, s0, s1,
                    [&](int s) { return ltr_slice_compared(c, tasks[s]); }, sad, lt);
    if (c.mode == ltr::LTR_BUFMAP)   // one slot per frame; ref1_mbs of every slice, clean ones included
        ltr::ltr_av1_reduce(c.slots, s0, s1, [&](int s) { return tasks[s].num_rows * mb_w; }, lt);
    if (c.mode == ltr::LTR_SECOND_REF)
        for (int s = s0; s < s1; s++)
            if (lt[s].slot >= 0) tasks[s].num_refs = 2;   // [previous picture, the slot]
}

// The stream's state after its picture was coded. A picture's stream (`fullframe`; HEVC and
// AV1 always) always codes one, an IDR or key frame when `picture_idr`; a stripe's says so itself.
SK_HD void ltr_stream_commit(const ltr::LtrConfig& c, ltr::LtrState& st, const SliceTask* tasks, const ltr::LtrTask* lt,
                             int s0, int s1, int mb_w, int num_mbs, bool fullframe, bool picture_idr) {
    const SliceTask& t = tasks[s0];
    if (fullframe) ltr::ltr_commit(c, st, true, picture_idr, t.frame_num, num_mbs, s0, s1, lt);
    else
        ltr::ltr_commit(c, st, t.final_action != ACT_NONE, t.final_action == ACT_I && t.idr_on_intra, t.frame_num,
                        t.num_rows * mb_w, s0, s1, lt);
}

struct MeResult;

// K10 frame QP from per-slice complexity sums (sad: motion-compensated SAD of the
// slice's MBs, dev: their source activity; both only for slices planned as P, where
// the motion search ran). Same code for the CPU controller and k_rc_qp.
SK_HD void rc_apply(RcState& rc, SliceTask* tasks, const long long* sad, const long long* dev, int ns, int mb_w,
                    int plan_qp, int stride = 1) {
    if (rc.mode == RC_CQP) return;
    long long cp = 0, ci = 0;
    int np = 0, ni = 0, ni_known = 0, nidr = 0;
    for (int s = 0; s < ns; s++) {
        const SliceTask& t = tasks[s];
        if (!rc_slice_adjustable(t, plan_qp, rc.mode)) continue;
        const int mbs = t.num_rows * mb_w;
        if (t.final_action == ACT_P) {
            cp += sad[(size_t)s * stride];
            np += mbs;
        } else {
            ni += mbs;
            if (t.action == ACT_I) nidr += mbs;   // planned key frame (IDR), not a scene cut
            {   // scene cut (ME's intra estimate) or planned key frame (MB activity, no search)
                ci += dev[(size_t)s * stride];
                ni_known += mbs;
            }
        }
    }
    if (np + ni == 0) return;
    const bool intra = ni > np;
    const int qpf = intra ? rc_frame_qpf(rc, ci, ni_known, true, nidr * 2 > ni, np + ni)
                          : rc_frame_qpf(rc, cp, np, false, false, np + ni);
    for (int s = 0, i = 0; s < ns; s++)
        if (rc_slice_adjustable(tasks[s], plan_qp, rc.mode)) tasks[s].qp = rc_clamp_qp(rc, rc_dither_qp(qpf, i++));
}

// K10 CBR guard on a coded frame of `frame_bits` payload bits: when it overflows the
// VBV, every rate-controlled slice (coded at the frame QP) moves rc_redo_step coarser
// for a second coding pass. Returns the step applied (0: keep the frame).
SK_HD int rc_redo(RcState& rc, SliceTask* tasks, int ns, long long frame_bits) {
    const int step = rc_redo_step(rc, frame_bits);
    if (!step) return 0;
    const int f0 = rc.cur_qpf, f1 = sk_min(f0 + (step << 8), rc.qp_max << 8);
    rc_raise_floor(rc);
    if (f1 == f0) return 0;
    rc.redo_qpf = f0;   // the pass being replaced: a slope for a further step and the model point
    rc.redo_bits = (int32_t)(frame_bits > (1ll << 30) ? (1ll << 30) : frame_bits);
    // the frame's slices sit at the two QPs of its dither (rc_dither_qp)
    const int lo = f0 >> 8, hi = (f0 + 255) >> 8;
    for (int s = 0; s < ns; s++) {
        SliceTask& t = tasks[s];
        if ((t.final_action == ACT_P || t.final_action == ACT_I) && (t.qp == lo || t.qp == hi))
            t.qp = rc_clamp_qp(rc, t.qp + step);
    }
    rc.cur_qpf = f1;
    rc.cur_qp = (f1 + 128) >> 8;
    rc.lam_boost = rc_lam_boost(f1);
    rc.redos++;
    rc.cur_redo++;
    return (f1 - f0 + 255) >> 8;
}

// Decides, per stripe, what to encode this frame.
class Controller {
   public:
    void init(const EncoderConfig& cfg, const Geometry& g);
    void request_keyframe();
    // Rate control: QP for changed stripes / paint-over from the next frame on.
    void set_qp(int qp, int paint_qp) {
        if (qp > 0) cfg_.qp = rc_.base_qp = qp;
        if (paint_qp > 0) cfg_.paint_qp = paint_qp;
    }
    // K10: mode (RC_CQP / RC_CRF / RC_CBR) and CBR bitrate from the next frame on.
    void set_rate(int mode, int kbps) {
        const RcState old = rc_;
        rc_init(rc_, mode, cfg_.qp, kbps, cfg_.fps, cfg_.width * cfg_.height, cfg_.vbv_ms, old.codec);
        if (old.mode == mode) {   // keep the model; a new budget recentres the buffer
            for (int k = 0; k < 2; k++) {
                rc_.last_qp[k] = old.last_qp[k];
                rc_.last_qpf[k] = old.last_qpf[k];
                rc_.last_bits[k] = old.last_bits[k];
                rc_.last_cplx[k] = old.last_cplx[k];
            }
            rc_.cplx_ema = old.cplx_ema;
        }
    }
    // K10 per frame: QP of the coded, non-paint-over slices from the frame complexity
    // (after motion search / scene cut), then the coded size.
    void rate_control(SliceTask* tasks, const MeResult* me);
    void rate_account(long long frame_bits) { rc_account(rc_, frame_bits); }
    int rate_redo(SliceTask* tasks, long long frame_bits) { return rc_redo(rc_, tasks, g_.num_slices, frame_bits); }
    RcState& rc() { return rc_; }
    // dirty[s] = stripe s changed since last frame. Fills tasks[num_slices].
    void plan(const uint8_t* dirty, SliceTask* tasks);
    // After the backend ran: update frame_num / idr state from final actions.
    void commit(const SliceTask* tasks);
    bool picture_is_idr(const SliceTask* tasks) const;
    const std::vector<StripeState>& stripes() const { return st_; }
    std::vector<StripeState>& stripes() { return st_; }
    // Session-state transfer (EncoderState): committed stripe states + picture state.
    void export_states(StripeState* out) const {
        for (size_t s = 0; s < st_.size(); s++) out[s] = st_[s];
        out[st_.size()] = pic_;
    }
    void import_states(const StripeState* in) {
        for (size_t s = 0; s < st_.size(); s++) st_[s] = in[s];
        pic_ = in[st_.size()];
    }
    int qp() const { return cfg_.qp; }
    int paint_qp() const { return cfg_.paint_qp; }

   private:
    EncoderConfig cfg_;
    Geometry g_;
    std::vector<StripeState> st_;
    StripeState pic_;  // full-frame mode picture state
    RcState rc_;
};


// ---- bitstream packaging (host) -------------------------------------------
int choose_level_idc(int mb_w, int mb_h, float fps, int dpb_frames = 0);
// SPS + PPS NAL units (Annex-B, with start codes) for a picture of w x h pixels.
void build_parameter_sets(int width, int height, int full_range, float fps,
                          std::vector<uint8_t>& out, int num_refs = 1, int ltr_slots = 0);
// Appends start code + NAL header + EP-escaped payload.
void append_nal(std::vector<uint8_t>& out, int nal_header_byte, const uint8_t* rbsp, size_t n);
size_t emulation_prevent(const uint8_t* in, size_t n, uint8_t* out);
// 10-byte 0x04 stripe header (selkies-core.js:2925-2938)
void write_stripe_header(uint8_t* p, int key, uint16_t frame_id, int y, int w, int h);

}  // namespace h264
}  // namespace sk

#include "h264_state.h"   // session state transfer: the blob's layout
