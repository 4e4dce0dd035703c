// Session state transfer: a portable snapshot of everything that carries over from one frame
// to the next, identical for every codec and for the CPU and HIP back ends, so a session can
// move between GPUs, or between a GPU and the CPU reference, without an IDR (parallel/migrate.py).
// The blob, in order:
//   StateHeader | StripeState[num_slices + 1] (committed controller state; the last is the
//   picture's, whose frame_num is also the next HEVC POC) | RcState (K10) | ref Y U V |
//   ref1 Y U V (second reference) | last source Y U V (damage baseline) | mvfield int16[2 * num_mbs]
// The reference planes are what the next frame predicts from (HEVC: after deblocking + SAO,
// AV1: after loop filter + CDEF). That is version 3. With the long-term cache on
// (ltr_slots > 0; AV1: LtrState holds the buffer map) the blob is version 4: the version-3 layout, then
//   LtrState[num_slices + 1] (last = the picture's, full-frame mode) | slot 0 Y U V | slot 1 Y U V | ...
// state_sections() below is this list as code; sizes and all four walkers (CPU and HIP, export
// and import) come from it.
#pragma once
#include "h264_encoder.h"

namespace sk {
namespace h264 {

struct StateHeader {
    char magic[4];          // "SKH4"
    int32_t version;        // 3 (codec, RcState); 4 = 3 + long-term cache (EncoderConfig::ltr_slots > 0)
    int32_t W, H, stripe_height, fullframe, num_slices;
    int32_t started;        // a frame has been encoded (else the next one is all-dirty)
    int32_t qp, paint_qp;   // rate-control QPs in force
    int32_t codec;          // EncoderConfig::codec
    int32_t ltr_slots;      // version 4: slot plane sets that follow (0 in version 3, where the word was reserved)
    int32_t reserved[4];
};
static_assert(sizeof(StateHeader) == 64, "StateHeader layout");

enum StateKind { ST_HEADER, ST_STRIPES, ST_RC, ST_REF, ST_REF1, ST_SRC, ST_MVFIELD, ST_LTR_STATE, ST_LTR_SLOT };
struct StateSection {
    StateKind kind;
    int plane;   // 0..2 = Y U V of the plane kinds (ST_REF, ST_REF1, ST_SRC, ST_LTR_SLOT)
    int slot;    // ST_LTR_SLOT: slot j
    size_t off, bytes;
};

// Calls f(section) for every section of the blob, in blob order; returns the blob's size.
template <class F>
inline size_t state_sections(const Geometry& g, int ltr_slots, F&& f) {
    size_t off = 0;
    auto put = [&](StateKind kind, size_t bytes, int plane = 0, int slot = 0) {
        f(StateSection{kind, plane, slot, off, bytes});
        off += bytes;
    };
    auto planes = [&](StateKind kind, int slot = 0) {
        for (int p = 0; p < 3; p++)
            put(kind, p ? (size_t)g.stride_c * g.plane_h_c : (size_t)g.stride_y * g.plane_h_y, p, slot);
    };
    put(ST_HEADER, sizeof(StateHeader));
    put(ST_STRIPES, sizeof(StripeState) * (size_t)(g.num_slices + 1));
    put(ST_RC, sizeof(RcState));
    planes(ST_REF);
    planes(ST_REF1);
    planes(ST_SRC);
    put(ST_MVFIELD, sizeof(int16_t) * 2 * (size_t)g.num_mbs());
    if (ltr_slots > 0) {
        put(ST_LTR_STATE, sizeof(ltr::LtrState) * (size_t)(g.num_slices + 1));
        for (int j = 0; j < ltr_slots; j++) planes(ST_LTR_SLOT, j);
    }
    return off;
}
inline size_t state_bytes(const Geometry& g, int ltr_slots = 0) {
    return state_sections(g, ltr_slots, [](const StateSection&) {});
}
inline size_t state_head_bytes(const Geometry& g) {   // header + controller + rate control
    size_t n = 0;
    state_sections(g, 0, [&](const StateSection& s) { n += s.kind <= ST_RC ? s.bytes : 0; });
    return n;
}

inline void state_header(const EncoderConfig& c, const Geometry& g, int started, int qp, int paint_qp,
                         StateHeader& h) {
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, "SKH4", 4);
    h.version = ltr_slots_of(c) > 0 ? 4 : 3;
    h.ltr_slots = ltr_slots_of(c);
    h.codec = c.codec;
    h.W = g.W;
    h.H = g.H;
    h.stripe_height = c.stripe_height;
    h.fullframe = c.fullframe;
    h.num_slices = g.num_slices;
    h.started = started;
    h.qp = qp;
    h.paint_qp = paint_qp;
}
inline bool state_header_matches(const EncoderConfig& c, const Geometry& g, const StateHeader& h) {
    return memcmp(h.magic, "SKH4", 4) == 0 && h.version == (ltr_slots_of(c) > 0 ? 4 : 3) &&
           h.ltr_slots == ltr_slots_of(c) && h.codec == c.codec && h.W == g.W && h.H == g.H &&
           h.stripe_height == c.stripe_height && h.fullframe == c.fullframe && h.num_slices == g.num_slices;
}

// The CPU encoder's state into / out of a host blob of state_bytes(e.g, e.ltr_cfg.slots) bytes
// (h264_cpu.cpp). HEVC / AV1 keep all their inter-frame state in the shared front end, itself a
// CpuH264Encoder. Import returns false, and changes nothing, when the header does not match.
class CpuH264Encoder;
void cpu_export_state(CpuH264Encoder& e, void* dst);
bool cpu_import_state(CpuH264Encoder& e, const void* src);

}  // namespace h264
}  // namespace sk
