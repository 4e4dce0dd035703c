// Device-side buffers and launch interface of the HIP H.264 pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include "../codec/overlay.h"
#include "../codec/h264_encoder.h"
#include "../codec/h264_frame.h"
#include "../codec/h264_deblock.h"

namespace sk {
namespace h264 {
namespace gpu {

constexpr int kMbSlotBytes = 1024;     // per-MB CAVLC bit buffer (A.3.1 caps a MB at 400 B)
constexpr int kSliceHdrMax = 64;       // SPS+PPS+stripe header prefix room per slot
constexpr int kPackMaxSliceMbs = 16384;   // k_slice_pack: macroblocks of one slice (16 MB rows of an 8K picture: 8192)

struct Planes {
    uint8_t* y;
    uint8_t* u;
    uint8_t* v;
};

// Everything a kernel needs, passed by value (pointers are device memory).
// One struct for all codecs of the HIP back end. The buffers of the H.264 coding chain (mbs,
// coefs, mb_bits, mb_nbits, slice_info, param_sets, param_set_len, host_out, host_size,
// cavlc_tabs, aq, db, dbe) are allocated by the H.264 tail alone (runtime/h264_tail.h) and null
// in HEVC and AV1 sessions: the kernels those launch (launch_convert_damage, launch_frontend,
// launch_rc_account, launch_rc_guard_sizes, k_commit without `account` and with deblock 0)
// must not touch them.
struct FrameArgs {
    int W, H, mb_w, mb_h, stride_y, stride_c, num_slices, rows_per_slice, fullframe;
    int full_range, me_range, me_iters;
    const uint8_t* bgrx;   // device copy of the captured frame
    int bgrx_stride;
    int scaled;            // K2: resample the capture (src_w x src_h) to W x H inside K1
    ScaleParams scale;
    Planes src, prev, ref, rec;
    Planes ref1;           // second reference (previous-but-one picture), num_refs == 2
    uint8_t* mb_dirty;     // [num_mbs]
    int* stripe_dirty;     // [num_slices] set by k_convert_damage, consumed (and cleared) by k_plan
    StripeState* plan_state;    // [num_slices + 1] controller state (last = picture state)
    int* plan_ctl;              // [0] keyframe requests seen, [1] frames planned (0 = first frame)
    const int* key_seq_host;    // host-mapped: [0] keyframe request counter, [1] qp, [2] paint qp (0 = config)
    int* key_dev;               // [6] device copy of the snapshot, left by the damage kernel (read by k_plan, k_rc_qp)
    PlanConfig plan_cfg;
    SliceTask* tasks;      // [num_slices]
    MeResult* me;          // [num_mbs]
    int16_t* mvfield;      // [num_mbs][2]
    MbInfo* mbs;           // [num_mbs]
    int16_t* coefs;        // [num_mbs][kCoefPerMb]
    uint32_t* mb_bits;     // [num_mbs][kMbSlotBytes/4]
    int* mb_nbits;         // [num_mbs]
    int* slice_info;       // [num_slices * nal_per_slice][4]: RBSP bytes, packet prefix bytes (k_slice_pack)
    int out_slot_bytes;    // bytes per slice slot in host_out
    const uint8_t* param_sets;  // [num_slices or 1][kParamSetMax]
    const int* param_set_len;
    int param_set_stride;
    uint8_t* host_out;     // host-mapped packet slots [num_slices][out_slot_bytes]
    int* host_size;        // host-mapped [num_slices] bytes in each slot
    int* frame_params_dev;           // device: [0] = frame_id (loaded by the damage kernel)
    const int* frame_params_host;    // host-mapped source
    SliceTask* tasks_host;           // host-mapped: final slice decisions (written by k_decide)
    unsigned long long* dbg;  // optional s_memtime stamps (SK_STAMPS=1), else nullptr
    const CavlcTables* cavlc_tabs;  // precomputed CAVLC tables (device memory), copied to LDS per WG
    int num_refs;          // EncoderConfig::num_refs (1 or 2)
    int deblock;           // K7 on: ref = deblocked rec (k_deblock), else k_commit copies rec
    int me_full;           // K4a on: MFMA exhaustive-search candidate per dirty MB
    int aq_strength;       // MB-level adaptive QP strength (Q4), 0 = off
    int subpel;            // K4c quarter-pel refinement (k_subpel) before K6
    int intra4x4;          // I slices may code I_NxN macroblocks (the pre-pass in k_code_inter decides, k_code_intra codes)
    const uint8_t* ov_img[kOverlaySlots];   // K12/K13 overlay images (premultiplied BGRA)
    const OverlayParams* ov;                // [kOverlaySlots] placement of this frame (device copy)
    int8_t* aq;            // [num_mbs] AQ offsets (k_aq), valid for MBs of coded slices
    DbInfo* db;            // [num_mbs] deblocking side info (k_deblock_prep)
    uint4* dbe;            // [num_mbs][3] per-MB edge record: bS nibbles, packed filter params (k_deblock_edges)
    int16_t* fs_mv;        // [num_mbs][2] MFMA full-search winner (integer pel)
    RcState* rc;           // K10 rate-control state (ratecontrol.h), device
    long long* rc_slice;   // [num_slices][2] complexity sums of P-planned slices (SAD, activity)
    float rc_fps;          // session frame rate (CBR frame budget)
    int* rc_redo;          // K10 CBR guard: device flag, 1 = code the frame again (k_rc_guard)
    // K5 sub-slices (h264_encoder.h intra_split): NAL slots per slice. slice_info is indexed
    // by NAL (slice * nal_per_slice + sub-slice).
    int nal_per_slice;
    const int* gate;       // second-pass launches: run only when *gate != 0 (null: always)
    // planar 4:2:0 input (YuvInput, h264_frame.h) staged on the device: W x H luma (pitch
    // W), then I420 U and V ((W+1)/2 x (H+1)/2 each) or NV12 interleaved UV (pitch
    // 2 * ((W+1)/2)); yuv_fmt 0: BGRx input through k_convert_damage
    const uint8_t* yuv;
    int yuv_fmt;
    // Long-term reference cache (codec/ltr.h), ltr_cfg.slots > 0. Slot j's planes lie at
    // ltr.y + j * ltr_ny and ltr.u / ltr.v + j * ltr_nc (a stripe's slot at the stripe's rows).
    ltr::LtrConfig ltr_cfg;     // ltr_config_of(cfg), as the CPU back end holds it
    Planes ltr;
    size_t ltr_ny, ltr_nc;
    ltr::LtrState* ltr_state;   // [num_slices + 1] per stream (last = the picture's, full-frame mode)
    ltr::LtrTask* ltr_task;     // [num_slices] this frame's decisions
    uint32_t* ltr_part;         // [num_slices][kLtrSadCols][rows_per_slice] zero-vector SADs per MB row (k_ltr_match)
    uint32_t* ltr_sad;          // [num_slices][kLtrSadCols] their sums (k_ltr_decide)
    int* ltr_cnt;               // [num_slices][2] the slice's stream: dirty MBs, SADs computed (gated frame)
};

#if defined(__HIPCC__)
// Reference index 0 of slice s: the previous picture, or in the exclusive modes (HEVC and AV1, ltr.h) the
// cached picture a matched slice predicts from. s must be wave-uniform: the slot index goes
// through readfirstlane, so the three base pointers are scalars (no per-lane select, no
// indexed Planes array, which would live in scratch).
__device__ __forceinline__ Planes ref0_planes(const FrameArgs& a, int s) {
    if (a.ltr_cfg.mode == ltr::LTR_SECOND_REF) return a.ref;
    const int j = __builtin_amdgcn_readfirstlane(a.ltr_task[s].slot);
    if (j < 0) return a.ref;
    return Planes{a.ltr.y + (size_t)j * a.ltr_ny, a.ltr.u + (size_t)j * a.ltr_nc, a.ltr.v + (size_t)j * a.ltr_nc};
}
#endif

// K1 + K3, or k_yuv_damage for planar input. Also fetches the frame's host-mapped words
// (key_seq_host, frame_params_host) into key_dev / frame_params_dev, which k_plan and the
// kernels after it read: every codec calls it first, ahead of launch_frontend / launch_encode.
void launch_convert_damage(const FrameArgs& a, hipStream_t s);
// k_plan and everything after it; guard: CBR overflow guard + gated second coding pass
void launch_encode(const FrameArgs& a, hipStream_t s, bool guard = false);
// k_plan, motion search and scene-cut decisions only (the HEVC back end follows it)
void launch_frontend(const FrameArgs& a, hipStream_t s);
// MV field + reference update (+ K7 deblocking). filter = false leaves the three deblocking
// kernels out: for frames in which no slice can be filtered (slice_deblock false for every
// slice, see max_slice_qp in h264_encoder.h), where they would only exit.
// account: the H.264 chain's K10 accounting (the NAL sizes k_slice_pack left in slice_info)
// runs in the first workgroup of k_commit; the HEVC / AV1 back ends use launch_rc_account.
void launch_commit(const FrameArgs& a, hipStream_t s, bool filter = true, bool account = false);
// K10 accounting of the frame just coded: frame bytes = sum of sizes[i * stride],
// i < n (per_slice: only slices that were coded).
void launch_rc_account(const FrameArgs& a, const int* sizes, int n, int stride, int per_slice, hipStream_t s);
// K10 per-frame cap of a back end whose payload is the sum of n byte counts (HEVC / AV1);
// chained: the check after a re-code pass (runs only when *redo is up)
void launch_rc_guard_sizes(const FrameArgs& a, const int* sizes, int n, int* redo, bool chained, hipStream_t s);

}  // namespace gpu
}  // namespace h264
}  // namespace sk
