// HIP back end of the stripe encoders: H.264, and HEVC and AV1 on the same front end. Owns
// the per-session HBM buffers, the stream and pinned staging, and drives the gfx950 kernels
// (csrc/kernels/h264_kernels.hip, hevc_kernels.hip, av1_kernels.hip). Frame flow of H.264:
//   H2D(BGRx) -> (overlay placement, only when it changed) -> [k_convert_damage, k_plan (stripe
//   controller on the GPU), k_me, k_decide, k_rc_qp, k_subpel, inter / intra coding, k_cavlc,
//   k_slice_pack into host-mapped packet slots] (one hipGraph per parity slot)
//   -> one sync -> packets; behind it, not waited on: k_commit with the K10 accounting (+ K7
//   deblocking when a slice of the frame can be filtered), a second graph. No host decision sits
//   inside a frame. HEVC and AV1 run the same front end (up to k_subpel), then their own back ends.
#include "encoder_iface.h"
#include "trace.h"
#include "hip_util.h"
#include "../kernels/h264_gpu.h"
#include "../kernels/hevc_gpu.h"
#include "../kernels/av1_gpu.h"
#include "../codec/av1_encoder.h"
#include "../kernels/runtime_kernels.h"
#include "../codec/hevc_encoder.h"
#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <thread>

namespace sk {
namespace {

using namespace h264;

// Everything that belongs to one frame in flight. Frame k uses slot k & 1: its upload overlaps
// the other slot's graph, and the host reads its packets while the other slot's frame encodes.
struct FrameSlot {
    uint8_t* bgrx = nullptr;   // input frame
    uint8_t* yuv = nullptr;    // planar input staging (upload_yuv)
    gpu::Planes src = {};      // converted source; `prev` of the next frame
    bool up_valid = false;     // bgrx holds a complete frame (upload_copy)
    uint16_t frame = 0;        // frame id of the launched frame
    // host-mapped: packet slots and their sizes, final decisions from k_decide, frame id for
    // k_plan, and the key-frame / QP / rate snapshot taken at launch
    Mapped<uint8_t> out;
    Mapped<int> out_size;
    Mapped<SliceTask> tasks;
    Mapped<int> frame_params, key_snap;
    // HEVC: host-mapped slice slots + device fallback; AV1: frame info and tile bytes (null otherwise)
    Mapped<uint8_t> hevc_out, av1_out;
    Mapped<int> hevc_size, av1_size, av1_frame;
    uint8_t* hevc_fallback = nullptr;
    hipEvent_t uploaded = nullptr, started = nullptr, packets_done = nullptr;   // stage_times()
    hipEvent_t copied = nullptr;   // upload on another stream than the encoder's
    // part 0 (frame -> packets), part 1 (commit + deblocking), part 1 without the deblocking kernels
    hipGraphExec_t graph = nullptr, post = nullptr, post_short = nullptr;
};

class HipBackend : public EncoderBackend {
   public:
    HipBackend(const EncoderConfig& c, int device) : cfg_(c), device_(device) {
        if (cfg_.codec == 2) av1::cbr_config(cfg_);   // AV1 CBR as the CPU encoder (av1_encoder.h)
        if (cfg_.codec == 1) {   // HEVC: CBR without scene-cut intra slices, stripes of whole CTB rows (hevc_encoder.h)
            hevc::cbr_config(cfg_);
            hevc::hevc_geometry(cfg_);
        }
        g_.init(cfg_);
        ctl_.init(cfg_, g_);
        HIPCHECK(hipSetDevice(device_));
        warm_copy_engines(device_);
        HIPCHECK(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
        mem_.stream = stream_;
        for (auto& f : slot_) {
            for (hipEvent_t* e : {&f.uploaded, &f.started, &f.packets_done}) HIPCHECK(hipEventCreate(e));
            HIPCHECK(hipEventCreateWithFlags(&f.copied, hipEventDisableTiming));
        }
        if (cfg_.shared_copy) copy_stream_ = device_copy_stream(device_);
        alloc();
        if (cfg_.codec == 1) alloc_hevc();
        if (cfg_.codec == 2) alloc_av1();
        build_debug_table();
    }
    ~HipBackend() override {
        hipSetDevice(device_);
        // a launched, uncollected frame may still replay the graphs and read the buffers freed
        // below, and an overlapped upload may still write an input buffer
        hipStreamSynchronize(stream_);
        if (up_stream_) hipStreamSynchronize(up_stream_);
        for (auto& f : slot_)   // an upload on the device's shared copy stream, which outlives this encoder
            if (f.copied) hipEventSynchronize(f.copied);
        invalidate_graphs();
        mem_.free_all();
        for (auto& f : slot_)
            for (hipEvent_t e : {f.uploaded, f.started, f.packets_done, f.copied})
                if (e) hipEventDestroy(e);
        if (ev_ext_) hipEventDestroy(ev_ext_);
        for (auto& f : slot_)
            if (f.bgrx) hipFree(f.bgrx);
        hipStreamDestroy(stream_);
        if (up_stream_) hipStreamDestroy(up_stream_);
    }

    // Picked up by k_plan at the start of the next frame.
    void request_keyframe() override { __atomic_fetch_add(h_key_seq_, 1, __ATOMIC_SEQ_CST); }
    // Host-mapped overrides, read by k_plan at the start of the next frame.
    void set_qp(int qp, int paint_qp) override {
        if (qp > 0) __atomic_store_n(&h_key_seq_[1], qp, __ATOMIC_SEQ_CST);
        if (paint_qp > 0) __atomic_store_n(&h_key_seq_[2], paint_qp, __ATOMIC_SEQ_CST);
    }
    // K10: picked up by k_plan at the next frame (a change counter tells it apart).
    void set_rate(int mode, int kbps) override {
        cfg_.rc_mode = mode;   // graphs re-captured with / without the CBR guard (launch)
        __atomic_store_n(&h_key_seq_[3], mode, __ATOMIC_SEQ_CST);
        __atomic_store_n(&h_key_seq_[4], kbps, __ATOMIC_SEQ_CST);
        __atomic_fetch_add(&h_key_seq_[5], 1, __ATOMIC_SEQ_CST);
    }
    int64_t rc_stats(int32_t* out, int n) override {
        HIPCHECK(hipSetDevice(device_));
        HIPCHECK(hipStreamSynchronize(stream_));
        RcState rc;
        copy_now(&rc, args_.rc, sizeof(rc));
        const int k = n < (int)(sizeof(rc) / 4) ? n : (int)(sizeof(rc) / 4);
        memcpy(out, &rc, (size_t)k * 4);
        return k;
    }

    // finish() returns the oldest frame in flight: with one uncollected, encode() and encode_yuv()
    // would hand back that frame's packets and leave the new frame behind, so they are refused.
    bool refuse_inflight(const char* call) {
        if (inflight() <= 0) return false;
        set_last_error(std::string(call) + ": a frame is in flight; finish() it first");
        return true;
    }

    int encode(const uint8_t* bgrx, int stride, uint16_t frame_id) override {
        if (refuse_inflight("encode()")) return -1;
        if (submit(bgrx, stride, frame_id) < 0) return -1;
        return finish();
    }

    int submit(const uint8_t* bgrx, int stride, uint16_t frame_id) override {
        if (upload(bgrx, stride, frame_id) < 0) return -1;
        return launch();
    }

    // Stage a frame: H2D into the input buffer of the frame's parity on the copy
    // stream. May be called while the previous frame is still encoding (its upload
    // then overlaps that frame's kernels); launch() comes after finish() of it.
    double upload_fraction() const override {
        const long long t = up_rows_total_.load();
        return t ? (double)up_rows_copied_.load() / (double)t : 1.0;
    }
    void set_upload_rows(const int* r, int n) override {
        up_next_known_ = n >= 0;
        up_next_.assign(r && n > 0 ? r : nullptr, r && n > 0 ? r + 2 * n : nullptr);
    }

    // Damage-driven upload: f.bgrx holds the frame uploaded two frames ago, so the
    // rows that changed since then (this frame's damage and the previous frame's) are
    // copied; everything else is already on the device. Full copy when either damage is
    // unknown, the buffer was never filled or the frame is scaled on the device.
    void upload_copy(FrameSlot& f, const uint8_t* bgrx, int stride, size_t in_bytes, hipStream_t cs) {
        const int rows = (int)(in_bytes / (size_t)stride);
        const bool partial = f.up_valid && up_next_known_ && up_prev_known_ && !args_.scaled;
        if (!partial) {
            HIPCHECK(hipMemcpyAsync(f.bgrx, bgrx, in_bytes, hipMemcpyDefault, cs));
        } else {
            // union of the two damage lists on 16-row bands, copied as maximal row ranges
            for (const auto& r : upload_ranges({&up_next_, &up_prev_}, rows)) {
                HIPCHECK(hipMemcpyAsync(f.bgrx + (size_t)r.first * stride, bgrx + (size_t)r.first * stride,
                                        (size_t)(r.second - r.first) * stride, hipMemcpyDefault, cs));
                up_rows_copied_ += r.second - r.first;
            }
        }
        if (!partial) up_rows_copied_ += rows;
        up_rows_total_ += rows;
        f.up_valid = true;
        up_prev_known_ = up_next_known_;
        up_prev_.swap(up_next_);
        up_next_known_ = false;   // one damage report per upload
        up_next_.clear();
    }

    // Planar input: the planes are staged (2D copies, H2D or D2D) into this parity's
    // staging buffer in the packed layout k_yuv_damage reads; the graphs are captured
    // per input kind (BGRx / I420 / NV12).
    int encode_yuv(const YuvInput& in, int on_device, uint16_t frame_id) override {
        if (refuse_inflight("encode_yuv()")) return -1;
        if (upload_yuv(in, on_device, frame_id) < 0) return -1;
        if (launch() < 0) return -1;
        return finish();
    }

    int upload_yuv(const YuvInput& in, int on_device, uint16_t frame_id) {
        trace::Range frame_range("h264.upload_yuv");
        HIPCHECK(hipSetDevice(device_));
        if (args_.scaled) {
            set_last_error("planar input cannot be resampled (src size != encoder size)");
            return -1;
        }
        if (inflight() >= 2) {
            set_last_error("upload(): two frames in flight; finish() the oldest first");
            return -1;
        }
        const int W = g_.W, H = g_.H, cw = (W + 1) / 2, ch = (H + 1) / 2;
        const size_t need = (size_t)W * H + (size_t)2 * cw * ch;
        if (!slot_[0].yuv || yuv_mode_ != in.fmt) {
            recapture([&] {
                if (!slot_[0].yuv)
                    for (auto& f : slot_) f.yuv = mem_.dmalloc<uint8_t>(need, false);
            });
            yuv_mode_ = in.fmt;
        }
        FrameSlot& f = slot_[launched_ & 1];
        HIPCHECK(hipEventRecord(f.uploaded, stream_));
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        uint8_t* d = f.yuv;
        HIPCHECK(hipMemcpy2DAsync(d, W, in.p[0], in.stride[0], W, H, k, stream_));
        if (in.fmt == YUV_NV12) {
            HIPCHECK(hipMemcpy2DAsync(d + (size_t)W * H, 2 * cw, in.p[1], in.stride[1], 2 * cw, ch, k, stream_));
        } else {
            HIPCHECK(hipMemcpy2DAsync(d + (size_t)W * H, cw, in.p[1], in.stride[1], cw, ch, k, stream_));
            HIPCHECK(hipMemcpy2DAsync(d + (size_t)W * H + (size_t)cw * ch, cw, in.p[2], in.stride[2], cw, ch, k,
                                      stream_));
        }
        drop_uploads();   // the BGRx buffers no longer hold the last frames
        staged_on_main_ = true;
        staged_ = true;
        staged_frame_ = frame_id;
        return 0;
    }

    int upload(const uint8_t* bgrx, int stride, uint16_t frame_id) override {
        trace::Range frame_range("h264.upload");
        HIPCHECK(hipSetDevice(device_));
        if (yuv_mode_) {   // back to BGRx input: graphs with k_convert_damage
            recapture([] {});
            yuv_mode_ = 0;
        }
        const size_t in_bytes = (size_t)stride * (args_.scaled ? args_.scale.src_h : g_.H);
        if (in_bytes > bgrx_cap_ || stride != args_.bgrx_stride) {
            recapture([&] {   // geometry change: drain, then reallocate
                if (in_bytes > bgrx_cap_) {
                    for (auto& f : slot_) {
                        if (f.bgrx) hipFree(f.bgrx);
                        HIPCHECK(hipMalloc(&f.bgrx, in_bytes));
                    }
                    bgrx_cap_ = in_bytes;
                }
                drop_uploads();
            });
            args_.bgrx_stride = stride;
        }
        if (inflight() >= 2) {
            set_last_error("upload(): two frames in flight; finish() the oldest first");
            return -1;
        }
        FrameSlot& f = slot_[launched_ & 1];   // parity this frame is launched with
        // A re-upload before launch (the staged frame was never launched) overwrites
        // f.bgrx again: the two-frames-ago invariant of upload_copy no longer holds
        // for either parity, so the next two uploads are full copies.
        if (staged_) drop_uploads();
        // Nothing in flight: copy on the encoder's own stream (no cross-stream wait).
        // Overlapped upload, or bands of one frame: the device's shared copy stream, so
        // the uploads of all encoders on this GPU run back to back at full PCIe rate
        // instead of contending (one copy queue, not one per session). Copies behind
        // kernels on one stream stall in a fresh process until warm_copy_engines() ran.
        hipStream_t cs = stream_;
        // Overlapped upload of a session: its own upload stream (the copies of many
        // sessions then spread over the SDMA engines; SK_SHARED_UPLOAD=1 funnels them
        // through the device's one shared copy stream instead).
        if (copy_stream_) cs = copy_stream_;
        else if (inflight() && upload_mode_ != 0) cs = upload_mode_ == 2 ? device_copy_stream(device_) : upload_stream();
        if (ext_wait_) {   // wait_stream(): the source is written by another stream's queued work
            HIPCHECK(hipStreamWaitEvent(cs, ev_ext_, 0));
            ext_wait_ = false;
        }
        // the last reader of f.bgrx is the graph two frames back: finished
        HIPCHECK(hipEventRecord(f.uploaded, cs));
        // hipMemcpyDefault: the frame may be host memory (capture) or device memory (a band
        // scattered to this GPU over RCCL, parallel/dist_banded.py)
        upload_copy(f, bgrx, stride, in_bytes, cs);
        if (cs != stream_) HIPCHECK(hipEventRecord(f.copied, cs));
        staged_on_main_ = cs == stream_;
        staged_ = true;
        staged_frame_ = frame_id;
        return 0;
    }

    int wait_stream(void* stream) override {
        HIPCHECK(hipSetDevice(device_));
        if (!ev_ext_) HIPCHECK(hipEventCreateWithFlags(&ev_ext_, hipEventDisableTiming));
        HIPCHECK(hipEventRecord(ev_ext_, (hipStream_t)stream));
        ext_wait_ = true;
        return 0;
    }

    int launch() override {
        if (!staged_ || inflight() >= 2) {
            set_last_error("launch() needs one uploaded frame and at most one frame in flight");
            return -1;
        }
        trace::Range frame_range("h264.launch");
        HIPCHECK(hipSetDevice(device_));
        parity_ = launched_ & 1;
        FrameSlot& f = slot_[parity_];
        if ((cfg_.rc_mode == RC_CBR) != graph_guard_) {   // K10 CBR guard in / out of the graphs
            recapture([] {});
            graph_guard_ = cfg_.rc_mode == RC_CBR;
        }
        set_parity_args();   // inputs and host outputs of slot f
        // host-mapped, read by this frame's k_plan: per parity, because with two frames
        // in flight the previous frame's k_plan may not have run yet
        f.frame_params.host[0] = staged_frame_;
        // keyframe request counter and QP overrides as of this launch: a request made
        // before launch(n) applies to frame n even when frame n-1 has not planned yet
        for (int i = 0; i < 6; i++) f.key_snap.host[i] = __atomic_load_n(&h_key_seq_[i], __ATOMIC_SEQ_CST);
        f.frame = staged_frame_;
        // Overlay placement of this frame: copied ahead of the graph, on the same stream (so
        // behind the previous frame's graph, which read the old placement), and only when it
        // differs from what the device holds; once more after the graphs were re-captured.
        if (ov_resend_ || memcmp(ov_sent_, ov_pending_, sizeof(ov_pending_)) != 0) {
            memcpy(ov_params_host_[ov_slot_], ov_pending_, sizeof(ov_pending_));
            HIPCHECK(hipMemcpyAsync(ov_params_dev_, ov_params_host_[ov_slot_], sizeof(ov_pending_),
                                    hipMemcpyHostToDevice, stream_));
            memcpy(ov_sent_, ov_pending_, sizeof(ov_pending_));
            ov_slot_ = (ov_slot_ + 1) % kOvStage;
            ov_resend_ = false;
        }
        if (!staged_on_main_) HIPCHECK(hipStreamWaitEvent(stream_, f.copied, 0));
        HIPCHECK(hipEventRecord(f.started, stream_));
        // convert/damage -> plan -> ME -> code -> CAVLC -> assembly -> commit: one graph,
        // one sync; k_decide leaves the final slice decisions in f.tasks.
        // MV field / reference update and K7 deblocking run after the packets are done:
        // the host only waits for packets_done; the next frame's work queues behind the update.
        // (An event record captured inside one fused graph did not order the host wait
        // after part 0 on ROCm 7: packets read back empty. Two launches it is.)
        run_graph(f.graph, 0);
        HIPCHECK(hipEventRecord(f.packets_done, stream_));
        // Part 1 without the deblocking kernels when no slice of this frame can be filtered.
        // H.264 only: HEVC and AV1 filter in their own back ends and replay part 1 as before.
        if (cfg_.codec != 0 || can_filter(f.key_snap.host)) run_graph(f.post, 1);
        else run_graph(f.post_short, 2);
        staged_ = false;
        launched_++;
        parity_ = launched_ & 1;
        return 0;
    }

    // Oldest frame in flight: wait for its packets. Up to two frames may be in flight
    // (launch(n+1) before finish(n)): the GPU then runs frame n+1's graph while the
    // host assembles frame n's packets, with no idle gap between the two graphs.
    int finish() override {
        if (inflight() <= 0) {
            set_last_error("finish() without a launched frame");
            return -1;
        }
        const FrameSlot& f = slot_[finished_ & 1];
        {
            trace::Range r("h264.wait");
            HIPCHECK(hipEventSynchronize(f.packets_done));
        }
        {
            trace::Range r("h264.packets");
            packets_.clear();
            build_packets(f);
        }
        finished_++;
        float t0 = 0, t1 = 0;
        hipEventElapsedTime(&t0, f.uploaded, f.started);
        hipEventElapsedTime(&t1, f.started, f.packets_done);
        stage_ms_[0] = t0;
        stage_ms_[1] = t1;
        return (int)packets_.size();
    }

    int64_t state_bytes() override { return (int64_t)h264::state_bytes(g_, args_.ltr_cfg.slots); }

    // Copies `n` bytes between this encoder's device buffer and a caller buffer
    // that is device (on_device) or host memory.
    void xfer(void* dst, const void* src, size_t n, bool to_caller, int on_device) {
        const hipMemcpyKind k = on_device ? hipMemcpyDeviceToDevice
                                          : (to_caller ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice);
        HIPCHECK(hipMemcpyAsync(dst, src, n, k, stream_));
    }

    int export_state(void* dst, int on_device) override {
        HIPCHECK(hipSetDevice(device_));
        HIPCHECK(hipStreamSynchronize(stream_));
        const PendingCommit pc = pending_commit();
        // the sections put together on the host: alive until the copies below are done
        StateHeader h;
        state_header(cfg_, g_, pc.started, h_key_seq_[1] > 0 ? h_key_seq_[1] : cfg_.qp,
                     h_key_seq_[2] > 0 ? h_key_seq_[2] : cfg_.paint_qp, h);
        const std::vector<StripeState> st = committed_stripes(pc);
        const std::vector<ltr::LtrState> ls = committed_ltr_state(pc);
        state_sections(g_, args_.ltr_cfg.slots, [&](const StateSection& s) {
            uint8_t* o = static_cast<uint8_t*>(dst) + s.off;
            const void* host = s.kind == ST_HEADER ? (const void*)&h
                               : s.kind == ST_STRIPES ? (const void*)st.data()
                               : s.kind == ST_LTR_STATE ? (const void*)ls.data() : nullptr;
            if (!host) xfer(o, section_dev(s), s.bytes, true, on_device);
            else if (on_device) HIPCHECK(hipMemcpyAsync(o, host, s.bytes, hipMemcpyHostToDevice, stream_));
            else memcpy(o, host, s.bytes);
        });
        HIPCHECK(hipStreamSynchronize(stream_));
        return 0;
    }

    int import_state(const void* src, int on_device) override {
        HIPCHECK(hipSetDevice(device_));
        HIPCHECK(hipStreamSynchronize(stream_));
        auto to_host = [&](void* d, const void* i, size_t n) {
            if (on_device) copy_now(d, i, n);
            else memcpy(d, i, n);
        };
        StateHeader h;
        to_host(&h, src, sizeof(h));
        if (!state_header_matches(cfg_, g_, h)) {
            set_last_error("encoder state does not match this encoder's geometry / codec");
            return -1;
        }
        RcState rc;   // alive until the copies below are done
        state_sections(g_, args_.ltr_cfg.slots, [&](const StateSection& s) {
            const uint8_t* i = static_cast<const uint8_t*>(src) + s.off;
            if (s.kind == ST_RC) {   // K10 state; its set_rate() counter is this encoder's, so k_plan keeps it
                to_host(&rc, i, sizeof(rc));
                rc.seq = __atomic_load_n(&h_key_seq_[5], __ATOMIC_SEQ_CST);
                dev_rc_mode_ = rc.mode;   // can_filter(): the device controller now runs in the imported mode
                dev_rc_seq_ = rc.seq;
                // launch(): graphs with the CBR guard exactly when the imported controller runs CBR (an
                // encoder created in another mode captured them without it and never coded a frame again)
                cfg_.rc_mode = rc.mode;
                HIPCHECK(hipMemcpyAsync(args_.rc, &rc, sizeof(rc), hipMemcpyHostToDevice, stream_));
            } else if (s.kind != ST_HEADER) {
                xfer(section_dev(s), i, s.bytes, false, on_device);
            }
        });
        // controller: committed state (2), and the host keyframe counter as already seen
        int ctl[2] = {__atomic_load_n(&h_key_seq_[0], __ATOMIC_SEQ_CST), h.started ? 2 : 0};
        HIPCHECK(hipMemcpyAsync(args_.plan_ctl, ctl, sizeof(ctl), hipMemcpyHostToDevice, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        __atomic_store_n(&h_key_seq_[1], h.qp, __ATOMIC_SEQ_CST);
        __atomic_store_n(&h_key_seq_[2], h.paint_qp, __ATOMIC_SEQ_CST);
        return 0;
    }

    int stage_times(float* dst, int n) override {
        int k = n < 2 ? n : 2;
        for (int i = 0; i < k; i++) dst[i] = stage_ms_[i] * 1000.f;
        return k;
    }

    int set_overlay_image(int slot, const uint8_t* bgra, int w, int h) override {
        if (slot < 0 || slot >= kOverlaySlots || w < 0 || h < 0 || w > kOverlayMaxDim || h > kOverlayMaxDim) return -1;
        HIPCHECK(hipSetDevice(device_));
        const size_t n = (size_t)w * h * 4;
        if (!ov_stage_) ov_stage_ = mem_.hmalloc<uint8_t>((size_t)kOverlayMaxDim * kOverlayMaxDim * 4);
        HIPCHECK(hipStreamSynchronize(stream_));   // frames in flight may still read the old image
        if (n) {
            memcpy(ov_stage_, bgra, n);
            HIPCHECK(hipMemcpyAsync(ov_img_dev_[slot], ov_stage_, n, hipMemcpyHostToDevice, stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
        }
        ov_pending_[slot].w = w;
        ov_pending_[slot].h = h;
        if (!n) ov_pending_[slot].on = 0;
        return 0;
    }
    int set_overlay_pos(int slot, int on, int x, int y, int tdx, int tdy) override {
        if (slot < 0 || slot >= kOverlaySlots) return -1;
        OverlayParams& o = ov_pending_[slot];
        o.on = on && o.w > 0 && o.h > 0;
        o.x = x;
        o.y = y;
        o.tdx = tdx > 0 ? tdx : 0;
        o.tdy = tdy > 0 ? tdy : 0;
        return 0;
    }

    int64_t debug_buffer(const char* name, void* dst, int64_t cap) override {
        HIPCHECK(hipSetDevice(device_));
        HIPCHECK(hipStreamSynchronize(stream_));
        const std::string s(name);
        auto from_host = [&](const void* src, size_t n) {
            if (dst && cap >= (int64_t)n) memcpy(dst, src, n);
            return (int64_t)n;
        };
        if (s == "tasks")   // of the last finished frame
            return from_host(slot_[(finished_ + 1) & 1].tasks.host, g_.num_slices * sizeof(SliceTask));
        if (s == "av1_geo" && cfg_.codec == 2) return from_host(&av1_geo_, sizeof(av1_geo_));
        if (s == "ltr_state" && args_.ltr_cfg.slots) {
            const std::vector<ltr::LtrState> ls = committed_ltr_state(pending_commit());
            return from_host(ls.data(), ls.size() * sizeof(ltr::LtrState));
        }
        const void* p = nullptr;
        int64_t n = 0;
        const int64_t ny = (int64_t)g_.stride_y * g_.plane_h_y, nc = (int64_t)g_.stride_c * g_.plane_h_c;
        // after a frame the parity flipped: the last source is in `prev` of the next frame
        const gpu::Planes& last_src = slot_[parity_ ^ 1].src;
        if (s == "src_y") { p = last_src.y; n = ny; }
        else if (s == "src_u") { p = last_src.u; n = nc; }
        else if (s == "src_v") { p = last_src.v; n = nc; }
        else if (s.size() == 6 && s.compare(0, 3, "ltr") == 0 && s.compare(4, 2, "_y") == 0 && s[3] >= '0' &&
                 s[3] < '0' + args_.ltr_cfg.slots) { p = args_.ltr.y + (size_t)(s[3] - '0') * ny; n = ny; }
        else
            for (const DebugEntry& e : debug_)
                if (s == e.name && (e.codec < 0 || e.codec == cfg_.codec)) { p = e.dev; n = e.bytes; break; }
        if (!p) return -1;   // unknown, or a buffer this configuration does not have (stamps without SK_STAMPS)
        if (dst && cap >= n) HIPCHECK(hipMemcpyAsync(dst, p, (size_t)n, hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        return n;
    }

   private:
    // Blocking copies are ordered on the encoder's own stream: a copy on the legacy
    // stream fails while any stream of the process is capturing a graph (several
    // sessions share one process in parallel/multi.py session hosts). No extra stream:
    // every stream takes a slot in the process's round-robin over its hardware queues,
    // and an idle one per session halved the queues the sessions' work spread over
    // (8 x 1080p: 4150 -> 3650 fps).
    void copy_now(void* dst, const void* src, size_t n) {
        HIPCHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
    }

    // The CPU back end commits its controller and cache state at the end of a frame, k_plan at
    // the start of the next one. `commit`: that commit is still pending on the device
    // (plan_ctl[1] == 1), so the host applies it to the copies it hands out, with the last
    // frame's final `tasks`; `idr`: every slice was an IDR slice (the picture, full-frame mode).
    struct PendingCommit {
        bool started, commit, idr;
        std::vector<SliceTask> tasks;
    };
    PendingCommit pending_commit() {
        int ctl[4];
        copy_now(ctl, args_.plan_ctl, sizeof(ctl));
        PendingCommit pc{ctl[1] != 0, ctl[1] == 1, g_.num_slices > 0, std::vector<SliceTask>(g_.num_slices)};
        copy_now(pc.tasks.data(), args_.tasks, sizeof(SliceTask) * pc.tasks.size());
        for (const SliceTask& t : pc.tasks) pc.idr &= t.final_action == ACT_I && t.idr_on_intra;
        return pc;
    }
    std::vector<StripeState> committed_stripes(const PendingCommit& pc) {
        const int ns = g_.num_slices, max_refs = cfg_.num_refs > 1 ? 2 : 1;
        std::vector<StripeState> st(ns + 1);
        copy_now(st.data(), args_.plan_state, sizeof(StripeState) * (ns + 1));
        if (!pc.commit) return st;
        if (cfg_.fullframe) commit_picture(st[ns], pc.idr, max_refs);
        else
            for (int s = 0; s < ns; s++)
                commit_stripe(st[s], pc.tasks[s].final_action, max_refs, pc.tasks[s].idr_on_intra != 0);
        return st;
    }
    // Long-term cache state as the CPU back end holds it after a frame (empty: cache off).
    std::vector<ltr::LtrState> committed_ltr_state(const PendingCommit& pc) {
        const int ns = g_.num_slices, slots = args_.ltr_cfg.slots;
        std::vector<ltr::LtrState> ls(slots ? ns + 1 : 0);
        if (!slots) return ls;
        std::vector<ltr::LtrTask> lt(ns);
        copy_now(ls.data(), args_.ltr_state, sizeof(ltr::LtrState) * (ns + 1));
        copy_now(lt.data(), args_.ltr_task, sizeof(ltr::LtrTask) * ns);
        const std::vector<SliceTask>& tasks = pc.tasks;
        if (!pc.commit) return ls;
        const bool ff = cfg_.fullframe != 0;
        for (int s = 0; s < (ff ? 1 : ns); s++)   // one stream: the picture, or every stripe
            ltr_stream_commit(args_.ltr_cfg, ls[ff ? ns : s], tasks.data(), lt.data(), s, ff ? ns : s + 1, g_.mb_w,
                              g_.num_mbs(), ff, pc.idr);
        return ls;
    }

    // Where a section of the state blob (h264_state.h) lives on the device; the header has no storage.
    void* section_dev(const StateSection& s) {
        auto plane = [&](const gpu::Planes& p) { return s.plane == 0 ? p.y : s.plane == 1 ? p.u : p.v; };
        switch (s.kind) {
            case ST_STRIPES: return args_.plan_state;
            case ST_RC: return args_.rc;
            case ST_REF: return plane(args_.ref);
            case ST_REF1: return plane(args_.ref1);
            case ST_SRC: return plane(slot_[parity_ ^ 1].src);   // the parity flipped after the frame
            case ST_MVFIELD: return args_.mvfield;
            case ST_LTR_STATE: return args_.ltr_state;
            case ST_LTR_SLOT: return plane(args_.ltr) + (size_t)s.slot * s.bytes;
            default: return nullptr;
        }
    }

    // debug_buffer names that are one device buffer of a fixed size; codec -1: every codec. A
    // codec's own entry comes before the shared one of the same name ("coefs").
    struct DebugEntry {
        const char* name;
        int codec;
        const void* dev;
        int64_t bytes;
    };
    void build_debug_table() {
        const gpu::FrameArgs& a = args_;
        const hevc::gpu::HevcArgs& h = hargs_;
        const av1::gpu::Av1Args& v = aargs_;
        const int64_t nmb = g_.num_mbs(), ny = (int64_t)g_.stride_y * g_.plane_h_y, nc = (int64_t)g_.stride_c * g_.plane_h_c;
        const int64_t tiles = av1_geo_.tile_cols * av1_geo_.tile_rows, blks = (int64_t)av1_geo_.c8 * av1_geo_.r8;
        const int64_t segs = (int64_t)h.ch * h.seg_k;
        debug_ = {
            {"ref_y", -1, a.ref.y, ny}, {"ref_u", -1, a.ref.u, nc}, {"ref_v", -1, a.ref.v, nc},
            {"ref1_y", -1, a.ref1.y, ny},
            {"ltr_task", -1, a.ltr_task, (int64_t)(g_.num_slices * sizeof(ltr::LtrTask))},
            {"fs_mv", -1, a.fs_mv, nmb * 4},
            {"mbs", -1, a.mbs, (int64_t)(nmb * sizeof(MbInfo))},
            {"blk", 2, v.blk, (int64_t)(blks * sizeof(av1::BlkInfo))},
            {"levels", 2, v.lev, nmb * av1::gpu::kLevPerUnit * 2},
            {"tok_n", 2, v.tok_n, nmb * 4},
            {"tokc", 2, v.tokc, tiles * v.tile_tok_cap * 4},
            {"tile_ntok", 2, v.tile_ntok, tiles * 4},
            {"frame", 2, v.frame, 16},   // key, qidx, lf level, -
            {"av1_qidx", 2, v.frame ? v.frame + 1 : nullptr, 4},   // the CPU back end's name for frame[1]
            {"tile_size", 2, v.tile_size, tiles * 4},
            {"coefs", 1, h.coefs, nmb * hevc::kCoefPerCu * 2},
            {"cus", 1, h.cus, (int64_t)(nmb * sizeof(hevc::CuInfo))},
            {"sao", 1, h.sao, (int64_t)((int64_t)h.cw * h.ch * sizeof(hevc::SaoParams))},
            {"bin_n", 1, h.bin_n, nmb * 4},
            {"cu_t", 1, h.cu_t, nmb * 4},
            {"cu_r", 1, h.cu_r, nmb * 2},
            {"tail", 1, h.tail, nmb * 2},
            {"sub", 1, h.sub, (int64_t)h.ch * h.sub_stride},
            {"sub_size", 1, h.sub_size, segs * 4},
            {"row_bits", 1, h.row_bits, segs * 4},
            {"hevc_stamps", 1, h.dbg, (int64_t)h.ch * 32},
            {"coefs", -1, a.coefs, nmb * kCoefPerMb * 2},
            {"me", -1, a.me, (int64_t)(nmb * sizeof(MeResult))},
            {"mb_dirty", -1, a.mb_dirty, nmb},
            {"aq", -1, a.aq, nmb},
            {"stamps", -1, a.dbg, (64 * 16 + 256) * 8},
        };
    }

    gpu::Planes make_planes() {
        size_t ny = (size_t)g_.stride_y * g_.plane_h_y, nc = (size_t)g_.stride_c * g_.plane_h_c;
        gpu::Planes p;
        p.y = mem_.dmalloc<uint8_t>(ny);
        p.u = mem_.dmalloc<uint8_t>(nc);
        p.v = mem_.dmalloc<uint8_t>(nc);
        return p;
    }

    void alloc() {
        const int nmb = g_.num_mbs(), ns = g_.num_slices;
        for (auto& f : slot_) f.src = make_planes();
        gpu::FrameArgs& a = args_;
        memset(&a, 0, sizeof(a));
        a.W = g_.W; a.H = g_.H; a.mb_w = g_.mb_w; a.mb_h = g_.mb_h;
        a.stride_y = g_.stride_y; a.stride_c = g_.stride_c;
        a.num_slices = ns; a.rows_per_slice = g_.rows_per_slice; a.fullframe = cfg_.fullframe;
        a.full_range = cfg_.full_range; a.me_range = cfg_.me_range; a.me_iters = cfg_.me_iters;
        a.deblock = cfg_.codec == 0 ? cfg_.deblock : 0;   // HEVC / AV1 filter in their own back ends
        a.me_full = cfg_.me_full;
        a.aq_strength = cfg_.codec == 1 ? 0 : cfg_.aq_strength;
        a.subpel = cfg_.codec == 2 ? 0 : cfg_.subpel;   // AV1 keeps integer vectors (av1_encoder.h front_config)
        a.intra4x4 = cfg_.codec == 1 ? 0 : cfg_.intra4x4;
        a.aq = mem_.dmalloc<int8_t>(nmb);
        for (int k = 0; k < kOverlaySlots; k++) {
            ov_img_dev_[k] = mem_.dmalloc<uint8_t>((size_t)kOverlayMaxDim * kOverlayMaxDim * 4);
            a.ov_img[k] = ov_img_dev_[k];
        }
        for (auto& h : ov_params_host_) h = mem_.hmalloc<OverlayParams>(kOverlaySlots);
        ov_params_dev_ = mem_.dmalloc<OverlayParams>(kOverlaySlots);
        a.ov = ov_params_dev_;
        memset(ov_pending_, 0, sizeof(ov_pending_));
        a.num_refs = cfg_.num_refs > 1 ? 2 : 1;
        a.scaled = (cfg_.src_width > 0 && cfg_.src_width != cfg_.width) ||
                   (cfg_.src_height > 0 && cfg_.src_height != cfg_.height);
        if (a.scaled)
            a.scale = scale_params(cfg_.src_width > 0 ? cfg_.src_width : cfg_.width,
                                   cfg_.src_height > 0 ? cfg_.src_height : cfg_.height, cfg_.width, cfg_.height);
        a.ref = make_planes();
        a.ref1 = make_planes();
        a.rec = make_planes();
        a.ltr_cfg = ltr_config_of(cfg_);
        if (a.ltr_cfg.slots) {   // long-term cache (codec/ltr.h): slot plane sets, stream states, per-frame decisions
            const size_t ny = (size_t)g_.stride_y * g_.plane_h_y, nc = (size_t)g_.stride_c * g_.plane_h_c;
            a.ltr_ny = ny;
            a.ltr_nc = nc;
            a.ltr.y = mem_.dmalloc<uint8_t>(ny * a.ltr_cfg.slots);
            a.ltr.u = mem_.dmalloc<uint8_t>(nc * a.ltr_cfg.slots);
            a.ltr.v = mem_.dmalloc<uint8_t>(nc * a.ltr_cfg.slots);
            ltr::LtrState z;
            ltr::ltr_state_reset(z);
            std::vector<ltr::LtrState> init(ns + 1, z);
            a.ltr_state = mem_.dmalloc<ltr::LtrState>(ns + 1);
            copy_now(a.ltr_state, init.data(), sizeof(ltr::LtrState) * (ns + 1));
            ltr::LtrTask zt;
            ltr::ltr_task_reset(zt);
            std::vector<ltr::LtrTask> tinit(ns, zt);
            a.ltr_task = mem_.dmalloc<ltr::LtrTask>(ns);
            copy_now(a.ltr_task, tinit.data(), sizeof(ltr::LtrTask) * ns);
            a.ltr_part = mem_.dmalloc<uint32_t>((size_t)ns * ltr::kLtrSadCols * g_.rows_per_slice);
            a.ltr_sad = mem_.dmalloc<uint32_t>((size_t)ns * ltr::kLtrSadCols);
            a.ltr_cnt = mem_.dmalloc<int>(2 * (size_t)ns);
        }
        a.mb_dirty = mem_.dmalloc<uint8_t>(nmb);
        a.stripe_dirty = mem_.dmalloc<int>(ns);
        a.plan_ctl = mem_.dmalloc<int>(4);
        a.plan_cfg = plan_config(cfg_);
        {
            std::vector<StripeState> init(ns + 1);  // need_idr on every stripe and the picture
            a.plan_state = mem_.dmalloc<StripeState>(ns + 1);
            HIPCHECK(hipMemcpyAsync(a.plan_state, init.data(), sizeof(StripeState) * (ns + 1),
                                    hipMemcpyHostToDevice, stream_));
            HIPCHECK(hipStreamSynchronize(stream_));
        }
        h_key_seq_ = mem_.hmalloc<int>(16, hipHostMallocCoherent);   // written by request_keyframe/set_qp
        // per-parity snapshot taken at launch, read by k_plan
        for (auto& f : slot_) f.key_snap = mem_.mapped<int>(8, hipHostMallocCoherent);
        a.key_seq_host = slot_[0].key_snap.dev;
        a.key_dev = mem_.dmalloc<int>(8);
        a.tasks = mem_.dmalloc<SliceTask>(ns);
        a.me = mem_.dmalloc<MeResult>(nmb);
        a.mvfield = mem_.dmalloc<int16_t>(2 * nmb);
        a.fs_mv = mem_.dmalloc<int16_t>(2 * nmb);
        {   // K10 rate control state (ratecontrol.h), initialised like the CPU controller's
            RcState rc;
            rc_init(rc, cfg_.rc_mode, cfg_.qp, cfg_.bitrate_kbps, cfg_.fps, cfg_.width * cfg_.height, cfg_.vbv_ms, cfg_.codec);
            a.rc = mem_.dmalloc<RcState>(1);
            copy_now(a.rc, &rc, sizeof(rc));
            a.rc_slice = mem_.dmalloc<long long>(2 * (size_t)ns);
            a.rc_redo = mem_.dmalloc<int>(1);
            a.gate = nullptr;
            a.rc_fps = cfg_.fps;
            h_key_seq_[3] = cfg_.rc_mode;
            dev_rc_mode_ = cfg_.rc_mode;
            h_key_seq_[4] = cfg_.bitrate_kbps;
        }
        a.db = mem_.dmalloc<DbInfo>(nmb);
        a.dbe = mem_.dmalloc<uint4>((size_t)3 * nmb);
        a.mbs = mem_.dmalloc<MbInfo>(nmb);
        a.coefs = mem_.dmalloc<int16_t>((size_t)nmb * kCoefPerMb);
        a.mb_bits = mem_.dmalloc<uint32_t>((size_t)nmb * (gpu::kMbSlotBytes / 4));
        a.mb_nbits = mem_.dmalloc<int>(nmb);
        int max_slice_mbs = g_.rows_per_slice * g_.mb_w;
        // K5: split I slices put one NAL per sub-slice (h264_encoder.h intra_split)
        const bool can_split = cfg_.codec == 0 && g_.mb_w > kIntraSubMbs;
        a.nal_per_slice = can_split ? max_nals_per_slice(g_.rows_per_slice, g_.mb_w) : 1;
        if (cfg_.codec == 0 && max_slice_mbs > gpu::kPackMaxSliceMbs)
            throw std::runtime_error("H.264: more than " + std::to_string(gpu::kPackMaxSliceMbs) +
                                     " macroblocks per slice is not supported");   // k_slice_pack's bbase[]
        a.slice_info = mem_.dmalloc<int>(4 * (size_t)ns * a.nal_per_slice);
        // A slice's RBSP at its worst: every MB fills its CAVLC slot, plus the slice header
        // (per sub-slice NAL where I slices are split). The RBSP itself only exists in LDS
        // (k_slice_pack); the bound sizes the host slot.
        const size_t sub_rbsp = (size_t)kIntraSubMbs * gpu::kMbSlotBytes + 1024;
        const size_t max_rbsp = std::max((size_t)max_slice_mbs * gpu::kMbSlotBytes + 1024,
                                         can_split ? a.nal_per_slice * sub_rbsp : (size_t)0);
        // worst case: header + SPS/PPS + 3/2 emulation-prevention growth, 64-byte multiple
        size_t slot = (max_rbsp * 3 / 2 + 1024 + 63) & ~(size_t)63;
        a.out_slot_bytes = (int)slot;
        for (auto& f : slot_) {   // host outputs per parity (two frames in flight)
            f.out = mem_.mapped<uint8_t>(slot * ns);
            f.out_size = mem_.mapped<int>(ns);
        }
        // parameter sets
        std::vector<std::vector<uint8_t>> ps;
        if (cfg_.fullframe) {
            ps.resize(1);
            build_parameter_sets(g_.W, g_.H, cfg_.full_range, cfg_.fps, ps[0], cfg_.num_refs, ltr_slots_of(cfg_));
        } else {
            ps.resize(ns);
            for (int s = 0; s < ns; s++)
                build_parameter_sets(g_.W, g_.slice_pix_h(s), cfg_.full_range, cfg_.fps, ps[s], cfg_.num_refs,
                                     ltr_slots_of(cfg_));
        }
        param_sets_ = ps;
        a.param_set_stride = 256;
        std::vector<uint8_t> flat((size_t)ns * 256, 0);
        std::vector<int> lens(ns, 0);
        for (int s = 0; s < ns; s++) {
            const std::vector<uint8_t>& v = ps[cfg_.fullframe ? 0 : s];
            if (v.size() > 256) throw std::runtime_error("parameter sets too large");
            memcpy(&flat[(size_t)s * 256], v.data(), v.size());
            lens[s] = (int)v.size();
        }
        uint8_t* dps = mem_.dmalloc<uint8_t>(flat.size());
        HIPCHECK(hipMemcpyAsync(dps, flat.data(), flat.size(), hipMemcpyHostToDevice, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        int* dlen = mem_.dmalloc<int>(ns);
        HIPCHECK(hipMemcpyAsync(dlen, lens.data(), sizeof(int) * ns, hipMemcpyHostToDevice, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        a.param_sets = dps;
        a.param_set_len = dlen;
        CavlcTables* ct = mem_.dmalloc<CavlcTables>(1);
        HIPCHECK(hipMemcpyAsync(ct, &host_cavlc_tables(), sizeof(CavlcTables), hipMemcpyHostToDevice, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        a.cavlc_tabs = ct;
        if (getenv("SK_STAMPS")) a.dbg = mem_.dmalloc<unsigned long long>(64 * 16 + 256);
        a.frame_params_dev = mem_.dmalloc<int>(4);
        for (auto& f : slot_) {
            f.tasks = mem_.mapped<SliceTask>(ns, hipHostMallocCoherent);  // final decisions from k_decide
            f.frame_params = mem_.mapped<int>(4, hipHostMallocCoherent);
        }
    }

    // The one place that maps the slot of parity_ onto FrameArgs.
    void set_parity_args() {
        const FrameSlot& f = slot_[parity_];
        args_.yuv = f.yuv;
        args_.yuv_fmt = yuv_mode_;
        args_.bgrx = f.bgrx;
        args_.src = f.src;
        args_.prev = slot_[parity_ ^ 1].src;
        args_.host_out = f.out.dev;
        args_.host_size = f.out_size.dev;
        args_.tasks_host = f.tasks.dev;
        args_.frame_params_host = f.frame_params.dev;
        args_.key_seq_host = f.key_snap.dev;
    }

    void invalidate_graphs() {
        ov_resend_ = true;
        for (auto& f : slot_)
            for (hipGraphExec_t* gx : {&f.graph, &f.post, &f.post_short})
                if (*gx) { hipGraphExecDestroy(*gx); *gx = nullptr; }
    }

    // A change of what the captured graphs bake in (input kind, input stride or buffers, the
    // CBR guard): drains the stream, applies `change` (frees, reallocations), then drops the
    // graphs; the next launch captures them again.
    template <class F>
    void recapture(F&& change) {
        HIPCHECK(hipStreamSynchronize(stream_));
        change();
        invalidate_graphs();
    }

    // Neither input buffer holds a complete earlier frame: the next two uploads copy everything.
    void drop_uploads() { slot_[0].up_valid = slot_[1].up_valid = false; }

    // part 0: convert/damage -> ... -> packets; part 1: commit (+ deblocking); part 2: commit
    // alone, for frames in which no slice can be filtered (can_filter).
    // The H.264 chain's K10 accounting runs in k_commit (both commit graphs), behind
    // k_slice_pack; every host reader of the controller state (rc_stats, export_state)
    // synchronises the stream, so behind part 1. Stripe flags are cleared by k_plan. The overlay
    // placement is not part of the graph: launch() copies it ahead of the graph when it changed.
    void enqueue(int part) {
        const FrameSlot& f = slot_[parity_];
        if (part == 0) {
            gpu::launch_convert_damage(args_, stream_);
            if (cfg_.codec == 2) {
                gpu::launch_frontend(args_, stream_);
                av1::gpu::Av1Args aa = aargs_;
                aa.f = args_;
                aa.frame_host = f.av1_frame.dev;
                aa.out_host = f.av1_out.dev;
                aa.out_size_host = f.av1_size.dev;
                av1::gpu::launch_backend(aa, stream_, graph_guard_ ? args_.rc_redo : nullptr);
                gpu::launch_rc_account(args_, aa.tile_size, av1_geo_.tile_cols * av1_geo_.tile_rows, 1, 0, stream_);
            } else if (cfg_.codec == 1) {
                gpu::launch_frontend(args_, stream_);
                hevc::gpu::HevcArgs ha = hargs_;
                ha.f = args_;
                ha.out_host = f.hevc_out.dev;
                ha.out_size = f.hevc_size.dev;
                ha.out_dev = f.hevc_fallback;
                hevc::gpu::launch_backend(ha, stream_, graph_guard_ ? args_.rc_redo : nullptr);
                gpu::launch_rc_account(args_, ha.sub_size, ha.ch * ha.seg_k, 1, 0, stream_);
            } else {
                gpu::launch_encode(args_, stream_, graph_guard_);
            }
        } else {
            gpu::launch_commit(args_, stream_, part == 1, cfg_.codec == 0);
        }
    }

    // Whether a slice of the frame launched with key snapshot `snap` (FrameSlot::key_snap) can be
    // deblocked, i.e. whether part 1 needs its deblocking kernels. Off: never. On: always.
    // Automatic (slices at QP >= kAutoDeblockQp): not when max_slice_qp, for the frame's
    // rate mode and QPs, stays below the threshold - every CQP / CRF session at the default
    // QPs. CBR reaches every QP and always takes the long graph. The rate mode is the device
    // controller's at that frame: k_plan takes the snapshot's mode when its set_rate()
    // counter moved (as here), else keeps its own (initial, or imported with a state).
    bool can_filter(const int* snap) {
        if (!args_.deblock) return false;
        if (snap[5] != dev_rc_seq_) {
            dev_rc_seq_ = snap[5];
            dev_rc_mode_ = snap[3];
        }
        if (args_.deblock != 2) return true;
        const int qp = snap[1] > 0 ? snap[1] : cfg_.qp, pqp = snap[2] > 0 ? snap[2] : cfg_.paint_qp;
        return max_slice_qp(dev_rc_mode_, qp, pqp) >= kAutoDeblockQp;
    }

    void run_graph(hipGraphExec_t& gx, int part) {
        if (!use_graphs_) {
            enqueue(part);
            return;
        }
        if (!gx) {
            hipGraph_t graph;
            HIPCHECK(hipStreamBeginCapture(stream_, hipStreamCaptureModeRelaxed));
            enqueue(part);
            HIPCHECK(hipStreamEndCapture(stream_, &graph));
            HIPCHECK(hipGraphInstantiate(&gx, graph, nullptr, nullptr, 0));
            hipGraphDestroy(graph);
        }
        HIPCHECK(hipGraphLaunch(gx, stream_));
    }

    // HEVC back-end buffers (hevc_gpu.h): CU decisions, levels, bin slots, WPP states,
    // one substream slot per CTB row, host-mapped slice slots + device fallback.
    void alloc_hevc() {
        const int n = g_.num_mbs(), ns = g_.num_slices;
        hevc::Geo geo;
        geo.init(g_);
        hevc::gpu::HevcArgs& h = hargs_;
        memset(&h, 0, sizeof(h));
        h.cw = geo.ctb_w;
        h.ch = geo.ctb_h;
        h.rps = geo.rows_per_slice;
        if (g_.rows_per_slice & 1) throw std::runtime_error("HEVC: stripes must be whole CTB rows");
        const int nc = geo.ctbs();
        h.cus = mem_.dmalloc<hevc::CuInfo>(n);
        h.coefs = mem_.dmalloc<int16_t>((size_t)n * hevc::kCoefPerCu);
        h.bins = mem_.dmalloc<uint16_t>((size_t)n * hevc::kCuBinCap, false);
        h.bin_n = mem_.dmalloc<int>(n);
        // intra slices: seg_k slices per CTB row (hevc_core.h SliceMap); per-substream
        // arrays hold ch * seg_k slots
        h.seg_k = hevc::intra_seg_k(h.cw, h.ch);
        if (h.rps * h.seg_k > 256) throw std::runtime_error("HEVC: more than 256 row segments per slice");
        const size_t slots = (size_t)h.ch * h.seg_k;
        h.sync = mem_.dmalloc<uint8_t>(slots * hevc::CTX_COUNT);
        h.sub_stride = h.cw * 4 * hevc::kSubstreamCtbBytes + 64 * h.seg_k + 64;
        h.sub = mem_.dmalloc<uint8_t>((size_t)h.ch * h.sub_stride, false);
        h.sub_size = mem_.dmalloc<int>(slots);
        h.sub_esc = mem_.dmalloc<int>(slots);
        h.row_off = mem_.dmalloc<int>(slots);
        h.addr_bits = geo.addr_bits;
        if (2 * g_.mb_w > 1024) throw std::runtime_error("HEVC: more than 1024 units per CTB row (8K) is not supported");
        h.srt = mem_.dmalloc<uint16_t>((size_t)n * hevc::kCuBinCap, false);
        h.coff = mem_.dmalloc<uint16_t>((size_t)h.ch * hevc::kPcCtxOff * 2 * g_.mb_w, false);
        h.rmap = mem_.dmalloc<uint32_t>((size_t)n * 256, false);
        h.cu_t = mem_.dmalloc<uint32_t>(n);
        h.cu_r = mem_.dmalloc<uint16_t>(n);
        h.tail = mem_.dmalloc<uint8_t>((size_t)n * 2);
        h.row_bits = mem_.dmalloc<uint32_t>(slots);
        h.sao_stats = mem_.dmalloc<hevc::SaoStats>((size_t)3 * nc, false);
        h.sao_own = mem_.dmalloc<hevc::SaoParams>(nc);
        h.sao_cost = mem_.dmalloc<long long>(nc);
        h.sao_md = mem_.dmalloc<long long>((size_t)nc * hevc::kSaoMd);
        h.sao = mem_.dmalloc<hevc::SaoParams>(nc);
        h.sao_tmp.y = mem_.dmalloc<uint8_t>((size_t)g_.stride_y * g_.mb_h * 16, false);
        h.sao_tmp.u = mem_.dmalloc<uint8_t>((size_t)g_.stride_c * g_.mb_h * 8, false);
        h.sao_tmp.v = mem_.dmalloc<uint8_t>((size_t)g_.stride_c * g_.mb_h * 8, false);
        // host slot: 1.5 KB per CTB (far above practical rates); larger slices go to the
        // device fallback slot (worst case: 3/2 emulation growth of the substream bound)
        h.out_slot = (g_.rows_per_slice * g_.mb_w * 1536 + 4096 + 63) & ~63;
        h.out_dev_slot = (int)(((size_t)h.rps * h.sub_stride * 3 / 2 + 4096 + 63) & ~(size_t)63);
        for (auto& f : slot_) {
            f.hevc_out = mem_.mapped<uint8_t>((size_t)h.out_slot * ns);
            f.hevc_size = mem_.mapped<int>(ns, hipHostMallocCoherent);
            f.hevc_fallback = mem_.dmalloc<uint8_t>((size_t)h.out_dev_slot * ns, false);
        }
        HIPCHECK(hipStreamSynchronize(stream_));
        if (getenv("SK_STAMPS")) h.dbg = mem_.dmalloc<unsigned long long>((size_t)4 * h.ch);
        h.reg_steps = getenv("SK_HEVC_REG_STEPS") ? atoi(getenv("SK_HEVC_REG_STEPS")) : 1;
        h.pc_seg = getenv("SK_HEVC_PC_SEG") ? sk_max(atoi(getenv("SK_HEVC_PC_SEG")), 1) : 32;
        hevc_params_.clear();
        hevc::build_parameter_sets(g_.W, g_.H, cfg_.full_range, cfg_.fps, hevc_params_, ltr_slots_of(cfg_));
    }

    // AV1 back-end buffers (av1_gpu.h): cells, levels, level contexts, token slots per
    // 16x16 unit, block-parallel coder state per tile, host-mapped frame info and tile bytes.
    void alloc_av1() {
        const int n = g_.num_mbs();
        av1::gpu::Av1Args& a = aargs_;
        memset(&a, 0, sizeof(a));
        av1::session_geo(av1_geo_, g_.W, g_.H, cfg_.tile_cols_log2, cfg_.tile_rows_log2);
        a.geo = av1_geo_;
        a.blk = mem_.dmalloc<av1::BlkInfo>((size_t)av1_geo_.c8 * av1_geo_.r8);
        a.pal = mem_.dmalloc<uint8_t>((size_t)av1_geo_.c8 * av1_geo_.r8 * 8);
        a.palette = av1::palette_enabled() ? 1 : 0;
        a.pal_rate = mem_.dmalloc<int>((size_t)av1_geo_.c8 * av1_geo_.r8);
        a.intra_inter = cfg_.av1_intra_inter > 0;
        if (a.intra_inter) {   // av1_gpu.h: the inter coding's J, the intra candidates and their count per tile
            a.jinter = mem_.dmalloc<long long>((size_t)av1_geo_.c8 * av1_geo_.r8);
            a.cand = mem_.dmalloc<int>((size_t)av1_geo_.c8 * av1_geo_.r8);
            a.tile_cand = mem_.dmalloc<int>((size_t)av1_geo_.tile_cols * av1_geo_.tile_rows);
        }
        a.lev = mem_.dmalloc<int16_t>((size_t)n * av1::gpu::kLevPerUnit);
        a.lctx_w[0] = av1_geo_.mi_cols;
        a.lctx_w[1] = a.lctx_w[2] = av1_geo_.mi_cols >> 1;
        a.lctx[0] = mem_.dmalloc<uint8_t>((size_t)av1_geo_.mi_cols * av1_geo_.mi_rows);
        a.lctx[1] = mem_.dmalloc<uint8_t>((size_t)(av1_geo_.mi_cols >> 1) * (av1_geo_.mi_rows >> 1));
        a.lctx[2] = mem_.dmalloc<uint8_t>((size_t)(av1_geo_.mi_cols >> 1) * (av1_geo_.mi_rows >> 1));
        a.tok = mem_.dmalloc<uint32_t>((size_t)n * av1::gpu::kTokCap, false);
        a.tok_n = mem_.dmalloc<int>(n);
        a.frame = mem_.dmalloc<int>(4);
        a.cdef_in.y = mem_.dmalloc<uint8_t>((size_t)g_.stride_y * g_.mb_h * 16, false);
        a.cdef_in.u = mem_.dmalloc<uint8_t>((size_t)g_.stride_c * g_.mb_h * 8, false);
        a.cdef_in.v = mem_.dmalloc<uint8_t>((size_t)g_.stride_c * g_.mb_h * 8, false);
        const int tiles = av1_geo_.tile_cols * av1_geo_.tile_rows;
        // tile bytes: 4 KB per unit of the largest tile (incompressible content codes
        // below ~1.5 bytes per sample)
        const int tile_units = (av1_geo_.tile_w_sb * 4) * (av1_geo_.tile_h_sb * 4);
        a.tile_tok_cap = tile_units * av1::gpu::kTokCap;
        a.tokc = mem_.dmalloc<uint32_t>((size_t)tiles * a.tile_tok_cap, false);
        // + per-wave junk slots of k_av1_cdf (words of tokens a wave does not own)
        a.pw = mem_.dmalloc<uint32_t>((size_t)tiles * a.tile_tok_cap + (size_t)tiles * 16 * 64, false);
        a.tok_off = mem_.dmalloc<int>(n);
        a.tile_ntok = mem_.dmalloc<int>(tiles);
        a.tile_cap = tile_units * 4096;
        if (tiles > 64) throw std::runtime_error("AV1: at most 64 tiles");
        av1::gpu::ec_buffers(tiles, a.tile_cap, &a.ec_max_blocks, &a.ec_vcap);
        a.ecmap = mem_.dmalloc<uint2>((size_t)a.ec_max_blocks * 128, false);
        a.ecblk = mem_.dmalloc<int4>((size_t)a.ec_max_blocks, false);
        a.ecv = mem_.dmalloc<unsigned long long>((size_t)tiles * a.ec_vcap, false);
        a.ecf = mem_.dmalloc<uint32_t>((size_t)tiles * a.ec_vcap, false);
        a.tile_bits = mem_.dmalloc<int>(tiles);
        a.tile_size = mem_.dmalloc<int>(tiles);
        a.out_cap = g_.W * g_.H * 3 + 4096;
        std::vector<uint8_t> q(52);
        for (int i = 0; i < 52; i++) q[i] = (uint8_t)av1::qidx_for_qp(i);
        uint8_t* dq = mem_.dmalloc<uint8_t>(52);
        copy_now(dq, q.data(), 52);
        a.qidx_of_qp = dq;
        for (auto& f : slot_) {
            f.av1_out = mem_.mapped<uint8_t>((size_t)a.out_cap);
            f.av1_size = mem_.mapped<int>(tiles, hipHostMallocCoherent);
            f.av1_frame = mem_.mapped<int>(8, hipHostMallocCoherent);
        }
        HIPCHECK(hipStreamSynchronize(stream_));
        av1_level_ = av1::choose_level_idx(g_.W, g_.H, cfg_.fps);
    }

    void build_packets_av1(const FrameSlot& f) {
        const int tiles = av1_geo_.tile_cols * av1_geo_.tile_rows;
        av1::FrameParams fp;
        fp.key = f.av1_frame.host[0];
        fp.qidx = f.av1_frame.host[1];
        fp.lf_level = f.av1_frame.host[2];
        if (args_.ltr_cfg.mode == ltr::LTR_BUFMAP) {   // long-term cache: the reference buffers k_av1_setup chose (ltr.h buffer map)
            fp.refresh = f.av1_frame.host[3];
            fp.last_buf = f.av1_frame.host[4];
            fp.last2_buf = f.av1_frame.host[5];
        }
        fp.screen = (fp.key || aargs_.intra_inter) && aargs_.palette;
        std::vector<std::vector<uint8_t>> tl(tiles);
        size_t off = 0;
        for (int t = 0; t < tiles; t++) {
            const int n = f.av1_size.host[t];
            if (n < 0) throw std::runtime_error("AV1 tile exceeded its output capacity");
            tl[t].assign(f.av1_out.host + off, f.av1_out.host + off + n);
            off += (size_t)n;
        }
        size_t maxsz = 1;
        for (int t = 0; t + 1 < tiles; t++) maxsz = std::max(maxsz, tl[t].size());
        fp.tile_size_bytes = maxsz <= 0x100 ? 1 : (maxsz <= 0x10000 ? 2 : (maxsz <= 0x1000000 ? 3 : 4));
        EncodedPacket pk;
        pk.y = 0; pk.w = g_.W; pk.h = g_.H; pk.key = fp.key;
        pk.data.resize(10);
        write_stripe_header(pk.data.data(), fp.key, f.frame, 0, g_.W, g_.H);
        av1::append_obu(pk.data, 2, nullptr, 0);
        if (fp.key) {
            av1::BitWriter sh;
            av1::write_sequence_header(sh, g_.W, g_.H, av1_level_, cfg_.full_range);
            av1::append_obu(pk.data, 1, sh.buf.data(), sh.buf.size());
        }
        av1::BitWriter fh;
        av1::write_frame_header(fh, av1_geo_, fp);
        std::vector<uint8_t> payload = fh.buf;
        if (tiles > 1) payload.push_back(0);
        for (int t = 0; t < tiles; t++) {
            if (t + 1 < tiles) {
                const uint32_t sz = (uint32_t)tl[t].size() - 1;
                for (int k = 0; k < fp.tile_size_bytes; k++) payload.push_back((uint8_t)(sz >> (8 * k)));
            }
            payload.insert(payload.end(), tl[t].begin(), tl[t].end());
        }
        av1::append_obu(pk.data, 6, payload.data(), payload.size());
        packets_.push_back(std::move(pk));
    }

    void build_packets_hevc(const FrameSlot& f) {
        const SliceTask* h_tasks = f.tasks.host;
        const int ns = g_.num_slices;
        const bool idr = ctl_.picture_is_idr(h_tasks);
        EncodedPacket pk;
        pk.y = 0; pk.w = g_.W; pk.h = g_.H; pk.key = idr;
        pk.data.resize(10);
        write_stripe_header(pk.data.data(), idr, f.frame, 0, g_.W, g_.H);
        if (idr) pk.data.insert(pk.data.end(), hevc_params_.begin(), hevc_params_.end());
        for (int s = 0; s < ns; s++) {
            const int n = f.hevc_size.host[s];
            const size_t o = pk.data.size();
            pk.data.resize(o + (size_t)n);
            if (n <= hargs_.out_slot) {
                memcpy(pk.data.data() + o, f.hevc_out.host + (size_t)s * hargs_.out_slot, (size_t)n);
            } else {   // rare: the slice did not fit its host slot
                copy_now(pk.data.data() + o, f.hevc_fallback + (size_t)s * hargs_.out_dev_slot, (size_t)n);
            }
        }
        packets_.push_back(std::move(pk));
    }

    void build_packets(const FrameSlot& f) {
        if (cfg_.codec == 2) return build_packets_av1(f);
        if (cfg_.codec == 1) return build_packets_hevc(f);
        const uint8_t* host_out = f.out.host;
        const int* h_out_size = f.out_size.host;
        const SliceTask* h_tasks = f.tasks.host;
        const int ns = g_.num_slices;
        std::vector<long> offs(ns);
        for (int s = 0; s < ns; s++) offs[s] = (long)s * args_.out_slot_bytes;
        if (cfg_.fullframe) {
            bool idr = ctl_.picture_is_idr(h_tasks);
            EncodedPacket pk;
            pk.y = 0; pk.w = g_.W; pk.h = g_.H; pk.key = idr;
            pk.data.resize(10);
            write_stripe_header(pk.data.data(), idr, f.frame, 0, g_.W, g_.H);
            if (idr) pk.data.insert(pk.data.end(), param_sets_[0].begin(), param_sets_[0].end());
            for (int s = 0; s < ns; s++) {
                const uint8_t* p = host_out + offs[s];
                pk.data.insert(pk.data.end(), p, p + h_out_size[s]);
            }
            packets_.push_back(std::move(pk));
            return;
        }
        for (int s = 0; s < ns; s++) {
            if (h_tasks[s].final_action == ACT_NONE || h_out_size[s] <= 0) continue;
            EncodedPacket pk;
            pk.y = g_.slice_pix_y(s);
            pk.w = g_.W;
            pk.h = g_.slice_pix_h(s);
            pk.key = h_tasks[s].final_action == ACT_I && h_tasks[s].idr_on_intra;   // non-IDR I: long-term cache on
            const uint8_t* p = host_out + offs[s];
            pk.data.assign(p, p + h_out_size[s]);
            packets_.push_back(std::move(pk));
        }
    }

    int inflight() const { return launched_ - finished_; }

    hipStream_t upload_stream() {
        if (!up_stream_) HIPCHECK(hipStreamCreateWithFlags(&up_stream_, hipStreamNonBlocking));
        return up_stream_;
    }

    // One H2D stream per device for encoders created with shared_copy: lives as long
    // as the process (encoders come and go, the stream is reused).
    static hipStream_t device_copy_stream(int device) {
        static std::mutex mu;
        static std::map<int, hipStream_t> streams;
        std::lock_guard<std::mutex> lk(mu);
        auto it = streams.find(device);
        if (it != streams.end()) return it->second;
        hipStream_t s = nullptr;
        HIPCHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        streams[device] = s;
        return s;
    }

    // ---- configuration ----
    EncoderConfig cfg_;
    Geometry g_;
    Controller ctl_;
    int device_;
    bool use_graphs_ = getenv("SK_NO_GRAPHS") == nullptr;
    // 0: on the session stream (behind the frame in flight), 1: own upload stream,
    // 2: the device's shared copy stream
    int upload_mode_ = getenv("SK_UPLOAD_MODE") ? atoi(getenv("SK_UPLOAD_MODE")) : 2;
    std::vector<std::vector<uint8_t>> param_sets_;
    std::vector<uint8_t> hevc_params_;
    av1::Av1Geo av1_geo_ = {};
    int av1_level_ = 8;
    std::vector<DebugEntry> debug_;

    // ---- device state ----
    HipAllocs mem_;
    hipStream_t stream_ = nullptr;
    hipStream_t copy_stream_ = nullptr;   // shared per device (not owned)
    hipStream_t up_stream_ = nullptr;     // this session's upload stream (owned, lazily created)
    gpu::FrameArgs args_;
    hevc::gpu::HevcArgs hargs_ = {};
    av1::gpu::Av1Args aargs_ = {};
    int* h_key_seq_ = nullptr;   // host-coherent: key-frame counter, QP overrides, rate mode / kbps / counter
    int dev_rc_mode_ = 0, dev_rc_seq_ = 0;   // rate mode of the device controller and the set_rate() counter it has seen
    bool graph_guard_ = false;   // the captured H.264 graphs contain the K10 CBR guard
    int yuv_mode_ = 0;           // YuvFormat of the captured graphs (0: BGRx)
    float stage_ms_[2] = {0, 0};

    // ---- per-parity slots ----
    FrameSlot slot_[2];
    int parity_ = 0;
    int launched_ = 0, finished_ = 0;   // frames launched / finished; frame k uses slot k & 1

    // ---- upload bookkeeping ----
    bool staged_ = false, staged_on_main_ = true;
    uint16_t staged_frame_ = 0;
    size_t bgrx_cap_ = 0;
    hipEvent_t ev_ext_ = nullptr;   // wait_stream(): foreign stream's work before the next upload
    bool ext_wait_ = false;
    // damage-driven upload (set_upload_rows / upload_copy)
    bool up_next_known_ = false, up_prev_known_ = false;
    std::vector<int> up_next_, up_prev_;     // row ranges of this frame / the previous one
    std::atomic<long long> up_rows_copied_{0}, up_rows_total_{0};   // read by the stats thread

    // ---- overlay staging ----
    uint8_t* ov_img_dev_[kOverlaySlots] = {};
    OverlayParams* ov_params_dev_ = nullptr;
    // Pinned staging of the placement copies, rotating: launch(n + 2) comes after
    // finish(n), so the copy queued ahead of graph n has run when its slot is written again.
    static constexpr int kOvStage = 2;
    OverlayParams* ov_params_host_[kOvStage] = {};
    OverlayParams ov_sent_[kOverlaySlots] = {};   // what the device holds
    int ov_slot_ = 0;
    bool ov_resend_ = true;                       // first launch, and after a re-capture
    OverlayParams ov_pending_[kOverlaySlots];
    uint8_t* ov_stage_ = nullptr;
};

}  // namespace

// A fresh process pays a one-time cost when several threads queue SDMA copies behind
// kernels on their streams: during the first ~50 such copies hipMemcpyAsync blocks
// the calling thread, and every other copying thread with it, for 6-9 ms while the
// GPU idles (rocprofv3 --hip-runtime-trace of the 8-session bench: all capture
// threads inside hipMemcpyAsync at once, four times within the first ~40 frames;
// tools/microbench/h2d_stall.cpp reproduces it with 8 threads x (copy + 12 small
// kernels): 46 stalled calls; 0 with HSA_ENABLE_SDMA=0, with copies on kernel-free
// streams, or after this warm-up; profiles/r2_driver_window.md). Whatever the
// runtime grows in that phase is per process, not per stream: the same pattern run
// here from 8 threads on streams of their own, destroyed afterwards, leaves the
// sessions' own streams stall-free. Serving would otherwise pay it inside the first
// second of the first sessions. SK_COPY_WARMUP=0 skips it.
void warm_copy_engines(int device) {
    static std::mutex mu;
    static std::map<int, bool> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done[device]) return;
    done[device] = true;
    const char* env = getenv("SK_COPY_WARMUP");
    if (env && atoi(env) == 0) return;
    const int kThreads = 8, kRounds = 60, kKernels = 12;
    const size_t bytes = (size_t)8 << 20;
    uint8_t* host = nullptr;
    if (hipHostMalloc((void**)&host, bytes, hipHostMallocDefault) != hipSuccess) return;
    for (size_t i = 0; i < bytes; i += 4096) host[i] = 0;
    std::vector<std::thread> th;
    for (int t = 0; t < kThreads; t++)
        th.emplace_back([=] {
            if (hipSetDevice(device) != hipSuccess) return;
            hipStream_t s = nullptr;
            uint8_t* dev = nullptr;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return;
            if (hipMalloc((void**)&dev, bytes) == hipSuccess) {
                for (int r = 0; r < kRounds; r++) {
                    if (hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s) != hipSuccess) break;
                    for (int k = 0; k < kKernels; k++) launch_touch_pages(dev, 2000, s);
                    if (hipStreamSynchronize(s) != hipSuccess) break;
                }
                hipFree(dev);
            }
            hipStreamDestroy(s);
        });
    for (auto& x : th) x.join();
    hipHostFree(host);
}

EncoderBackend* create_hip_backend(const h264::EncoderConfig& c, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= device)
        throw std::runtime_error("no HIP device available for the gfx950 backend");
    return new HipBackend(c, device);
}

}  // namespace sk
