// HIP back end of the stripe encoders, the codec-neutral part: HipBackend<Tail> is one encoder
// session on the GPU. It owns the stream, the upload path and its damage-driven copies, the two
// parity slots with their graphs, overlays, the key / QP / rate snapshots, state export / import
// and the buffers of the shared front end (csrc/kernels/h264_kernels.hip up to k_subpel, the
// long-term cache). What only one codec needs lives in its tail (h264_tail.h, hevc_tail.h,
// av1_tail.h), as the CPU side has CpuBackend<Enc> (sk_api.cpp). Frame flow:
//   H2D(BGRx) -> (overlay placement, only when it changed) -> [k_convert_damage, then the tail's
//   enqueue_backend: k_plan (stripe controller on the GPU), k_me, k_decide, k_rc_qp, k_subpel and
//   the codec's coding kernels, into host-mapped packet slots] (one hipGraph per parity slot)
//   -> one sync -> Tail::build_packets; behind it, not waited on: k_commit (+ for H.264 the K10
//   accounting, and K7 deblocking when a slice of the frame can be filtered), a second graph.
//   No host decision sits inside a frame.
//
// A codec tail is a plain struct, constructed from a TailCtx, that provides
//   static EncoderConfig config(EncoderConfig c)   the codec's normalisation of the configuration
//   void alloc(gpu::FrameArgs& a)                  its front-end overrides in `a` (defaults: the
//                                                  configuration's; nal_per_slice 1), its device
//                                                  buffers and per-parity host outputs, all from
//                                                  TailCtx::mem, so the session frees them
//   void enqueue_backend(const gpu::FrameArgs& args, int parity, hipStream_t s, bool redo)
//                                                  everything of part 0 behind launch_convert_damage,
//                                                  the K10 accounting of the frame included unless
//                                                  kAccountInCommit; redo: with the K10 CBR guard
//   static constexpr bool kAccountInCommit         k_commit does the K10 accounting
//   bool can_filter(int rc_mode, const int* snap)  part 1 of this frame needs launch_commit's
//                                                  deblocking kernels (false: the short graph)
//   void build_packets(const FrameSlot& f, int parity, std::vector<EncodedPacket>& out)
//   DebugEntry codec_debug(const std::string& name) const   debug_buffer names of its own buffers
#pragma once
#include "encoder_iface.h"
#include "trace.h"
#include "hip_util.h"
#include "../kernels/h264_gpu.h"
#include <atomic>
#include <map>
#include <mutex>

namespace sk {
namespace hip_backend {

using namespace h264;

// Everything of one frame in flight that every codec has. Frame k uses slot k & 1: its upload
// overlaps the other slot's graph, and the host reads its packets while the other slot's frame
// encodes. A tail keeps its host outputs in a two-element array of its own, by the same parity.
struct FrameSlot {
    uint8_t* bgrx = nullptr;   // input frame
    uint8_t* yuv = nullptr;    // planar input staging (upload_yuv)
    gpu::Planes src = {};      // converted source; `prev` of the next frame
    bool up_valid = false;     // bgrx holds a complete frame (upload_copy)
    uint16_t frame = 0;        // frame id of the launched frame
    // host-mapped: final decisions from k_decide, frame id for k_plan, and the key-frame / QP /
    // rate snapshot taken at launch
    Mapped<SliceTask> tasks;
    Mapped<int> frame_params, key_snap;
    hipEvent_t uploaded = nullptr, started = nullptr, packets_done = nullptr;   // stage_times()
    hipEvent_t copied = nullptr;   // upload on another stream than the encoder's
    // part 0 (frame -> packets), part 1 (commit + deblocking), part 1 without the deblocking kernels
    hipGraphExec_t graph = nullptr, post = nullptr, post_short = nullptr;
};

// What a tail sees of its session. mem.stream is the session's stream.
struct TailCtx {
    const EncoderConfig& cfg;   // after Tail::config
    const Geometry& g;
    const Controller& ctl;
    HipAllocs& mem;
};

// A debug_buffer name that is one buffer of a fixed size, in device memory unless `host`.
// ptr null: no such name, or a buffer this configuration does not have.
struct DebugEntry {
    const char* name;
    const void* ptr;
    int64_t bytes;
    bool host = false;
};
template <class Table>
DebugEntry find_debug(const Table& table, const std::string& s) {
    for (const DebugEntry& e : table)
        if (s == e.name) return e;
    return {};
}

// Blocking copies are ordered on the encoder's own stream: a copy on the legacy
// stream fails while any stream of the process is capturing a graph (several
// sessions share one process in parallel/multi.py session hosts). No extra stream:
// every stream takes a slot in the process's round-robin over its hardware queues,
// and an idle one per session halved the queues the sessions' work spread over
// (8 x 1080p: 4150 -> 3650 fps).
inline void copy_now(void* dst, const void* src, size_t n, hipStream_t stream) {
    HIPCHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDefault, stream));
    HIPCHECK(hipStreamSynchronize(stream));
}

template <class Tail>
class HipBackend : public EncoderBackend {
   public:
    HipBackend(const EncoderConfig& c, int device)
        : cfg_(Tail::config(c)), device_(device), tail_(TailCtx{cfg_, g_, ctl_, mem_}) {
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
        build_debug_table();
    }
    ~HipBackend() override {
        hipSetDevice(device_);
        // a launched, uncollected frame may still replay the graphs and read the buffers freed
        // below (the tail's are among them), and an overlapped upload may still write an input buffer
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
        // convert/damage -> plan -> ME -> code -> entropy coding -> assembly -> commit: one graph,
        // one sync; k_decide leaves the final slice decisions in f.tasks.
        // MV field / reference update and K7 deblocking run after the packets are done:
        // the host only waits for packets_done; the next frame's work queues behind the update.
        // (An event record captured inside one fused graph did not order the host wait
        // after part 0 on ROCm 7: packets read back empty. Two launches it is.)
        run_graph(f.graph, 0);
        HIPCHECK(hipEventRecord(f.packets_done, stream_));
        // The rate mode of the device controller at this frame: k_plan takes the snapshot's mode
        // when its set_rate() counter moved (as here), else keeps its own (initial, or imported
        // with a state).
        if (f.key_snap.host[5] != dev_rc_seq_) {
            dev_rc_seq_ = f.key_snap.host[5];
            dev_rc_mode_ = f.key_snap.host[3];
        }
        // Part 1 without the deblocking kernels when no slice of this frame can be filtered.
        if (tail_.can_filter(dev_rc_mode_, f.key_snap.host)) run_graph(f.post, 1);
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
            tail_.build_packets(f, finished_ & 1, packets_);
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
                dev_rc_mode_ = rc.mode;   // launch(): the device controller now runs in the imported mode
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

    // The front end's names are resolved here, the codec's own by Tail::codec_debug.
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
        if (s == "ltr_state" && args_.ltr_cfg.slots) {
            const std::vector<ltr::LtrState> ls = committed_ltr_state(pending_commit());
            return from_host(ls.data(), ls.size() * sizeof(ltr::LtrState));
        }
        DebugEntry e = {};
        const int64_t ny = (int64_t)g_.stride_y * g_.plane_h_y, nc = (int64_t)g_.stride_c * g_.plane_h_c;
        // after a frame the parity flipped: the last source is in `prev` of the next frame
        const gpu::Planes& last_src = slot_[parity_ ^ 1].src;
        if (s == "src_y") e = {name, last_src.y, ny};
        else if (s == "src_u") e = {name, last_src.u, nc};
        else if (s == "src_v") e = {name, last_src.v, nc};
        else if (s.size() == 6 && s.compare(0, 3, "ltr") == 0 && s.compare(4, 2, "_y") == 0 && s[3] >= '0' &&
                 s[3] < '0' + args_.ltr_cfg.slots) e = {name, args_.ltr.y + (size_t)(s[3] - '0') * ny, ny};
        else e = find_debug(debug_, s);
        if (!e.ptr) e = tail_.codec_debug(s);
        if (!e.ptr) return -1;   // unknown, or a buffer this configuration does not have (stamps without SK_STAMPS)
        if (e.host) return from_host(e.ptr, (size_t)e.bytes);
        if (dst && cap >= e.bytes) HIPCHECK(hipMemcpyAsync(dst, e.ptr, (size_t)e.bytes, hipMemcpyDeviceToHost, stream_));
        HIPCHECK(hipStreamSynchronize(stream_));
        return e.bytes;
    }

   private:
    void copy_now(void* dst, const void* src, size_t n) { hip_backend::copy_now(dst, src, n, stream_); }

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

    // The front end's debug_buffer names that are one device buffer of a fixed size. `aq` is
    // written by the H.264 coding chain only and null elsewhere, as on the CPU back ends.
    void build_debug_table() {
        const gpu::FrameArgs& a = args_;
        const int64_t nmb = g_.num_mbs(), ny = (int64_t)g_.stride_y * g_.plane_h_y, nc = (int64_t)g_.stride_c * g_.plane_h_c;
        debug_ = {
            {"ref_y", a.ref.y, ny}, {"ref_u", a.ref.u, nc}, {"ref_v", a.ref.v, nc},
            {"ref1_y", a.ref1.y, ny},
            {"ltr_task", a.ltr_task, (int64_t)(g_.num_slices * sizeof(ltr::LtrTask))},
            {"fs_mv", a.fs_mv, nmb * 4},
            {"me", a.me, (int64_t)(nmb * sizeof(MeResult))},
            {"mb_dirty", a.mb_dirty, nmb},
            {"aq", a.aq, nmb},
            {"stamps", a.dbg, (64 * 16 + 256) * 8},
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
        a.me_full = cfg_.me_full;
        // the configuration's, unless the tail's alloc() overrides them
        a.deblock = cfg_.deblock;
        a.aq_strength = cfg_.aq_strength;
        a.subpel = cfg_.subpel;
        a.intra4x4 = cfg_.intra4x4;
        a.nal_per_slice = 1;
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
        if (getenv("SK_STAMPS")) a.dbg = mem_.dmalloc<unsigned long long>(64 * 16 + 256);
        a.frame_params_dev = mem_.dmalloc<int>(4);
        for (auto& f : slot_) {
            f.tasks = mem_.mapped<SliceTask>(ns, hipHostMallocCoherent);  // final decisions from k_decide
            f.frame_params = mem_.mapped<int>(4, hipHostMallocCoherent);
        }
        tail_.alloc(a);
    }

    // The one place that maps the slot of parity_ onto FrameArgs; the tail adds its own host
    // outputs of that parity in enqueue_backend.
    void set_parity_args() {
        const FrameSlot& f = slot_[parity_];
        args_.yuv = f.yuv;
        args_.yuv_fmt = yuv_mode_;
        args_.bgrx = f.bgrx;
        args_.src = f.src;
        args_.prev = slot_[parity_ ^ 1].src;
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
    // alone, for frames in which no slice can be filtered (Tail::can_filter).
    // Every host reader of the controller state (rc_stats, export_state) synchronises the
    // stream, so it reads behind part 1 and the K10 accounting, wherever the tail runs that.
    // Stripe flags are cleared by k_plan. The overlay placement is not part of the graph:
    // launch() copies it ahead of the graph when it changed.
    void enqueue(int part) {
        if (part == 0) {
            gpu::launch_convert_damage(args_, stream_);
            tail_.enqueue_backend(args_, parity_, stream_, graph_guard_);
        } else {
            gpu::launch_commit(args_, stream_, part == 1, Tail::kAccountInCommit);
        }
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
    std::vector<DebugEntry> debug_;

    // ---- device state ----
    HipAllocs mem_;
    hipStream_t stream_ = nullptr;
    hipStream_t copy_stream_ = nullptr;   // shared per device (not owned)
    hipStream_t up_stream_ = nullptr;     // this session's upload stream (owned, lazily created)
    gpu::FrameArgs args_;
    Tail tail_;                  // the codec's buffers, back-end launches and packet assembly
    int* h_key_seq_ = nullptr;   // host-coherent: key-frame counter, QP overrides, rate mode / kbps / counter
    int dev_rc_mode_ = 0, dev_rc_seq_ = 0;   // rate mode of the device controller and the set_rate() counter it has seen
    bool graph_guard_ = false;   // the captured graphs contain the K10 CBR guard
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

}  // namespace hip_backend
}  // namespace sk
