// H.264 tail of the HIP back end (hip_session.h): the coding chain's buffers (MB records,
// levels, CAVLC slots and tables, deblocking side info, parameter sets), the host-mapped packet
// slots, launch_encode, the commit policy (K10 accounting in k_commit, short commit graph for
// frames no slice of which can be filtered) and the packets.
#pragma once
#include "hip_session.h"

namespace sk {
namespace hip_backend {

struct H264Tail {
    explicit H264Tail(const TailCtx& s) : s_(s) {}
    static EncoderConfig config(EncoderConfig c) { return c; }

    void alloc(gpu::FrameArgs& a) {
        const EncoderConfig& cfg = s_.cfg;
        const Geometry& g = s_.g;
        HipAllocs& mem = s_.mem;
        const int nmb = g.num_mbs(), ns = g.num_slices;
        a.aq = mem.dmalloc<int8_t>(nmb);
        a.db = mem.dmalloc<DbInfo>(nmb);
        a.dbe = mem.dmalloc<uint4>((size_t)3 * nmb);
        a.mbs = mem.dmalloc<MbInfo>(nmb);
        a.coefs = mem.dmalloc<int16_t>((size_t)nmb * kCoefPerMb);
        a.mb_bits = mem.dmalloc<uint32_t>((size_t)nmb * (gpu::kMbSlotBytes / 4));
        a.mb_nbits = mem.dmalloc<int>(nmb);
        int max_slice_mbs = g.rows_per_slice * g.mb_w;
        // K5: split I slices put one NAL per sub-slice (h264_encoder.h intra_split)
        const bool can_split = g.mb_w > kIntraSubMbs;
        a.nal_per_slice = can_split ? max_nals_per_slice(g.rows_per_slice, g.mb_w) : 1;
        if (max_slice_mbs > gpu::kPackMaxSliceMbs)
            throw std::runtime_error("H.264: more than " + std::to_string(gpu::kPackMaxSliceMbs) +
                                     " macroblocks per slice is not supported");   // k_slice_pack's bbase[]
        a.slice_info = mem.dmalloc<int>(4 * (size_t)ns * a.nal_per_slice);
        // A slice's RBSP at its worst: every MB fills its CAVLC slot, plus the slice header
        // (per sub-slice NAL where I slices are split). The RBSP itself only exists in LDS
        // (k_slice_pack); the bound sizes the host slot.
        const size_t sub_rbsp = (size_t)kIntraSubMbs * gpu::kMbSlotBytes + 1024;
        const size_t max_rbsp = std::max((size_t)max_slice_mbs * gpu::kMbSlotBytes + 1024,
                                         can_split ? a.nal_per_slice * sub_rbsp : (size_t)0);
        // worst case: header + SPS/PPS + 3/2 emulation-prevention growth, 64-byte multiple
        size_t slot = (max_rbsp * 3 / 2 + 1024 + 63) & ~(size_t)63;
        a.out_slot_bytes = (int)slot;
        for (auto& o : out_) {   // host outputs per parity (two frames in flight)
            o.data = mem.mapped<uint8_t>(slot * ns);
            o.size = mem.mapped<int>(ns);
        }
        // parameter sets
        std::vector<std::vector<uint8_t>> ps;
        if (cfg.fullframe) {
            ps.resize(1);
            build_parameter_sets(g.W, g.H, cfg.full_range, cfg.fps, ps[0], cfg.num_refs, ltr_slots_of(cfg));
        } else {
            ps.resize(ns);
            for (int s = 0; s < ns; s++)
                build_parameter_sets(g.W, g.slice_pix_h(s), cfg.full_range, cfg.fps, ps[s], cfg.num_refs,
                                     ltr_slots_of(cfg));
        }
        param_sets_ = ps;
        a.param_set_stride = 256;
        std::vector<uint8_t> flat((size_t)ns * 256, 0);
        std::vector<int> lens(ns, 0);
        for (int s = 0; s < ns; s++) {
            const std::vector<uint8_t>& v = ps[cfg.fullframe ? 0 : s];
            if (v.size() > 256) throw std::runtime_error("parameter sets too large");
            memcpy(&flat[(size_t)s * 256], v.data(), v.size());
            lens[s] = (int)v.size();
        }
        uint8_t* dps = mem.dmalloc<uint8_t>(flat.size());
        copy_now(dps, flat.data(), flat.size(), mem.stream);
        int* dlen = mem.dmalloc<int>(ns);
        copy_now(dlen, lens.data(), sizeof(int) * ns, mem.stream);
        a.param_sets = dps;
        a.param_set_len = dlen;
        CavlcTables* ct = mem.dmalloc<CavlcTables>(1);
        copy_now(ct, &host_cavlc_tables(), sizeof(CavlcTables), mem.stream);
        a.cavlc_tabs = ct;
        mbs_ = a.mbs;
        coefs_ = a.coefs;
        slot_bytes_ = slot;
    }

    // The K10 accounting of the chain runs in k_commit (both commit graphs), behind k_slice_pack.
    static constexpr bool kAccountInCommit = true;
    void enqueue_backend(const gpu::FrameArgs& args, int parity, hipStream_t stream, bool redo) {
        gpu::FrameArgs a = args;
        a.host_out = out_[parity].data.dev;
        a.host_size = out_[parity].size.dev;
        gpu::launch_encode(a, stream, redo);
    }

    // Whether a slice of the frame launched with key snapshot `snap` (FrameSlot::key_snap) can be
    // deblocked, i.e. whether part 1 needs its deblocking kernels. Off: never. On: always.
    // Automatic (slices at QP >= kAutoDeblockQp): not when max_slice_qp, for the frame's
    // rate mode and QPs, stays below the threshold - every CQP / CRF session at the default
    // QPs. CBR reaches every QP and always takes the long graph. rc_mode: the device
    // controller's at that frame.
    bool can_filter(int rc_mode, const int* snap) const {
        if (s_.cfg.deblock != 2) return s_.cfg.deblock != 0;
        const int qp = snap[1] > 0 ? snap[1] : s_.cfg.qp, pqp = snap[2] > 0 ? snap[2] : s_.cfg.paint_qp;
        return max_slice_qp(rc_mode, qp, pqp) >= kAutoDeblockQp;
    }

    void build_packets(const FrameSlot& f, int parity, std::vector<EncodedPacket>& out) {
        const Geometry& g = s_.g;
        const uint8_t* host_out = out_[parity].data.host;
        const int* h_out_size = out_[parity].size.host;
        const SliceTask* h_tasks = f.tasks.host;
        const int ns = g.num_slices;
        std::vector<long> offs(ns);
        for (int s = 0; s < ns; s++) offs[s] = (long)(s * slot_bytes_);
        if (s_.cfg.fullframe) {
            bool idr = s_.ctl.picture_is_idr(h_tasks);
            EncodedPacket pk;
            pk.y = 0; pk.w = g.W; pk.h = g.H; pk.key = idr;
            pk.data.resize(10);
            write_stripe_header(pk.data.data(), idr, f.frame, 0, g.W, g.H);
            if (idr) pk.data.insert(pk.data.end(), param_sets_[0].begin(), param_sets_[0].end());
            for (int s = 0; s < ns; s++) {
                const uint8_t* p = host_out + offs[s];
                pk.data.insert(pk.data.end(), p, p + h_out_size[s]);
            }
            out.push_back(std::move(pk));
            return;
        }
        for (int s = 0; s < ns; s++) {
            if (h_tasks[s].final_action == ACT_NONE || h_out_size[s] <= 0) continue;
            EncodedPacket pk;
            pk.y = g.slice_pix_y(s);
            pk.w = g.W;
            pk.h = g.slice_pix_h(s);
            pk.key = h_tasks[s].final_action == ACT_I && h_tasks[s].idr_on_intra;   // non-IDR I: long-term cache on
            const uint8_t* p = host_out + offs[s];
            pk.data.assign(p, p + h_out_size[s]);
            out.push_back(std::move(pk));
        }
    }

    DebugEntry codec_debug(const std::string& s) const {
        const int64_t nmb = s_.g.num_mbs();
        const DebugEntry table[] = {
            {"mbs", mbs_, (int64_t)(nmb * sizeof(MbInfo))},
            {"coefs", coefs_, nmb * kCoefPerMb * 2},
        };
        return find_debug(table, s);
    }

   private:
    TailCtx s_;
    const MbInfo* mbs_ = nullptr;      // FrameArgs::mbs, coefs and out_slot_bytes, for the host side
    const int16_t* coefs_ = nullptr;
    size_t slot_bytes_ = 0;
    struct Out {   // host-mapped: packet slots and their sizes
        Mapped<uint8_t> data;
        Mapped<int> size;
    } out_[2];
    std::vector<std::vector<uint8_t>> param_sets_;
};

}  // namespace hip_backend
}  // namespace sk
