// HEVC tail of the HIP back end (hip_session.h): the shared front end, then the HEVC back end
// (csrc/kernels/hevc_kernels.hip) with its buffers, host-mapped slice slots with a device
// fallback, the K10 accounting over the substream sizes, and the one packet of a picture.
#pragma once
#include "hip_session.h"
#include "../kernels/hevc_gpu.h"
#include "../codec/hevc_encoder.h"

namespace sk {
namespace hip_backend {

struct HevcTail {
    explicit HevcTail(const TailCtx& s) : s_(s) {}
    // CBR without scene-cut intra slices, stripes of whole CTB rows (hevc_encoder.h)
    static EncoderConfig config(EncoderConfig c) {
        hevc::cbr_config(c);
        hevc::hevc_geometry(c);
        return c;
    }

    // HEVC back-end buffers (hevc_gpu.h): CU decisions, levels, bin slots, WPP states,
    // one substream slot per CTB row, host-mapped slice slots + device fallback.
    void alloc(gpu::FrameArgs& a) {
        const Geometry& g = s_.g;
        HipAllocs& mem = s_.mem;
        a.deblock = 0;   // filters in its own back end
        a.aq_strength = 0;
        a.intra4x4 = 0;
        const int n = g.num_mbs(), ns = g.num_slices;
        hevc::Geo geo;
        geo.init(g);
        hevc::gpu::HevcArgs& h = hargs_;
        memset(&h, 0, sizeof(h));
        h.cw = geo.ctb_w;
        h.ch = geo.ctb_h;
        h.rps = geo.rows_per_slice;
        if (g.rows_per_slice & 1) throw std::runtime_error("HEVC: stripes must be whole CTB rows");
        const int nc = geo.ctbs();
        h.cus = mem.dmalloc<hevc::CuInfo>(n);
        h.coefs = mem.dmalloc<int16_t>((size_t)n * hevc::kCoefPerCu);
        h.bins = mem.dmalloc<uint16_t>((size_t)n * hevc::kCuBinCap, false);
        h.bin_n = mem.dmalloc<int>(n);
        // intra slices: seg_k slices per CTB row (hevc_core.h SliceMap); per-substream
        // arrays hold ch * seg_k slots
        h.seg_k = hevc::intra_seg_k(h.cw, h.ch);
        if (h.rps * h.seg_k > 256) throw std::runtime_error("HEVC: more than 256 row segments per slice");
        const size_t slots = (size_t)h.ch * h.seg_k;
        h.sync = mem.dmalloc<uint8_t>(slots * hevc::CTX_COUNT);
        h.sub_stride = h.cw * 4 * hevc::kSubstreamCtbBytes + 64 * h.seg_k + 64;
        h.sub = mem.dmalloc<uint8_t>((size_t)h.ch * h.sub_stride, false);
        h.sub_size = mem.dmalloc<int>(slots);
        h.sub_esc = mem.dmalloc<int>(slots);
        h.row_off = mem.dmalloc<int>(slots);
        h.addr_bits = geo.addr_bits;
        if (2 * g.mb_w > 1024) throw std::runtime_error("HEVC: more than 1024 units per CTB row (8K) is not supported");
        h.srt = mem.dmalloc<uint16_t>((size_t)n * hevc::kCuBinCap, false);
        h.coff = mem.dmalloc<uint16_t>((size_t)h.ch * hevc::kPcCtxOff * 2 * g.mb_w, false);
        h.rmap = mem.dmalloc<uint32_t>((size_t)n * 256, false);
        h.cu_t = mem.dmalloc<uint32_t>(n);
        h.cu_r = mem.dmalloc<uint16_t>(n);
        h.tail = mem.dmalloc<uint8_t>((size_t)n * 2);
        h.row_bits = mem.dmalloc<uint32_t>(slots);
        h.sao_stats = mem.dmalloc<hevc::SaoStats>((size_t)3 * nc, false);
        h.sao_own = mem.dmalloc<hevc::SaoParams>(nc);
        h.sao_cost = mem.dmalloc<long long>(nc);
        h.sao_md = mem.dmalloc<long long>((size_t)nc * hevc::kSaoMd);
        h.sao = mem.dmalloc<hevc::SaoParams>(nc);
        h.sao_tmp.y = mem.dmalloc<uint8_t>((size_t)g.stride_y * g.mb_h * 16, false);
        h.sao_tmp.u = mem.dmalloc<uint8_t>((size_t)g.stride_c * g.mb_h * 8, false);
        h.sao_tmp.v = mem.dmalloc<uint8_t>((size_t)g.stride_c * g.mb_h * 8, false);
        // host slot: 1.5 KB per CTB (far above practical rates); larger slices go to the
        // device fallback slot (worst case: 3/2 emulation growth of the substream bound)
        h.out_slot = (g.rows_per_slice * g.mb_w * 1536 + 4096 + 63) & ~63;
        h.out_dev_slot = (int)(((size_t)h.rps * h.sub_stride * 3 / 2 + 4096 + 63) & ~(size_t)63);
        for (auto& o : out_) {
            o.data = mem.mapped<uint8_t>((size_t)h.out_slot * ns);
            o.size = mem.mapped<int>(ns, hipHostMallocCoherent);
            o.fallback = mem.dmalloc<uint8_t>((size_t)h.out_dev_slot * ns, false);
        }
        HIPCHECK(hipStreamSynchronize(mem.stream));
        if (getenv("SK_STAMPS")) h.dbg = mem.dmalloc<unsigned long long>((size_t)4 * h.ch);
        h.reg_steps = getenv("SK_HEVC_REG_STEPS") ? atoi(getenv("SK_HEVC_REG_STEPS")) : 1;
        h.pc_seg = getenv("SK_HEVC_PC_SEG") ? sk_max(atoi(getenv("SK_HEVC_PC_SEG")), 1) : 32;
        params_.clear();
        hevc::build_parameter_sets(g.W, g.H, s_.cfg.full_range, s_.cfg.fps, params_, ltr_slots_of(s_.cfg));
    }

    static constexpr bool kAccountInCommit = false;
    void enqueue_backend(const gpu::FrameArgs& args, int parity, hipStream_t stream, bool redo) {
        gpu::launch_frontend(args, stream);
        hevc::gpu::HevcArgs ha = hargs_;
        ha.f = args;
        ha.out_host = out_[parity].data.dev;
        ha.out_size = out_[parity].size.dev;
        ha.out_dev = out_[parity].fallback;
        hevc::gpu::launch_backend(ha, stream, redo ? args.rc_redo : nullptr);
        gpu::launch_rc_account(args, ha.sub_size, ha.ch * ha.seg_k, 1, 0, stream);
    }

    // FrameArgs::deblock is 0: part 1 is k_commit alone either way, one graph of it is enough.
    bool can_filter(int, const int*) const { return true; }

    void build_packets(const FrameSlot& f, int parity, std::vector<EncodedPacket>& out) {
        const Geometry& g = s_.g;
        const Out& o = out_[parity];
        const int ns = g.num_slices;
        const bool idr = s_.ctl.picture_is_idr(f.tasks.host);
        EncodedPacket pk;
        pk.y = 0; pk.w = g.W; pk.h = g.H; pk.key = idr;
        pk.data.resize(10);
        write_stripe_header(pk.data.data(), idr, f.frame, 0, g.W, g.H);
        if (idr) pk.data.insert(pk.data.end(), params_.begin(), params_.end());
        for (int s = 0; s < ns; s++) {
            const int n = o.size.host[s];
            const size_t at = pk.data.size();
            pk.data.resize(at + (size_t)n);
            if (n <= hargs_.out_slot) {
                memcpy(pk.data.data() + at, o.data.host + (size_t)s * hargs_.out_slot, (size_t)n);
            } else {   // rare: the slice did not fit its host slot
                copy_now(pk.data.data() + at, o.fallback + (size_t)s * hargs_.out_dev_slot, (size_t)n, s_.mem.stream);
            }
        }
        out.push_back(std::move(pk));
    }

    DebugEntry codec_debug(const std::string& s) const {
        const hevc::gpu::HevcArgs& h = hargs_;
        const int64_t nmb = s_.g.num_mbs(), segs = (int64_t)h.ch * h.seg_k;
        const DebugEntry table[] = {
            {"coefs", h.coefs, nmb * hevc::kCoefPerCu * 2},
            {"cus", h.cus, (int64_t)(nmb * sizeof(hevc::CuInfo))},
            {"sao", h.sao, (int64_t)((int64_t)h.cw * h.ch * sizeof(hevc::SaoParams))},
            {"bin_n", h.bin_n, nmb * 4},
            {"cu_t", h.cu_t, nmb * 4},
            {"cu_r", h.cu_r, nmb * 2},
            {"tail", h.tail, nmb * 2},
            {"sub", h.sub, (int64_t)h.ch * h.sub_stride},
            {"sub_size", h.sub_size, segs * 4},
            {"row_bits", h.row_bits, segs * 4},
            {"hevc_stamps", h.dbg, (int64_t)h.ch * 32},
        };
        return find_debug(table, s);
    }

   private:
    TailCtx s_;
    hevc::gpu::HevcArgs hargs_ = {};
    struct Out {   // host-mapped slice slots and their sizes, device fallback slots
        Mapped<uint8_t> data;
        Mapped<int> size;
        uint8_t* fallback = nullptr;
    } out_[2];
    std::vector<uint8_t> params_;   // VPS / SPS / PPS
};

}  // namespace hip_backend
}  // namespace sk
