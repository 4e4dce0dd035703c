// AV1 tail of the HIP back end (hip_session.h): the shared front end with integer vectors, then
// the AV1 back end (csrc/kernels/av1_kernels.hip) with its buffers, host-mapped frame info and
// tile bytes, the K10 accounting over the tile sizes, and the temporal unit of a frame.
#pragma once
#include "hip_session.h"
#include "../kernels/av1_gpu.h"
#include "../codec/av1_encoder.h"

namespace sk {
namespace hip_backend {

struct Av1Tail {
    explicit Av1Tail(const TailCtx& s) : s_(s) {}
    // CBR as the CPU encoder (av1_encoder.h)
    static EncoderConfig config(EncoderConfig c) {
        av1::cbr_config(c);
        return c;
    }

    // AV1 back-end buffers (av1_gpu.h): cells, levels, level contexts, token slots per
    // 16x16 unit, block-parallel coder state per tile, host-mapped frame info and tile bytes.
    void alloc(gpu::FrameArgs& f) {
        const EncoderConfig& cfg = s_.cfg;
        const Geometry& g = s_.g;
        HipAllocs& mem = s_.mem;
        f.deblock = 0;   // filters in its own back end
        f.subpel = 0;    // integer vectors (av1_encoder.h front_config)
        bufmap_ = f.ltr_cfg.mode == ltr::LTR_BUFMAP;
        const int n = g.num_mbs();
        av1::gpu::Av1Args& a = aargs_;
        memset(&a, 0, sizeof(a));
        av1::session_geo(geo_, g.W, g.H, cfg.tile_cols_log2, cfg.tile_rows_log2);
        a.geo = geo_;
        a.blk = mem.dmalloc<av1::BlkInfo>((size_t)geo_.c8 * geo_.r8);
        a.pal = mem.dmalloc<uint8_t>((size_t)geo_.c8 * geo_.r8 * 8);
        a.palette = av1::palette_enabled() ? 1 : 0;
        a.pal_rate = mem.dmalloc<int>((size_t)geo_.c8 * geo_.r8);
        a.tools = av1::session_tools(cfg, a.palette != 0);
        a.pal_uv = mem.dmalloc<uint8_t>((size_t)geo_.c8 * geo_.r8 * 16);
        a.pal_rate_uv = mem.dmalloc<int>((size_t)geo_.c8 * geo_.r8);
        if (av1::has_intra_inter(a.tools)) {   // av1_gpu.h: the inter coding's J, the intra candidates and their count per tile
            a.jinter = mem.dmalloc<long long>((size_t)geo_.c8 * geo_.r8);
            a.cand = mem.dmalloc<int>((size_t)geo_.c8 * geo_.r8);
            a.tile_cand = mem.dmalloc<int>((size_t)geo_.tile_cols * geo_.tile_rows);
        }
        a.lev = mem.dmalloc<int16_t>((size_t)n * av1::gpu::kLevPerUnit);
        a.lctx_w[0] = geo_.mi_cols;
        a.lctx_w[1] = a.lctx_w[2] = geo_.mi_cols >> 1;
        a.lctx[0] = mem.dmalloc<uint8_t>((size_t)geo_.mi_cols * geo_.mi_rows);
        a.lctx[1] = mem.dmalloc<uint8_t>((size_t)(geo_.mi_cols >> 1) * (geo_.mi_rows >> 1));
        a.lctx[2] = mem.dmalloc<uint8_t>((size_t)(geo_.mi_cols >> 1) * (geo_.mi_rows >> 1));
        a.tok = mem.dmalloc<uint32_t>((size_t)n * av1::gpu::kTokCap, false);
        a.tok_n = mem.dmalloc<int>(n);
        a.frame = mem.dmalloc<int>(4);
        a.cdef_in.y = mem.dmalloc<uint8_t>((size_t)g.stride_y * g.mb_h * 16, false);
        a.cdef_in.u = mem.dmalloc<uint8_t>((size_t)g.stride_c * g.mb_h * 8, false);
        a.cdef_in.v = mem.dmalloc<uint8_t>((size_t)g.stride_c * g.mb_h * 8, false);
        const int tiles = geo_.tile_cols * geo_.tile_rows;
        // tile bytes: 4 KB per unit of the largest tile (incompressible content codes
        // below ~1.5 bytes per sample)
        const int tile_units = (geo_.tile_w_sb * 4) * (geo_.tile_h_sb * 4);
        a.tile_tok_cap = tile_units * av1::gpu::kTokCap;
        a.tokc = mem.dmalloc<uint32_t>((size_t)tiles * a.tile_tok_cap, false);
        // + per-wave junk slots of k_av1_cdf (words of tokens a wave does not own)
        a.pw = mem.dmalloc<uint32_t>((size_t)tiles * a.tile_tok_cap + (size_t)tiles * 16 * 64, false);
        a.tok_off = mem.dmalloc<int>(n);
        a.tile_ntok = mem.dmalloc<int>(tiles);
        a.tile_cap = tile_units * 4096;
        if (tiles > 64) throw std::runtime_error("AV1: at most 64 tiles");
        av1::gpu::ec_buffers(tiles, a.tile_cap, &a.ec_max_blocks, &a.ec_vcap);
        a.ecmap = mem.dmalloc<uint2>((size_t)a.ec_max_blocks * 128, false);
        a.ecblk = mem.dmalloc<int4>((size_t)a.ec_max_blocks, false);
        a.ecv = mem.dmalloc<unsigned long long>((size_t)tiles * a.ec_vcap, false);
        a.ecf = mem.dmalloc<uint32_t>((size_t)tiles * a.ec_vcap, false);
        a.tile_bits = mem.dmalloc<int>(tiles);
        a.tile_size = mem.dmalloc<int>(tiles);
        a.out_cap = g.W * g.H * 3 + 4096;
        std::vector<uint8_t> q(52);
        for (int i = 0; i < 52; i++) q[i] = (uint8_t)av1::qidx_for_qp(i);
        uint8_t* dq = mem.dmalloc<uint8_t>(52);
        copy_now(dq, q.data(), 52, mem.stream);
        a.qidx_of_qp = dq;
        for (auto& o : out_) {
            o.data = mem.mapped<uint8_t>((size_t)a.out_cap);
            o.size = mem.mapped<int>(tiles, hipHostMallocCoherent);
            o.frame = mem.mapped<int>(8, hipHostMallocCoherent);
        }
        HIPCHECK(hipStreamSynchronize(mem.stream));
        level_ = av1::choose_level_idx(g.W, g.H, cfg.fps);
    }

    static constexpr bool kAccountInCommit = false;
    void enqueue_backend(const gpu::FrameArgs& args, int parity, hipStream_t stream, bool redo) {
        gpu::launch_frontend(args, stream);
        av1::gpu::Av1Args aa = aargs_;
        aa.f = args;
        aa.frame_host = out_[parity].frame.dev;
        aa.out_host = out_[parity].data.dev;
        aa.out_size_host = out_[parity].size.dev;
        av1::gpu::launch_backend(aa, stream, redo ? args.rc_redo : nullptr);
        gpu::launch_rc_account(args, aa.tile_size, geo_.tile_cols * geo_.tile_rows, 1, 0, stream);
    }

    // FrameArgs::deblock is 0: part 1 is k_commit alone either way, one graph of it is enough.
    bool can_filter(int, const int*) const { return true; }

    void build_packets(const FrameSlot& f, int parity, std::vector<EncodedPacket>& out) {
        const Geometry& g = s_.g;
        const Out& o = out_[parity];
        const int tiles = geo_.tile_cols * geo_.tile_rows;
        av1::FrameParams fp;
        fp.key = o.frame.host[0];
        fp.qidx = o.frame.host[1];
        fp.lf_level = o.frame.host[2];
        if (bufmap_) {   // long-term cache: the reference buffers k_av1_setup chose (ltr.h buffer map)
            fp.refresh = o.frame.host[3];
            fp.last_buf = o.frame.host[4];
            fp.last2_buf = o.frame.host[5];
        }
        fp.screen = av1::frame_screen(fp.key != 0, aargs_.tools, aargs_.palette != 0);
        std::vector<std::vector<uint8_t>> tl(tiles);
        size_t off = 0;
        for (int t = 0; t < tiles; t++) {
            const int n = o.size.host[t];
            if (n < 0) throw std::runtime_error("AV1 tile exceeded its output capacity");
            tl[t].assign(o.data.host + off, o.data.host + off + n);
            off += (size_t)n;
        }
        EncodedPacket pk;
        pk.y = 0; pk.w = g.W; pk.h = g.H; pk.key = fp.key;
        pk.data.resize(10);
        write_stripe_header(pk.data.data(), fp.key, f.frame, 0, g.W, g.H);
        av1::write_temporal_unit(pk.data, geo_, fp, tl, level_, s_.cfg.full_range);
        out.push_back(std::move(pk));
    }

    DebugEntry codec_debug(const std::string& s) const {
        const av1::gpu::Av1Args& v = aargs_;
        const int64_t nmb = s_.g.num_mbs(), tiles = geo_.tile_cols * geo_.tile_rows, blks = (int64_t)geo_.c8 * geo_.r8;
        const DebugEntry table[] = {
            {"av1_geo", &geo_, (int64_t)sizeof(geo_), true},
            {"blk", v.blk, (int64_t)(blks * sizeof(av1::BlkInfo))},
            {"levels", v.lev, nmb * av1::gpu::kLevPerUnit * 2},
            {"pal", v.pal, blks * 8},          // meaningful in cells whose PaletteSizeY is nonzero
            {"pal_uv", v.pal_uv, blks * 16},   // meaningful in cells whose PaletteSizeUV is nonzero
            {"tok_n", v.tok_n, nmb * 4},
            {"tokc", v.tokc, tiles * v.tile_tok_cap * 4},
            {"tile_ntok", v.tile_ntok, tiles * 4},
            {"frame", v.frame, 16},   // key, qidx, lf level, -
            {"av1_qidx", v.frame ? v.frame + 1 : nullptr, 4},   // the CPU back end's name for frame[1]
            {"tile_size", v.tile_size, tiles * 4},
        };
        return find_debug(table, s);
    }

   private:
    TailCtx s_;
    av1::gpu::Av1Args aargs_ = {};
    av1::Av1Geo geo_ = {};
    int level_ = 8;
    bool bufmap_ = false;   // long-term cache in the buffer-map mode (ltr.h)
    struct Out {   // host-mapped: tile bytes, tile sizes, frame info
        Mapped<uint8_t> data;
        Mapped<int> size, frame;
    } out_[2];
};

}  // namespace hip_backend
}  // namespace sk
