// C ABI implementation: encoder factory (CPU reference / HIP backend), packet
// access and debug hooks used by the Python layer and the tests.
#include "sk_api.h"
#include "encoder_iface.h"
#include "../codec/hevc_encoder.h"
#include "../codec/av1_encoder.h"
#include <hip/hip_runtime_api.h>
#include <string.h>
#include <string>
#include <mutex>
#include <stdlib.h>
#include <type_traits>
#include <utility>

namespace sk {

static thread_local std::string g_last_error;
void set_last_error(const std::string& e) { g_last_error = e; }

namespace {

// Planar input for a CPU encoder: device planes are copied to host memory first.
struct HostYuv {
    std::vector<uint8_t> buf[3];
    h264::YuvInput in;
    int load(const h264::YuvInput& src, int on_device, int W, int H) {
        in = src;
        if (!on_device) return 0;
        const int cw = (W + 1) / 2, ch = (H + 1) / 2;
        const int nplanes = src.fmt == h264::YUV_NV12 ? 2 : 3;
        for (int p = 0; p < nplanes; p++) {
            const int w = p == 0 ? W : (src.fmt == h264::YUV_NV12 ? 2 * cw : cw), h = p == 0 ? H : ch;
            buf[p].resize((size_t)w * h);
            if (hipMemcpy2D(buf[p].data(), w, src.p[p], src.stride[p], w, h, hipMemcpyDeviceToHost) != hipSuccess) {
                set_last_error("device planes: copy to the host failed");
                return -1;
            }
            in.p[p] = buf[p].data();
            in.stride[p] = w;
        }
        return 0;
    }
};

// The shared front end of a CPU encoder (references, controller, K10, damage baseline): the
// H.264 encoder itself, `fe` of the HEVC and AV1 encoders.
h264::CpuH264Encoder& front(h264::CpuH264Encoder& e) { return e; }
template <class Enc>
h264::CpuH264Encoder& front(Enc& e) { return e.fe; }

// debug_buffer view: data and byte count (-1: no such name)
using DebugBuf = std::pair<const void*, int64_t>;
template <class V>
DebugBuf bytes_of(const V& v) { return {v.data(), (int64_t)(v.size() * sizeof(*v.data()))}; }

// The debug_buffer names of each codec's own buffers; the front end's are resolved by CpuBackend.
// The long-term cache's buffers live in the front end.
DebugBuf ltr_debug(h264::CpuH264Encoder& e, const std::string& s) {
    if (s == "ltr_state") return bytes_of(e.ltr_state);
    if (s == "ltr_task") return bytes_of(e.ltr_task);
    if (s.size() == 6 && s.compare(0, 3, "ltr") == 0 && s.compare(4, 2, "_y") == 0 && s[3] >= '0' &&
        s[3] < '0' + e.ltr_cfg.slots) return bytes_of(e.ltr_planes[s[3] - '0'][0]);
    return {nullptr, -1};
}
DebugBuf codec_debug(h264::CpuH264Encoder& e, const std::string& s) {
    if (s == "ref1_y") return bytes_of(e.ref1[0]);
    if (s.compare(0, 3, "ltr") == 0) return ltr_debug(e, s);
    if (s == "mbs") return bytes_of(e.mbs);
    if (s == "coefs") return bytes_of(e.coefs);
    if (s == "mb_dirty") return bytes_of(e.mb_dirty);
    if (s == "aq") return bytes_of(e.aq);
    if (s == "fs_mv") return bytes_of(e.fs_mv);
    return {nullptr, -1};
}
DebugBuf codec_debug(hevc::CpuHevcEncoder& e, const std::string& s) {
    if (s == "cus") return bytes_of(e.cus);
    if (s == "sao") return bytes_of(e.sao);
    if (s == "coefs") return bytes_of(e.coefs);
    if (s == "bin_n") return bytes_of(e.bin_n);
    if (s == "bins") return bytes_of(e.bins);   // the binariser's entries (hevc_core.h BinBuf): context indices, not states
    if (s == "pc_dbg") return bytes_of(e.pc_dbg_);
    if (s.compare(0, 3, "ltr") == 0) return ltr_debug(e.fe, s);
    return {nullptr, -1};
}
DebugBuf codec_debug(av1::CpuAv1Encoder& e, const std::string& s) {
    if (s == "blk") return bytes_of(e.blk);
    if (s == "levels") return bytes_of(e.lev);
    if (s == "pal") return bytes_of(e.pal);         // meaningful in cells whose PaletteSizeY is nonzero
    if (s == "pal_uv") return bytes_of(e.pal_uv);   // meaningful in cells whose PaletteSizeUV is nonzero
    if (s == "av1_geo") return {&e.geo, (int64_t)sizeof(av1::Av1Geo)};
    if (s == "av1_qidx") return {&e.fp.qidx, 4};
    if (s.compare(0, 3, "ltr") == 0) return ltr_debug(e.fe, s);
    return {nullptr, -1};
}

// After a state import. HEVC: the next POC is the picture state's frame_num (the GPU back end
// codes POC from it).
template <class Enc>
void after_import(Enc&) {}
void after_import(hevc::CpuHevcEncoder& e) {
    std::vector<h264::StripeState> st(e.fe.g.num_slices + 1);
    e.fe.ctl_.export_states(st.data());
    e.poc = st.back().frame_num;
}

// CPU reference back end of one codec: Enc is its encoder, `ctor` its arguments after the configuration.
template <class Enc>
class CpuBackend : public EncoderBackend {
   public:
    template <class... A>
    explicit CpuBackend(const h264::EncoderConfig& c, A... ctor) : enc_(c, ctor...) {}
    void request_keyframe() override { enc_.request_keyframe(); }
    void set_qp(int qp, int paint_qp) override { enc_.set_qp(qp, paint_qp); }
    void set_rate(int mode, int kbps) override { fe().ctl_.set_rate(mode, kbps); }
    int64_t rc_stats(int32_t* out, int n) override {
        const int k = n < (int)(sizeof(h264::RcState) / 4) ? n : (int)(sizeof(h264::RcState) / 4);
        memcpy(out, &fe().ctl_.rc(), (size_t)k * 4);
        return k;
    }
    int set_overlay_image(int slot, const uint8_t* bgra, int w, int h) override {
        fe().set_overlay_image(slot, bgra, w, h);
        return 0;
    }
    int set_overlay_pos(int slot, int on, int x, int y, int tdx, int tdy) override {
        fe().set_overlay_pos(slot, on, x, y, tdx, tdy);
        return 0;
    }
    int encode(const uint8_t* bgrx, int stride, uint16_t frame_id) override {
        if (refuse_queued("encode()")) return -1;
        packets_.clear();
        enc_.encode(bgrx, stride, frame_id, packets_);
        return (int)packets_.size();
    }
    int encode_yuv(const h264::YuvInput& in, int on_device, uint16_t frame_id) override {
        if (refuse_queued("encode_yuv()")) return -1;
        if (fe().scaled_) { set_last_error("planar input cannot be resampled"); return -1; }
        HostYuv h;
        if (h.load(in, on_device, fe().g.W, fe().g.H) < 0) return -1;
        fe().yuv_in = h.in;
        return encode(nullptr, 0, frame_id);
    }
    int64_t debug_buffer(const char* name, void* dst, int64_t cap) override {
        const std::string s(name);
        const size_t plane = s.size() == 5 ? std::string("yuv").find(s[4]) : std::string::npos;   // "src_y": 0
        DebugBuf b;
        if (plane < 3 && s.compare(0, 4, "src_") == 0) b = bytes_of(fe().prev[plane]);   // after finish_frame the source lives in prev
        else if (plane < 3 && s.compare(0, 4, "ref_") == 0) b = bytes_of(fe().ref[plane]);
        else if (s == "me") b = bytes_of(fe().me);
        else if (s == "tasks") b = bytes_of(fe().tasks);
        else b = codec_debug(enc_, s);
        if (b.second < 0) return -1;
        if (dst && cap >= b.second) memcpy(dst, b.first, (size_t)b.second);
        return b.second;
    }

    int64_t state_bytes() override { return (int64_t)h264::state_bytes(fe().g, fe().ltr_cfg.slots); }
    int export_state(void* dst, int on_device) override {
        if (on_device) return -1;
        h264::cpu_export_state(fe(), dst);
        return 0;
    }
    int import_state(const void* src, int on_device) override {
        if (on_device) return -1;
        if (!h264::cpu_import_state(fe(), src)) {
            set_last_error("encoder state does not match this encoder's geometry / codec");
            return -1;
        }
        after_import(enc_);
        return 0;
    }

   private:
    h264::CpuH264Encoder& fe() { return front(enc_); }
    Enc enc_;
};

class CpuJpegBackend : public EncoderBackend {
   public:
    explicit CpuJpegBackend(const jpeg::JpegConfig& c) : enc_(c) {}
    void request_keyframe() override { enc_.request_keyframe(); }
    int encode(const uint8_t* bgrx, int stride, uint16_t frame_id) override {
        if (refuse_queued("encode()")) return -1;
        packets_.clear();
        enc_.encode(bgrx, stride, frame_id, packets_);
        return (int)packets_.size();
    }
    int64_t debug_buffer(const char*, void*, int64_t) override { return -1; }

   private:
    jpeg::CpuJpegEncoder enc_;
};

}  // namespace

EncoderBackend* create_cpu_jpeg_backend(const jpeg::JpegConfig& c) { return new CpuJpegBackend(c); }

EncoderBackend* create_cpu_backend(const h264::EncoderConfig& c) {
    if (c.codec == 1) return new CpuBackend<hevc::CpuHevcEncoder>(c);
    if (c.codec == 2) return new CpuBackend<av1::CpuAv1Encoder>(c, c.tile_cols_log2, c.tile_rows_log2);
    return new CpuBackend<h264::CpuH264Encoder>(c);
}

h264::EncoderConfig to_config(const sk_h264_config* c) {
    h264::EncoderConfig e;
    e.width = c->width;
    e.height = c->height;
    e.stripe_height = c->stripe_height > 0 ? c->stripe_height : 64;
    e.fullframe = c->fullframe;
    e.full_range = c->full_range;
    e.qp = c->qp;
    e.paint_qp = c->paint_qp;
    e.use_paint_over = c->use_paint_over;
    e.paint_over_trigger = c->paint_over_trigger;
    e.paint_over_burst = c->paint_over_burst;
    e.streaming_mode = c->streaming_mode;
    e.damage_threshold = c->damage_threshold;
    e.damage_duration = c->damage_duration;
    e.me_range = c->me_range > 0 ? c->me_range : 64;
    e.me_iters = c->me_iters > 0 ? c->me_iters : 24;
    e.scenecut = c->scenecut;
    e.fps = c->fps > 0 ? c->fps : 60.f;
    e.deblock = c->deblock < 0 ? 0 : (c->deblock == 1 ? 1 : 2);   // default automatic (h264_encoder.h slice_deblock)
    e.me_full = c->me_full >= 0 ? 1 : 0;
    e.shared_copy = c->shared_copy > 0 ? 1 : 0;
    e.src_width = c->src_width > 0 ? c->src_width : 0;
    e.src_height = c->src_height > 0 ? c->src_height : 0;
    e.num_refs = c->num_refs > 1 ? 2 : 1;
    e.codec = (c->codec == 1 || c->codec == 2) ? c->codec : 0;
    e.tile_cols_log2 = c->tile_cols_log2;
    e.tile_rows_log2 = c->tile_rows_log2;
    e.rc_mode = c->rc_mode >= 0 && c->rc_mode <= 2 ? c->rc_mode : 0;
    e.bitrate_kbps = c->bitrate_kbps > 0 ? c->bitrate_kbps : 0;
    if (e.rc_mode == h264::RC_CBR && e.bitrate_kbps <= 0) e.rc_mode = h264::RC_CRF;
    e.aq_strength = c->aq_strength > 0 ? (c->aq_strength > 64 ? 64 : c->aq_strength) : 0;
    e.subpel = c->subpel >= 0 ? 1 : 0;
    e.intra4x4 = c->intra4x4 > 0 ? 1 : 0;
    e.ltr_slots = c->ltr_slots > 0 ? c->ltr_slots : 0;
    h264::set_av1_tools(e, c->av1_intra_inter, c->av1_chroma_palette, c->av1_cfl, c->av1_palette_cluster);
    if (e.codec >= 1) {   // HEVC / AV1: full-frame pictures, slices of whole CTB rows, one reference
        e.aq_strength = 0;   // no cu_qp_delta in this HEVC profile setup
        e.fullframe = 1;
        e.num_refs = 1;
        e.deblock = 0;
    }
    return e;
}

}  // namespace sk

using namespace sk;

extern "C" {

const char* sk_version(void) { return "selkies-mi355x native 0.1 (gfx950)"; }

int sk_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int sk_hip_pci_bus_id(int device, char* buf, int len) {
    if (hipDeviceGetPCIBusId(buf, len, device) != hipSuccess) return -1;
    return 0;
}

const char* sk_last_error(void) { return g_last_error.c_str(); }

void* sk_host_alloc(int64_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        p = aligned_alloc(4096, ((size_t)bytes + 4095) & ~(size_t)4095);  // no GPU: plain memory
    }
    return p;
}

void sk_host_free(void* p) {
    if (!p) return;
    if (hipHostFree(p) != hipSuccess) free(p);
}

void* sk_h264_create(const sk_h264_config* c) {
    if (!c || c->width < 16 || c->height < 16 || (c->width & 1) || (c->height & 1)) {
        set_last_error("invalid encoder geometry (width/height must be even and >= 16)");
        return nullptr;
    }
    if (c->stripe_height > 0 && (c->stripe_height % 16) != 0) {
        set_last_error("stripe_height must be a multiple of 16");
        return nullptr;
    }
    // the HIP intra/deblock wavefronts run one wave per MB row of a stripe (+1 producer wave)
    // in one workgroup: at most 15 rows (1024 threads). Same limit on the CPU reference so
    // both backends accept the same configurations.
    if (c->stripe_height > 240) {
        set_last_error("stripe_height must be <= 240 (15 macroblock rows per stripe)");
        return nullptr;
    }
    if (c->qp < 0 || c->qp > 51 || c->paint_qp < 0 || c->paint_qp > 51) {
        set_last_error("qp out of range");
        return nullptr;
    }
    h264::EncoderConfig e = to_config(c);
    if (const char* err = h264::ltr_config_error(e)) {   // long-term reference cache (codec/ltr.h)
        set_last_error(err);
        return nullptr;
    }
    try {
        if (c->backend == 1) return create_hip_backend(e, c->device);
        return create_cpu_backend(e);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return nullptr;
    }
}

void* sk_jpeg_create(const sk_jpeg_config* c) {
    if (!c || c->width < 16 || c->height < 16 || (c->stripe_height % 16) != 0 || c->stripe_height <= 0) {
        set_last_error("invalid JPEG encoder geometry");
        return nullptr;
    }
    jpeg::JpegConfig j;
    j.width = c->width;
    j.height = c->height;
    j.stripe_height = c->stripe_height;
    j.quality = c->quality;
    j.paint_quality = c->paint_quality;
    j.use_paint_over = c->use_paint_over;
    j.paint_over_trigger = c->paint_over_trigger;
    try {
        if (c->backend == 1) return create_hip_jpeg_backend(j, c->device);
        return create_cpu_jpeg_backend(j);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return nullptr;
    }
}

void sk_h264_destroy(void* enc) { delete static_cast<EncoderBackend*>(enc); }
void sk_h264_request_keyframe(void* enc) { static_cast<EncoderBackend*>(enc)->request_keyframe(); }
void sk_h264_set_qp(void* enc, int qp, int paint_qp) { static_cast<EncoderBackend*>(enc)->set_qp(qp, paint_qp); }
void sk_h264_set_rate(void* enc, int mode, int kbps) { static_cast<EncoderBackend*>(enc)->set_rate(mode, kbps); }
int sk_h264_rc_stats(void* enc, int32_t* out, int n) {
    return (int)static_cast<EncoderBackend*>(enc)->rc_stats(out, n);
}
int sk_h264_set_overlay_image(void* enc, int slot, const uint8_t* bgra, int w, int h) {
    return static_cast<EncoderBackend*>(enc)->set_overlay_image(slot, bgra, w, h);
}
int sk_h264_set_overlay_pos(void* enc, int slot, int on, int x, int y, int tdx, int tdy) {
    return static_cast<EncoderBackend*>(enc)->set_overlay_pos(slot, on, x, y, tdx, tdy);
}

int sk_h264_encode(void* enc, const uint8_t* bgrx, int32_t stride, int32_t frame_id) {
    try {
        return static_cast<EncoderBackend*>(enc)->encode(bgrx, stride, (uint16_t)frame_id);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_submit(void* enc, const uint8_t* bgrx, int32_t stride, int32_t frame_id) {
    try {
        return static_cast<EncoderBackend*>(enc)->submit(bgrx, stride, (uint16_t)frame_id);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_wait_stream(void* enc, void* stream) {
    try {
        return static_cast<EncoderBackend*>(enc)->wait_stream(stream);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_upload(void* enc, const uint8_t* bgrx, int32_t stride, int32_t frame_id) {
    try {
        return static_cast<EncoderBackend*>(enc)->upload(bgrx, stride, (uint16_t)frame_id);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_set_upload_rows(void* enc, const int32_t* rows, int32_t n) {
    static_cast<EncoderBackend*>(enc)->set_upload_rows(rows, n);
    return 0;
}

int sk_upload_ranges(const int32_t* pairs, int32_t n, int32_t rows, int32_t* out, int32_t cap) {
    std::vector<int> v(pairs && n > 0 ? pairs : nullptr, pairs && n > 0 ? pairs + 2 * n : nullptr);
    const auto r = upload_ranges({&v}, rows);
    for (int i = 0; i < (int)r.size() && i < cap; i++) {
        out[2 * i] = r[i].first;
        out[2 * i + 1] = r[i].second;
    }
    return (int)r.size();
}

int sk_h264_encode_yuv(void* enc, int32_t fmt, const uint8_t* y, int32_t ys, const uint8_t* u, int32_t us,
                       const uint8_t* v, int32_t vs, int32_t on_device, int32_t frame_id) {
    if (fmt != h264::YUV_I420 && fmt != h264::YUV_NV12) {
        set_last_error("planar format must be 1 (I420) or 2 (NV12)");
        return -1;
    }
    h264::YuvInput in;
    in.fmt = fmt;
    in.p[0] = y; in.p[1] = u; in.p[2] = fmt == h264::YUV_NV12 ? u : v;
    in.stride[0] = ys; in.stride[1] = us; in.stride[2] = fmt == h264::YUV_NV12 ? us : vs;
    try {
        return static_cast<EncoderBackend*>(enc)->encode_yuv(in, on_device, (uint16_t)frame_id);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_launch(void* enc) {
    try {
        return static_cast<EncoderBackend*>(enc)->launch();
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_finish(void* enc) {
    try {
        return static_cast<EncoderBackend*>(enc)->finish();
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int64_t sk_h264_state_bytes(void* enc) { return static_cast<EncoderBackend*>(enc)->state_bytes(); }

int sk_h264_export_state(void* enc, void* dst, int32_t on_device) {
    try {
        return static_cast<EncoderBackend*>(enc)->export_state(dst, on_device);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_import_state(void* enc, const void* src, int32_t on_device) {
    try {
        return static_cast<EncoderBackend*>(enc)->import_state(src, on_device);
    } catch (const std::exception& ex) {
        set_last_error(ex.what());
        return -1;
    }
}

int sk_h264_get_packet(void* enc, int32_t i, sk_packet* out) {
    auto* e = static_cast<EncoderBackend*>(enc);
    if (i < 0 || i >= (int)e->packets_.size()) return -1;
    const h264::EncodedPacket& p = e->packets_[i];
    out->data = p.data.data();
    out->size = (int32_t)p.data.size();
    out->y = p.y;
    out->w = p.w;
    out->h = p.h;
    out->key = p.key;
    return 0;
}

int64_t sk_h264_debug_buffer(void* enc, const char* name, void* dst, int64_t cap) {
    return static_cast<EncoderBackend*>(enc)->debug_buffer(name, dst, cap);
}

int sk_h264_stage_times(void* enc, float* dst, int32_t n) {
    return static_cast<EncoderBackend*>(enc)->stage_times(dst, n);
}

}  // extern "C"
