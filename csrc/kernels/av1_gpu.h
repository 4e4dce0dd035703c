// Device buffers and launch interface of the HIP AV1 back end. It runs after the
// H.264 front end (k_convert_damage, k_plan, k_me, k_decide)
// on the same FrameArgs and before k_commit (reference / motion-field update).
#pragma once
#include <hip/hip_runtime.h>
#include "h264_gpu.h"
#include "../codec/av1_core.h"
#include "../codec/av1_lf.h"
#include "../codec/av1_cdef.h"

namespace sk {
namespace av1 {
namespace gpu {

constexpr int kLevPerUnit = 384;
constexpr int kTokCap = 4096;        // tokens per 16x16 unit slot (worst case tok_bound::kUnit = 2827, below)
constexpr int kTileChunkCap = 1 << 20;

// The most tokens code_unit (av1_core.h; k_av1_tokens) can put into one unit's slot, over every
// level quantize can return. A unit with residual is one 16x16 block (luma 16x16 + two 8x8 chroma
// transform blocks) or four 8x8 blocks (luma 8x8 + two 4x4 each); larger blocks carry no residual.
// Literal bits are packed 24 to a token; a symbol first flushes the pending bits as a token of their own.
namespace tok_bound {
constexpr int kLevelCap = 4095;      // quantize: |level| <= 4095
constexpr int golomb_bits(int a) {   // code_coeffs: Golomb code of a - 14 (a > 14)
    int len = 0;
    while (((a - 14) >> (len + 1)) != 0) len++;
    return 2 * len + 1;
}
constexpr int kCoefs = 256 + 2 * 64;                        // levels of a unit
constexpr int kCoefBits = 1 + golomb_bits(kLevelCap);       // sign + Golomb remainder: 24
constexpr int kTxbs = 4 * 3;                                // transform blocks of four 8x8 blocks
constexpr int kTxbHead = 1 + 1 + 1 + 1 + 1 + 1 + 1;         // txb_skip, tx set, eob_pt, eob_extra, its literal bits, dc_sign, the
                                                            // bits left over after the block's full 24-bit literals
constexpr int kPaletteBits = 16 + 8 + 2 + 7 * 8;            // cache flags, first colour, extra bits, seven deltas
constexpr int kPaletteUvBits = kPaletteBits                 // U: cache flags, first colour, extra bits, seven deltas
                               + 1 + 8 * 8;                 // V: the delta flag, eight raw colours (delta coding only where shorter)
constexpr int kKeyHead = 1 + 1 + 1 + 1 + 1                  // skip, y mode, angle delta, uv mode, angle delta
                         + 1 + 1 + 1                        // cfl_alpha_signs, cfl_alpha_u, cfl_alpha_v (av1_cfl)
                         + 1 + 1                            // palette_y_mode, palette_y_size
                         + (kPaletteBits + 23) / 24 + 1     // the colours' literals (the first may join pending bits)
                         + 1                                // palette_uv_mode
                         + 1                                // palette_uv_size (av1_chroma_palette)
                         + (kPaletteUvBits + 23) / 24 + 1;  // the chroma colours' literals
constexpr int kMvComp = 1 + 1 + 10 + 1;                     // sign, class, class bits, fraction
constexpr int kInterHead = 1 + 1 + 3                        // skip, is_inter, three single_ref symbols
                           + 1 + 2                          // new_mv, two drl symbols (zero_mv / ref_mv: without a vector)
                           + 1 + 2 * kMvComp;               // mv_joint, both components
constexpr int kPaletteMap = 64 - 1 + 1 + 1                  // an 8x8 block: the other 63 indices, the first as literal bits, its flush
                            + 16 - 1 + 1 + 1;               // its 4x4 chroma map likewise (a 16x16 block's two maps, 257 + 65
                                                            // tokens, stay below four 8x8 blocks')
constexpr int kPartition = 2 + 1 + 4;                       // the 64 and 32 nodes the unit opens, its own, four 8x8 nodes
constexpr int kBlocks = 4;
constexpr int kIntraHead = kKeyHead + 1;                    // an intra block of an inter frame: is_inter too (av1_intra_inter)
constexpr int kHead = kIntraHead + kPaletteMap > kInterHead ? kIntraHead + kPaletteMap : kInterHead;
constexpr int kUnit = kPartition                            // partition symbols
                      + kBlocks * kHead                     // mode info (and index maps) of four blocks
                      + kTxbs * kTxbHead                    // per transform block
                      + kCoefs * (1 + 4)                    // coeff_base(_eob) + four coeff_br per level
                      + kCoefs * kCoefBits / 24;            // full literals of the sign / Golomb runs
static_assert(kCoefBits == 24 && 256 * kCoefBits <= 256 * 32, "a 16x16 block's sign / Golomb run fits the 256-word LDS bit buffer");
static_assert(kUnit == 2827, "tok_bound changed: update the comment on kTokCap");
static_assert(kUnit <= kTokCap, "a unit's tokens can overflow its slot (the tokens past it are dropped)");
}   // namespace tok_bound

struct Av1Args {
    h264::gpu::FrameArgs f;   // planes, geometry (mb = 16x16 unit), tasks, motion field
    Av1Geo geo;
    BlkInfo* blk;             // [r8][c8]
    uint8_t* pal;             // [r8][c8][8] palette colours of each cell's block (key frames)
    int palette;              // palette coding of key frames enabled (av1_encoder.h palette_enabled)
    int tools;                // the session's tools word (av1_core.h Tools; av1_encoder.h session_tools)
    int* pal_rate;            // [r8][c8] palette_rate2 of the luma palette candidate of the block at that origin cell
                              // (k_av1_intra_modes / k_av1_cand_modes; a clustered candidate's word carries
                              // kPalClusterMark). The candidates' counts: av1_core.h cand_pack
    uint8_t* pal_uv;          // [r8][c8][16] chroma palette of each cell's block: U at 0, V at 8 (av1_core.h FrameView)
    int* pal_rate_uv;         // [r8][c8] rate (half bits) of the chroma palette candidate of the block at that origin cell
    // kToolIntraInter only:
    long long* jinter;        // [r8][c8] J of the inter coding of the block at that origin cell (k_av1_inter)
    int* cand;                // [r8][c8] the candidate word of the block at that origin cell (cand_pack; k_av1_cand_modes)
    int* tile_cand;           // [tiles] candidates of the tile (k_av1_setup clears, k_av1_inter counts)
    int16_t* lev;             // [units][kLevPerUnit]
    uint8_t* lctx[3];         // level contexts per plane (4x4 units), strides lctx_w
    int lctx_w[3];
    uint32_t* tok;            // [units][kTokCap]
    int* tok_n;               // [units]
    uint32_t* tokc;           // [tiles][tile_tok_cap]: each tile's tokens in coding order
    uint32_t* pw;             // [tiles][tile_tok_cap]: interval word of each symbol token (k_av1_cdf)
    int tile_tok_cap;
    int* tok_off;             // [units] offset of the unit's tokens in its tile's stream
    int* tile_ntok;           // [tiles]
    int* frame;               // device: [0] key, [1] qidx, [2] loop filter level
    int* frame_host;          // host-mapped copy of frame[0..2]; with the long-term cache (ltr.h) the reference buffers
                              // of the header: [3] refresh_frame_flags, [4] LAST's buffer, [5] LAST2's buffer
    h264::gpu::Planes cdef_in;   // the deblocked picture CDEF reads (k_av1_cdef writes f.rec)
    const uint8_t* qidx_of_qp;   // [52]
    int tile_cap;             // byte capacity per tile
    // block-parallel coder (k_av1_ec_*): per block 128 candidate (exit rng, shift count)
    // maps and {first token, end, entry rng, shift prefix}; per tile the big integer low
    // as 64-bit digit sums (ecv), its carried 32-bit digits (ecf) and its total shift
    uint2* ecmap;             // [ec_max_blocks][128]
    int4* ecblk;              // [ec_max_blocks]
    int ec_max_blocks;
    unsigned long long* ecv;  // [tiles][ec_vcap]
    uint32_t* ecf;            // [tiles][ec_vcap]
    int ec_vcap;
    int* tile_bits;           // [tiles] total shift D (-1: over capacity)
    int* tile_size;           // device [tiles] bytes
    uint8_t* out_host;        // host-mapped tile bytes, concatenated [out_cap]
    int out_cap;
    int* out_size_host;       // host-mapped [tiles] bytes (-1: did not fit out_cap)
};

// redo: the K10 re-code flag (CBR sessions): the coding kernels run a second time,
// gated on it, after k_rc_guard_sizes checked the frame against its cap; nullptr: one pass.
void launch_backend(const Av1Args& a, hipStream_t s, int* redo = nullptr);
// Sizes of the coder's block maps and big-integer digits for tiles of tile_bytes.
void ec_buffers(int tiles, int tile_bytes, int* max_blocks, int* vcap);

}  // namespace gpu
}  // namespace av1
}  // namespace sk
