// Emulation prevention (7.4.1): the carry of a tile looked up backwards (the tile-parallel
// form, kept for its host test) and the chunked forward form that k_slice_pack runs (below).
//
// Whether a 0x03 goes before RBSP byte i depends on the zero run right before i,
// so a tile of the RBSP that is processed on its own needs one number from the
// bytes before it: the index of the last non-zero byte before its first byte t0
// (-1: none; the NAL header byte before the RBSP is non-zero). The tile finds it
// by looking backwards from t0 - 1. No kernel calls ep_tile_carry any more (the
// tile-parallel kernels gave way to k_slice_pack); it is SK_HD with a serial host
// form (one lane), which tests/test_h264_ep_carry.py runs.
#pragma once
#include "sk_common.h"

namespace sk {
namespace h264 {

// RBSP words hold their bytes most significant first (AtomicBitWriter): byte i of
// the RBSP is bits 31 - 8 (i & 3) .. 24 - 8 (i & 3) of word i >> 2.
SK_HD uint8_t ep_rbsp_byte(uint32_t word, int q) { return (uint8_t)(word >> (24 - 8 * q)); }

// index (0..3) of the last non-zero byte of a non-zero RBSP word
SK_HD int ep_last_nz_in_word(uint32_t word) { return 3 - (__builtin_ctz(word) >> 3); }

// Last non-zero byte before t0 (a multiple of 4, so whole words lie before it), or -1.
// `nlanes` lanes call it together, lane = 0 .. nlanes - 1: every step each lane tests
// one word, the word (t0 / 4 - 1 - step * nlanes - lane), and ballot(pred) returns the
// mask of the lanes whose pred holds (bit k = lane k), the same value in every lane.
// The lowest set bit is the highest word, which every lane then reads for itself.
// The serial host form is nlanes = 1 with ballot(p) = p.
template <class Ballot>
SK_HD int ep_tile_carry(const uint32_t* rbsp, int t0, int lane, int nlanes, Ballot ballot) {
    for (int top = (t0 >> 2) - 1; top >= 0; top -= nlanes) {
        const int wi = top - lane;
        const uint64_t m = ballot(wi >= 0 && rbsp[wi] != 0u);
        if (m) {
            const int f = top - __builtin_ctzll(m);
            return 4 * f + ep_last_nz_in_word(rbsp[f]);
        }
    }
    return -1;
}

// ---------------------------------------------------------------------------
// Chunked form (k_slice_pack): one workgroup walks a NAL's RBSP forwards, chunk by
// chunk, so nothing looks backwards; what a chunk needs from the bytes before it is
// carried along.
//
// A 0x03 goes before RBSP byte i iff b_i <= 3 and the zero run right before i is even
// and >= 2 (7.4.1: after every two zeros that a byte <= 3 follows), which depends on
// the input bytes alone: on the index of the last non-zero byte before i.
struct EpState {
    int last_nz = -1;   // index of the last non-zero RBSP byte so far (-1: none; the NAL header byte is non-zero)
    int ins = 0;        // insertions so far
};

constexpr int kEpLaneBytes = 16;   // bytes one lane decides

// One lane's share of a chunk: the cnt <= kEpLaneBytes bytes by[0 .. cnt) at RBSP index
// i0 .. i0 + cnt. The lanes of a chunk call it together, in byte order. `carry` is
// EpState::last_nz before the chunk; before_me(v) takes this lane's own last non-zero
// index (-1: none) and returns the maximum over the lanes before it (-1: none): a
// workgroup scan on the GPU, a running maximum in the serial host form (ep_chunk).
// Returns the insertion mask (bit q: a 0x03 goes before by[q]); *last_nz is the lane's
// own last non-zero index.
template <class BeforeMe>
SK_HD uint32_t ep_lane(const uint8_t* by, int i0, int cnt, int carry, BeforeMe before_me, int* last_nz) {
    // constant trip counts: on the GPU the loops unroll and by[] stays in registers
    int own = -1;
#pragma unroll
    for (int q = 0; q < kEpLaneBytes; q++)
        if (q < cnt && by[q]) own = i0 + q;
    *last_nz = own;
    int prev = before_me(own);
    if (carry > prev) prev = carry;
    uint32_t mask = 0;
#pragma unroll
    for (int q = 0; q < kEpLaneBytes; q++) {
        if (q < cnt) {
            const int i = i0 + q, z = i - 1 - prev;
            if (by[q] <= 3 && z >= 2 && !(z & 1)) mask |= 1u << q;
            if (by[q]) prev = i;
        }
    }
    return mask;
}

// Serial form of a whole chunk: bytes[0 .. n) at RBSP index i0 .. i0 + n, the state as
// the bytes before it left it. Writes the RBSP indices before which a 0x03 goes to
// pos[] (room for n), updates the state, returns their number.
SK_HD int ep_chunk(const uint8_t* bytes, int i0, int n, EpState& st, int* pos) {
    int run = -1, count = 0;
    for (int k = 0; k < n; k += kEpLaneBytes) {
        const int cnt = n - k < kEpLaneBytes ? n - k : kEpLaneBytes;
        int own;
        const uint32_t mask = ep_lane(bytes + k, i0 + k, cnt, st.last_nz,
                                      [&](int v) {
                                          const int r = run;
                                          if (v > run) run = v;
                                          return r;
                                      },
                                      &own);
        for (int q = 0; q < cnt; q++)
            if (mask & (1u << q)) pos[count++] = i0 + k + q;
    }
    if (run > st.last_nz) st.last_nz = run;
    st.ins += count;
    return count;
}

}  // namespace h264
}  // namespace sk
