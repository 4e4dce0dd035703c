// Emulation prevention (7.4.1), tile-parallel form: the carry of a tile.
//
// Whether a 0x03 goes before RBSP byte i depends on the zero run right before i,
// so a tile of the RBSP that is processed on its own needs one number from the
// bytes before it: the index of the last non-zero byte before its first byte t0
// (-1: none; the NAL header byte before the RBSP is non-zero). The tile finds it
// by looking backwards from t0 - 1. SK_HD so the GPU kernels and a serial host
// form (one lane) share one definition.
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

}  // namespace h264
}  // namespace sk
