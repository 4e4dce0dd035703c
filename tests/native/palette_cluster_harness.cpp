// Host-only check of the shared functions of av1_palette_cluster (codec/av1_core.h): palette_cluster
// over random and extreme luma histograms of 8x8 and 16x16 blocks, palette_nearest and palette_has_ramp,
// against the invariants their comments state. Built with -fsanitize=address,undefined by
// tests/test_av1_palette_cluster.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Icsrc -Icsrc/codec \
//       tests/native/palette_cluster_harness.cpp -o /tmp/pch && /tmp/pch [blocks] [seed]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include "av1_core.h"

using namespace sk::av1;

static int fails = 0;
#define CHECK(cond, ...)                \
    do {                                \
        if (!(cond)) {                  \
            fails++;                    \
            printf("FAIL %s: ", #cond); \
            printf(__VA_ARGS__);        \
            printf("\n");               \
        }                               \
    } while (0)

static int clustered = 0;

static void check_block(const uint8_t* px, int nn, int tol, const char* what) {
    uint16_t hist[256];
    memset(hist, 0, sizeof(hist));
    for (int i = 0; i < nn; i++) hist[px[i]]++;
    int m = 0;
    for (int v = 0; v < 256; v++) m += hist[v] != 0;
    uint8_t col[kPalMax];
    memset(col, 0xaa, sizeof(col));
    const int k = palette_cluster(hist, tol, col);
    CHECK(k == 0 || (k >= 2 && k <= kPalMax), "%s: k %d", what, k);
    if (m <= kPalMax || m > kPalClusterValues || tol < 1) CHECK(k == 0, "%s: m %d tol %d gave k %d", what, m, tol, k);
    if (!k) return;
    clustered++;
    uint64_t C = 0;
    for (int q = 0; q < kPalMax; q++) {
        if (q > 0 && q < k) CHECK(col[q] > col[q - 1], "%s: colours %d %d at %d", what, col[q - 1], col[q], q);
        if (q >= k) CHECK(col[q] == 0, "%s: colour %d past the count", what, q);
        C |= (uint64_t)col[q] << (8 * q);
    }
    int lo = 255, hi = 0;
    for (int v = 0; v < 256; v++)
        if (hist[v]) {
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
    CHECK(col[0] >= lo && col[k - 1] <= hi, "%s: colours outside the values' range", what);
    for (int i = 0; i < nn; i++) {
        const int x = palette_nearest(C, k, px[i]);
        CHECK(x >= 0 && x < k, "%s: index %d of %d", what, x, k);
        for (int q = 0; q < k; q++) {
            const int d = abs((int)col[q] - px[i]), dx = abs((int)col[x] - px[i]);
            CHECK(dx < d || (dx == d && x <= q), "%s: value %d on colour %d, colour %d is nearer or lower", what, px[i], x, q);
        }
        CHECK(palette_map_index<true>(col, k, px[i]) == x, "%s: map index", what);
    }
}

int main(int argc, char** argv) {
    const int blocks = argc > 1 ? atoi(argv[1]) : 4000;
    std::mt19937 rng(argc > 2 ? (unsigned)atoi(argv[2]) : 1u);
    uint8_t px[256];
    for (int b = 0; b < blocks; b++) {
        const int nn = b & 1 ? 64 : 256, m = 2 + (int)(rng() % 40), tol = (int)(rng() % 36);
        uint8_t vals[48];
        const int mode = (int)(rng() % 4);
        for (int i = 0; i < m; i++)   // spread values, tight groups, a ramp, the extremes
            vals[i] = (uint8_t)(mode == 0 ? rng() % 256 : mode == 1 ? (rng() % 3) * 100 + rng() % 6 : mode == 2 ? 40 + i : (rng() & 1) * 255 - (int)(rng() % 9) * ((int)(rng() & 1) * 2 - 1));
        for (int i = 0; i < nn; i++) px[i] = vals[i < m ? i : (rng() % 4 ? 0 : rng() % m)];
        check_block(px, nn, tol, "random");
    }
    for (int i = 0; i < 256; i++) px[i] = (uint8_t)i;   // every value once: more than kPalClusterValues
    check_block(px, 256, 16, "all values");
    for (int i = 0; i < 256; i++) px[i] = (uint8_t)(i < 128 ? 0 : 255 - (i & 7) * 3);   // the largest sums and counts
    check_block(px, 256, 1, "extremes");
    for (int i = 0; i < 256; i++) px[i] = (uint8_t)(i < 247 ? 255 : 10 * (i - 247));    // one heavy value, nine single ones
    check_block(px, 256, 4, "heavy");
    CHECK(palette_merge_cost(128 * 255, 128, 0, 128) == 128 * 128 * 255 * 255 / 256, "merge cost at its bound");
    CHECK(!palette_has_ramp(0x7f) && palette_has_ramp(0xff) && palette_has_ramp(0xffull << 23) && !palette_has_ramp(0x7f7f7f7f7f7f7f7full),
          "ramp runs");
    CHECK(clustered > blocks / 20, "only %d of %d blocks clustered: the harness does not reach the code", clustered, blocks);
    printf("%d blocks, %d clustered, %d failures\n", blocks + 3, clustered, fails);
    if (!fails) printf("sanitized run ok\n");
    return fails ? 1 : 0;
}
