// Geometry of an AV1 frame and its uniform tile split. On its own so that the shared
// configuration checks (h264_encoder.h) can ask for a session's tile rows without the codec.
#pragma once
#include "sk_common.h"

namespace sk {
namespace av1 {

// ---------------------------------------------------------------------------------
// Geometry of one frame and its tiles (uniform tile spacing, §5.9.15).
struct Av1Geo {
    int W = 0, H = 0;            // frame size
    int mi_cols = 0, mi_rows = 0;
    int sb_cols = 0, sb_rows = 0;
    int tile_cols_log2 = 0, tile_rows_log2 = 0;
    int tile_cols = 0, tile_rows = 0;
    int tile_w_sb = 0, tile_h_sb = 0;
    int min_log2_tile_cols = 0, max_log2_tile_cols = 0, max_log2_tile_rows = 0, min_log2_tiles = 0;
    int c8 = 0, r8 = 0;          // 8x8 cell grid (mi_cols / 2, mi_rows / 2)
};

SK_HD int tile_log2(int blk, int target) {
    int k = 0;
    while ((blk << k) < target) k++;
    return k;
}

// Automatic tile split (log2 columns / rows) of a frame of sbc x sbr superblocks: up to
// 8 x 8 tiles; from 48 superblock columns (3072 px: 4K, 8K) 16 columns x 4 rows, the
// level-5.1 limits (MaxTileCols 16, MaxTiles 64). A key frame's tile is one workgroup of
// 16 waves stepping along anti-diagonals of 16x16 units (k_av1_intra_rec): 4K tiles of
// 16 x 36 units never hold more units on a diagonal than there are waves, where 8 x 7 tiles
// of 32 x 20 units needed a second round on 19 of their 51 steps.
SK_HD void auto_tiles(int sbc, int sbr, int* cols_log2, int* rows_log2) {
    if (sbc >= 48) {
        *cols_log2 = 4;
        *rows_log2 = tile_log2(1, sk_min(4, sbr));
        return;
    }
    *cols_log2 = tile_log2(1, sk_min(8, sbc));
    *rows_log2 = tile_log2(1, sk_min(8, sbr));
}

// want_cols_log2 / want_rows_log2: requested split, clamped to the legal range.
SK_HD void geo_init(Av1Geo& g, int W, int H, int want_cols_log2, int want_rows_log2) {
    g.W = W;
    g.H = H;
    g.mi_cols = 2 * ((W + 7) >> 3);
    g.mi_rows = 2 * ((H + 7) >> 3);
    g.c8 = g.mi_cols >> 1;
    g.r8 = g.mi_rows >> 1;
    g.sb_cols = (g.mi_cols + 15) >> 4;
    g.sb_rows = (g.mi_rows + 15) >> 4;
    const int max_tile_w_sb = 4096 >> 6, max_tile_area_sb = (4096 * 2304) >> 12;
    g.min_log2_tile_cols = tile_log2(max_tile_w_sb, g.sb_cols);
    g.max_log2_tile_cols = tile_log2(1, sk_min(g.sb_cols, 64));
    g.max_log2_tile_rows = tile_log2(1, sk_min(g.sb_rows, 64));
    g.min_log2_tiles = sk_max(g.min_log2_tile_cols, tile_log2(max_tile_area_sb, g.sb_rows * g.sb_cols));
    g.tile_cols_log2 = sk_clip(want_cols_log2, g.min_log2_tile_cols, g.max_log2_tile_cols);
    g.tile_w_sb = (g.sb_cols + (1 << g.tile_cols_log2) - 1) >> g.tile_cols_log2;
    g.tile_cols = (g.sb_cols + g.tile_w_sb - 1) / g.tile_w_sb;
    const int min_log2_rows = sk_max(g.min_log2_tiles - g.tile_cols_log2, 0);
    g.tile_rows_log2 = sk_clip(want_rows_log2, min_log2_rows, g.max_log2_tile_rows);
    g.tile_h_sb = (g.sb_rows + (1 << g.tile_rows_log2) - 1) >> g.tile_rows_log2;
    g.tile_rows = (g.sb_rows + g.tile_h_sb - 1) / g.tile_h_sb;
}

// The split a session codes with (requested log2 counts, -1 = automatic) and the rows of
// 16x16 units in one of its tile rows: the long-term cache's decision unit (ltr.h).
SK_HD void session_geo(Av1Geo& g, int W, int H, int want_cols_log2, int want_rows_log2) {
    int auto_c, auto_r;
    auto_tiles((W + 63) / 64, (H + 63) / 64, &auto_c, &auto_r);
    geo_init(g, W, H, want_cols_log2 < 0 ? auto_c : want_cols_log2, want_rows_log2 < 0 ? auto_r : want_rows_log2);
}
SK_HD int tile_row_units(int W, int H, int want_cols_log2, int want_rows_log2) {
    Av1Geo g;
    session_geo(g, W, H, want_cols_log2, want_rows_log2);
    return g.tile_h_sb * 4;
}

}  // namespace av1
}  // namespace sk
