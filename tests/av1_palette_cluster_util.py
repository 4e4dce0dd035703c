"""Shared helpers of the AV1 clustered-palette tests (test_av1_palette_cluster.py,
test_av1_palette_cluster_gpu.py): two anti-aliased contents, a designed picture, accessors of the
luma palette cells and a numpy model of the clustering rule written from its description
(docs/design.md, "AV1 clustered luma palettes"), not from the C++.

aa_field: the glyph field of av1_chroma_palette_util rendered at a quarter-pixel offset: enlarged 4x,
moved by (1, 2) samples and averaged over 4x4 boxes. A pixel mixes up to four neighbours with the
weights (3/4, 1/4) x (1/2, 1/2): 9 luma values in a 16x16 unit.

soft_field: dark grey glyphs on a light grey background, enlarged 8x, moved by (3, 5), the mean of
three copies displaced by (0, 0), (2, 2) and (-2, 1), averaged over 8x8 boxes: 14 values in a unit.

designed picture: 128x128 I420 planes for encode_yuv, flat chroma. Each designed 16x16 unit holds one
set of luma values in a pseudo-random arrangement (UNITS); every other unit is flat. 128 rows: the
units of row 4 start a superblock row and see no palette cache from above."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from tests import av1_intra_inter_util as U
from tests.av1_chroma_palette_util import glyph_field

BLK_MODE, BLK_FLAGS, BLK_PAL_N = 1, 3, 10     # bytes of a BlkInfo cell (csrc/codec/av1_core.h)
PAL_MAX, CLUSTER_VALUES, RAMP_GAP = 8, 32, 2
SOFT_BG, SOFT_INK = (236, 236, 232, 255), (40, 30, 30, 255)


def _box(f: np.ndarray, k: int, roll, offsets=((0, 0),)) -> np.ndarray:
    h, w = f.shape[:2]
    up = np.roll(f[:, :, :3].astype(np.float64).repeat(k, 0).repeat(k, 1), roll, axis=(0, 1))
    up = sum(np.roll(up, o, axis=(0, 1)) for o in offsets) / len(offsets)
    out = np.empty((h, w, 4), np.uint8)
    out[:, :, :3] = np.floor(up.reshape(h, k, w, k, 3).mean(axis=(1, 3)) + 0.5).astype(np.uint8)
    out[:, :, 3] = 255
    return out


def aa_field(w: int, h: int, shift: int = 0) -> np.ndarray:
    """BGRx picture: coloured glyphs with 4x box anti-aliasing."""
    return _box(glyph_field(w, h, shift), 4, (1, 2))


def soft_field(w: int, h: int, shift: int = 0) -> np.ndarray:
    """BGRx picture: grey glyphs with soft 8x anti-aliasing."""
    return _box(glyph_field(w, h, shift, bg=SOFT_BG, ink=SOFT_INK), 8, (3, 5), ((0, 0), (2, 2), (-2, 1)))


CONTENTS = {"aa": aa_field, "soft": soft_field}


def shifted_frames(make, w: int, h: int) -> list:
    """A key frame and two frames whose odd glyph rows have moved."""
    return [make(w, h, s) for s in (0, 3, 6)]


def window_frames(w: int, h: int, base: np.ndarray | None = None) -> list:
    """The window sequence of av1_intra_inter_util with the window filled by aa_field, its odd glyph
    rows moving from the window frame on."""
    seq = U.frames(w, h, base)
    x0, y0, ww, wh = U.window_rect(w, h)
    for k, f in enumerate(seq[U.WINDOW_FRAME:]):
        f[y0:y0 + wh, x0:x0 + ww] = aa_field(ww, wh, 3 * k)
    return seq


# ---------------------------------------------------------------------------------- designed picture
DESIGN_W = DESIGN_H = 128
FLAT = 128
_TWO = [60, 61, 62, 63, 200, 201, 202, 203, 204]               # nine values in two tight groups
_THREE = [30, 31, 33, 120, 121, 122, 123, 230, 232, 233]       # ten values in three groups
_EIGHT = [10, 40, 75, 110, 140, 170, 215, 250]                 # exactly eight: the exact palette
_SPREAD = list(range(20, 140, 10))                             # twelve values ten apart: more than eight intervals
# unit (row, col) -> (name, values).  two*, three*: clustered, also in row 0, column 0 and row 4;
# n1..n4: neighbours with the colours of `two` or `three`, cache hits from the left (n2), from above
# (n3) and from both (n4); below: like the unit above it across the superblock row boundary.
UNITS = {
    (0, 0): ("two_corner", _TWO), (0, 3): ("three_row0", _THREE), (2, 0): ("two_col0", _TWO),
    (1, 2): ("two", _TWO), (1, 4): ("three", _THREE), (1, 6): ("spread", _SPREAD),
    (2, 2): ("eight", _EIGHT), (2, 4): ("gradient", list(range(256))), (2, 6): ("flat", [90]),
    (3, 1): ("above", _THREE), (4, 1): ("below", _THREE), (4, 4): ("two_row4", _TWO),
    (5, 5): ("n1", _TWO), (5, 6): ("n2", _TWO), (6, 5): ("n3", _TWO), (6, 6): ("n4", _TWO + [205, 206]),
}
CLUSTERED = [u for u, (name, _) in UNITS.items() if name not in ("eight", "gradient", "flat")]


def designed_picture():
    """(Y, U, V) planes of the designed picture."""
    rng = np.random.default_rng(23)
    y = np.full((DESIGN_H, DESIGN_W), FLAT, np.uint8)
    u = np.full((DESIGN_H // 2, DESIGN_W // 2), 128, np.uint8)
    v = np.full((DESIGN_H // 2, DESIGN_W // 2), 128, np.uint8)
    for (r, c), (_, vals) in UNITS.items():
        k = len(vals)
        idx = np.concatenate([np.arange(k), rng.integers(0, k, 256 - k)])   # every value occurs
        rng.shuffle(idx)
        y[16 * r:16 * r + 16, 16 * c:16 * c + 16] = np.array(vals, np.uint8)[idx].reshape(16, 16)
    return y, u, v


# ------------------------------------------------------------------------------------------ the model
def ac_q(qidx: int) -> int:
    """Ac_Qlookup[0][qidx] of the AV1 specification, from the encoder's table header."""
    src = (Path(__file__).resolve().parents[1] / "csrc" / "codec" / "av1_tables.h").read_text()
    m = re.search(r"AV1_AC_QLOOKUP\[256\]\s*=\s*\{([^}]*)\}", src)
    return [int(x) for x in m.group(1).replace("\n", " ").split(",") if x.strip()][qidx]


def _mean(s: int, n: int) -> int:
    return (2 * s + n) // (2 * n)      # the rounded mean, halves up


def model_colours(block: np.ndarray, qidx: int):
    """The colours the documented rule gives the luma block, ascending, or None where the rule
    rejects it."""
    vals, cnt = np.unique(block.astype(np.int64), return_counts=True)
    tol = ac_q(qidx) // 12
    if not PAL_MAX < len(vals) <= CLUSTER_VALUES or tol < 1:
        return None
    run = 1                            # a ramp: more than eight values in a row, each at most 2 above the last
    for a, b in zip(vals, vals[1:]):
        run = run + 1 if b - a <= RAMP_GAP else 1
        if run > PAL_MAX:
            return None
    k, hi = 0, -1                      # the fewest intervals of width 2 tol, from the lowest value
    for x in vals:
        if x > hi:
            k, hi = k + 1, x + 2 * tol
    if k < 2:
        return None
    groups = [(int(x) * int(n), int(n)) for x, n in zip(vals, cnt)]      # (sum, count), ascending
    while len(groups) > min(k, PAL_MAX):
        cost = []
        for (s1, n1), (s2, n2) in zip(groups, groups[1:]):
            d = _mean(s2, n2) - _mean(s1, n1)
            cost.append(n1 * n2 * d * d // (n1 + n2))
        i = cost.index(min(cost))      # the first of equal costs
        groups[i:i + 2] = [(groups[i][0] + groups[i + 1][0], groups[i][1] + groups[i + 1][1])]
    return [_mean(s, n) for s, n in groups]


def nearest_map(block: np.ndarray, col) -> np.ndarray:
    """Index of the nearest colour of every sample, ties to the lower index."""
    d = np.abs(block.astype(np.int64)[..., None] - np.array(col, np.int64))
    return d.argmin(axis=-1)           # argmin returns the first minimum


def pal_y(enc, w: int, h: int) -> np.ndarray:
    """The luma palette cells, [rows][cols][8]; meaningful where PaletteSizeY is nonzero."""
    return enc.debug_buffer("pal").reshape((h + 7) // 8, (w + 7) // 8, 8)


def pal_n(cells: np.ndarray) -> np.ndarray:
    """PaletteSizeY of every cell: the low nibble of BlkInfo byte 10."""
    return cells[..., BLK_PAL_N] & 15


def distinct_values(src_y: np.ndarray, cells: np.ndarray, mask: np.ndarray | None = None) -> np.ndarray:
    """[rows][cols]: the number of distinct source luma values of the block each cell belongs to
    (16x16 unit, or the 8x8 cell itself where its block is 8x8); with a mask, of its cells only."""
    rows, cols = cells.shape[:2]
    out = np.zeros((rows, cols), int)
    for r in range(rows):
        for c in range(cols):
            if mask is not None and not mask[r, c]:
                continue
            if cells[r, c, 0] >= 2:
                blk = src_y[(r & ~1) * 8:(r & ~1) * 8 + 16, (c & ~1) * 8:(c & ~1) * 8 + 16]
            else:
                blk = src_y[r * 8:r * 8 + 8, c * 8:c * 8 + 8]
            out[r, c] = len(np.unique(blk))
    return out


def luma_psnr(src, rec) -> float:
    e = ((src[0].astype(np.float64) - rec[0].astype(np.float64)) ** 2).mean()
    return 99.0 if e == 0 else float(10 * np.log10(255.0 ** 2 / e))


def clustered(src_y: np.ndarray, cells: np.ndarray) -> np.ndarray:
    """[rows][cols] bool: cells of luma palette blocks whose source holds more than eight values."""
    n = pal_n(cells)
    return (n > 0) & (distinct_values(src_y, cells, n > 0) > PAL_MAX)
