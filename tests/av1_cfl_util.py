"""Shared helpers of the AV1 chroma-from-luma tests (test_av1_cfl.py, test_av1_cfl_gpu.py): two
contents and accessors of the CfL fields of the cells. The encode loop is Checked of
av1_chroma_palette_util: every temporal unit goes through dav1d, all planes.

alpha picture: 128x128 I420 planes for encode_yuv. A designed 16x16 unit has a pseudo-random luma
texture, constant over each 2x2 quad so that the 8x8 chroma block sees it unfiltered, and chroma
built from the *source* luma by the prediction's own formula (av1_core.h cfl_px) with a designed
(alpha_u, alpha_v) and dc 128. Every other unit is flat (128, 128, 128). 128 rows: the units of row
4 start a superblock row; row 0 and column 0 have no neighbours.

hue texture: a BGRx picture of four regions (quadrants, cut at the picture's edges), each one
saturated colour whose brightness is modulated by a blocky pseudo-random texture: through the front
end's matrix the chroma of a region is proportional to its luma."""
from __future__ import annotations

import numpy as np

from tests import av1_intra_inter_util as U
from tests.av1_chroma_palette_util import glyph_field

BLK_UV_MODE, BLK_FLAGS, BLK_PAL_N = 2, 3, 10     # bytes of a BlkInfo cell (csrc/codec/av1_core.h)
UV_DC_PRED, UV_CFL_PRED = 0, 13
ALPHA_W = ALPHA_H = 128
# unit (row, col) -> (alpha_u, alpha_v, luma amplitude about 128). All eight joint signs, magnitudes 1
# (at amplitude 100: the chroma then swings +-12 and keeps a level under UV_DC_PRED) and 16 in each
# plane, units in row 0, column 0 and row 4.
DESIGN = {
    (0, 0): (4, 4, 40), (0, 2): (-4, 6, 40), (0, 5): (3, -5, 40),
    (2, 0): (6, -4, 40), (6, 0): (-6, -6, 40),
    (1, 2): (0, -8, 40), (1, 4): (0, 8, 40), (1, 6): (-8, 0, 40),
    (2, 3): (8, 0, 40), (2, 5): (-8, -8, 40), (3, 1): (-8, 8, 40),
    (3, 4): (16, -16, 40), (3, 6): (-16, 16, 40),
    (4, 1): (8, 8, 40), (4, 3): (1, -1, 100), (4, 5): (-1, 1, 100), (4, 7): (12, -2, 40),
    (6, 2): (1, 1, 100), (6, 6): (-16, -16, 40),
}
ZERO_UNIT = (6, 4)        # textured luma, both alphas 0: flat chroma, no CfL
FLAT_LUMA_UNIT = (5, 6)   # flat luma, textured chroma: no CfL


def _round2s(x, n):
    return np.where(x < 0, -((-x + (1 << (n - 1))) >> n), (x + (1 << (n - 1))) >> n)


def alpha_picture():
    """(Y, U, V) planes of the alpha picture."""
    rng = np.random.default_rng(11)
    y = np.full((ALPHA_H, ALPHA_W), 128, np.uint8)
    u = np.full((ALPHA_H // 2, ALPHA_W // 2), 128, np.uint8)
    v = np.full((ALPHA_H // 2, ALPHA_W // 2), 128, np.uint8)
    units = dict(DESIGN)
    units[ZERO_UNIT] = (0, 0, 40)
    for (r, c), (au, av, amp) in units.items():
        q = rng.integers(-amp, amp + 1, (8, 8))
        q[0, 0], q[7, 7] = -amp, amp     # the full swing occurs
        y[16 * r:16 * r + 16, 16 * c:16 * c + 16] = np.kron(128 + q, np.ones((2, 2), np.int64)).astype(np.uint8)
        lum = (128 + q) * 8              # (sum of the 2x2 samples) << 1
        ac = lum - ((int(lum.sum()) + 32) >> 6)
        for plane, a in ((u, au), (v, av)):
            plane[8 * r:8 * r + 8, 8 * c:8 * c + 8] = np.clip(128 + _round2s(a * ac, 6), 0, 255).astype(np.uint8)
    r, c = FLAT_LUMA_UNIT
    u[8 * r:8 * r + 8, 8 * c:8 * c + 8] = rng.integers(60, 200, (8, 8))
    v[8 * r:8 * r + 8, 8 * c:8 * c + 8] = rng.integers(60, 200, (8, 8))
    return y, u, v


HUES = [(255, 40, 20, 255), (30, 30, 255, 255), (255, 30, 255, 255), (40, 230, 40, 255)]   # BGRx: blue, red, magenta, green


def hue_texture(w: int, h: int, seed: int = 0) -> np.ndarray:
    """BGRx picture: four quadrants of one saturated colour each, brightness from a pseudo-random
    texture of 2x2 .. 4x4 pixel grains; `seed` selects another texture."""
    rng = np.random.default_rng(100 + seed)
    g = 2 + seed % 3
    t = np.kron(rng.integers(50, 256, ((h + g - 1) // g, (w + g - 1) // g)), np.ones((g, g), np.int64))[:h, :w]
    f = np.empty((h, w, 4), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    region = (yy >= h // 2) * 2 + (xx >= w // 2)
    for k, col in enumerate(HUES):
        m = region == k
        for ch in range(3):
            f[:, :, ch][m] = (t[m] * col[ch]) // 255
    f[:, :, 3] = 255
    return f


def window_frames(w: int, h: int, base: np.ndarray | None = None) -> list:
    """The window sequence of av1_intra_inter_util with the window filled by hue texture, a new
    texture in every frame from the window frame on."""
    seq = U.frames(w, h, base)
    x0, y0, ww, wh = U.window_rect(w, h)
    for k, f in enumerate(seq[U.WINDOW_FRAME:]):
        f[y0:y0 + wh, x0:x0 + ww] = hue_texture(ww, wh, k)
    return seq


ISO_INK = (40, 147, 200, 255)   # BGRx: the glyph field's background (230, 170, 60) at nearly its luma (145 against 146)


def combined_picture(w: int, h: int, seed: int = 0) -> np.ndarray:
    """Left half glyph field (chroma palettes), right half hue texture (CfL). The default glyph
    field has two colours, so its chroma is a linear function of its luma and CfL codes it in fewer
    bits than the palette. Here the ink has the background's luma within one step: the luma is not
    flat, so the blocks are CfL candidates, but it says nothing about the chroma, and the palette
    stands."""
    f = glyph_field(w, h, 2 * seed, ink=ISO_INK)
    f[:, w // 2:] = hue_texture(w - w // 2, h, seed)
    return f


def uv_mode(cells: np.ndarray) -> np.ndarray:
    return cells[..., BLK_UV_MODE]


def alphas(cells: np.ndarray):
    """(alpha_u, alpha_v) of every cell, [rows][cols] each: the int16 fields that hold the vector of an
    inter cell; meaningful where uv_mode is UV_CFL_PRED."""
    a = np.ascontiguousarray(cells[..., 4:8]).view(np.int16)
    return a[..., 0].astype(int), a[..., 1].astype(int)


def is_cfl(cells: np.ndarray) -> np.ndarray:
    """Intra cells with UV_CFL_PRED."""
    return ((cells[..., BLK_FLAGS] & 1) == 0) & (uv_mode(cells) == UV_CFL_PRED)
