"""Shared helpers of the AV1 chroma palette tests (test_av1_chroma_palette.py,
test_av1_chroma_palette_gpu.py): two contents, accessors of the chroma palette's cells, and an
encode loop for planar input that decodes every temporal unit with dav1d.

glyph field: a BGRx picture that is two-colour 5x7 glyphs on a flat tinted background all over.
The front end sums R, G and B over each 2x2 quad before the matrix, so a chroma sample depends only
on how many of its four pixels are ink: at most five (Cb, Cr) pairs in any block.

pairs picture: 128x128 I420 planes for encode_yuv with flat luma. Each 16x16 unit's 8x8 chroma
block holds one designed set of (U, V) pairs in a pseudo-random arrangement (PAIR_SETS); every other
unit is one flat pair. 128 rows: the units of row 4 start a superblock row (mi row 16) and see no
palette cache from above."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.models.av1 import dav1d
from tests.ltr_util import ref_planes

BLK_BSL, BLK_FLAGS, BLK_PAL_N = 0, 3, 10     # bytes of a BlkInfo cell (csrc/codec/av1_core.h)
PAIRS_W = PAIRS_H = 128
FLAT = (128, 128)
_SHARED = [(40, 220), (90, 30), (160, 200), (230, 60)]
_EIGHT = [(20, 200), (50, 40), (80, 230), (110, 20), (140, 180), (170, 70), (200, 250), (240, 10)]
# unit (row, col) -> (name, pairs). Names as in the feature's description:
#   a  two pairs with equal U (the second U is a zero delta)
#   b  V that is cheap only with wrap-around (250, 3, 248, 5 in U order)
#   c  a V delta of 128: no wrapped delta fits, V is coded raw
#   d  eight pairs;  e  nine pairs (no palette);  f  one pair (no palette)
#   g* neighbours that share colours: cache hits from the left (g2, g3), from above and left (g5)
#   h  below d across a superblock row boundary with three of d's pairs: no cache from above
PAIR_SETS = {
    (1, 1): ("a", [(100, 40), (100, 200)]),
    (1, 3): ("b", [(60, 250), (90, 3), (120, 248), (150, 5)]),
    (1, 5): ("c", [(50, 10), (200, 138)]),
    (3, 1): ("d", _EIGHT),
    (3, 3): ("e", _EIGHT + [(250, 128)]),
    (3, 5): ("f", [(60, 190)]),
    (4, 1): ("h", _EIGHT[:3] + [(250, 120)]),
    (5, 1): ("g1", _SHARED[:3]),
    (5, 2): ("g2", _SHARED[1:]),
    (5, 3): ("g3", _SHARED),
    (6, 1): ("g4", _SHARED[:2]),
    (6, 2): ("g5", [_SHARED[0], _SHARED[2], _SHARED[3], (250, 250)]),
}


def pairs_picture():
    """(Y, U, V) planes of the pairs picture."""
    rng = np.random.default_rng(7)
    y = np.full((PAIRS_H, PAIRS_W), 128, np.uint8)
    u = np.full((PAIRS_H // 2, PAIRS_W // 2), FLAT[0], np.uint8)
    v = np.full((PAIRS_H // 2, PAIRS_W // 2), FLAT[1], np.uint8)
    for (r, c), (_, pairs) in PAIR_SETS.items():
        k = len(pairs)
        idx = np.concatenate([np.arange(k), rng.integers(0, k, 64 - k)])   # every pair occurs
        rng.shuffle(idx)
        p = np.array(pairs, np.uint8)[idx].reshape(8, 8, 2)
        u[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = p[:, :, 0]
        v[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = p[:, :, 1]
    return y, u, v


def glyph_field(w: int, h: int, shift: int = 0, bg=(230, 170, 60, 255), ink=(40, 30, 200, 255)) -> np.ndarray:
    """BGRx picture: rows of 5x7 glyphs in `ink` on `bg` over the whole picture, cut at its edges;
    `shift` moves every second glyph row to the right."""
    f = np.empty((h, w, 4), np.uint8)
    f[...] = bg
    glyphs = np.random.default_rng(5).integers(0, 2, (16, 7, 5)).astype(bool)
    for row, gy in enumerate(range(1, h, 9)):
        dx = shift if row & 1 else 0
        for k, gx in enumerate(range(1 + dx, w, 6)):
            g = glyphs[(3 * row + k) % 16][:h - gy, :w - gx]
            f[gy:gy + 7, gx:gx + 5][g] = ink
    return f


def cells(enc, w: int, h: int) -> np.ndarray:
    """BlkInfo of every 8x8 cell of the frame just coded, [rows][cols][12 bytes]."""
    return enc.debug_buffer("blk").reshape((h + 7) // 8, (w + 7) // 8, 12)


def uv_count(enc, w: int, h: int) -> np.ndarray:
    """PaletteSizeUV of every 8x8 cell, [rows][cols]: the high nibble of BlkInfo byte 10."""
    return cells(enc, w, h)[:, :, BLK_PAL_N] >> 4


def pal_uv(enc, w: int, h: int) -> np.ndarray:
    """The chroma palette cells, [rows][cols][16]: U colours at 0..7, V at 8..15; meaningful where
    uv_count is nonzero."""
    return enc.debug_buffer("pal_uv").reshape((h + 7) // 8, (w + 7) // 8, 16)


def src_planes(enc, w: int, h: int):
    """The source picture of the frame just coded, cropped like ref_planes: (Y, U, V)."""
    sy, ph = ((w + 15) // 16) * 16, ((h + 15) // 16) * 16
    y = enc.debug_buffer("src_y").reshape(ph, sy)[:h, :w]
    u = enc.debug_buffer("src_u").reshape(ph // 2, sy // 2)[:h // 2, :w // 2]
    v = enc.debug_buffer("src_v").reshape(ph // 2, sy // 2)[:h // 2, :w // 2]
    return y.copy(), u.copy(), v.copy()


def chroma_sse(src, rec, mask=None) -> int:
    """Squared error of both chroma planes, over the luma mask subsampled 2:1 if given."""
    e = 0
    for p in (1, 2):
        d = (src[p].astype(np.int64) - rec[p].astype(np.int64)) ** 2
        e += int(d[mask[::2, ::2][:d.shape[0], :d.shape[1]]].sum() if mask is not None else d.sum())
    return e


class Checked:
    """An encoder plus dav1d (where available): every temporal unit must decode to a picture whose
    planes all equal the encoder's reconstruction. A frame is a BGRx array or a (Y, U, V) tuple."""

    def __init__(self, enc, w: int, h: int):
        self.enc, self.w, self.h = enc, w, h
        self.dec = dav1d.Decoder() if dav1d.available() else None
        self.t = 0

    def step(self, frame) -> dict:
        if isinstance(frame, tuple):
            pk = self.enc.encode_yuv("i420", *frame, frame_id=self.t)
        else:
            pk = self.enc.encode(frame, self.t)
        self.t += 1
        assert len(pk) == 1
        rec = [p.copy() for p in ref_planes(self.enc, self.w, self.h)]
        if self.dec is not None:
            pic = self.dec.decode(bytes(pk[0].data[10:]))
            assert pic is not None, f"frame {self.t - 1}: dav1d returned no picture"
            for a, b, n in zip(pic, rec, "YUV"):
                assert np.array_equal(a, b), f"frame {self.t - 1}: dav1d's {n} differs from the encoder's " \
                                             f"reconstruction at {np.argwhere(a != b)[:3].tolist()}"
        return {"bytes": len(pk[0].data), "key": bool(pk[0].key), "data": bytes(pk[0].data), "rec": rec,
                "src": src_planes(self.enc, self.w, self.h), "cells": cells(self.enc, self.w, self.h).copy(),
                "pal_uv": pal_uv(self.enc, self.w, self.h).copy()}


def run(enc, w: int, h: int, seq: list, hook=None) -> list:
    """Encodes seq through a Checked encoder; hook(t, enc, result) after each frame."""
    ck = Checked(enc, w, h)
    out = []
    for t, f in enumerate(seq):
        out.append(ck.step(f))
        if hook:
            hook(t, enc, out[-1])
    return out
