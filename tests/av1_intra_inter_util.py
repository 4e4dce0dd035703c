"""Shared helpers of the AV1 intra-in-inter tests (test_av1_intra_inter.py, test_av1_intra_inter_gpu.py):
content in which a window opens over a desktop, and an encode loop that decodes every temporal
unit with dav1d and compares all planes with the encoder's reconstruction.

The sequence: frames 0..1 are SyntheticDesktop(kind="desktop") held still (its frame 0, so the
window is the only new content of the sequence), at frame 2 a window appears at a position that is
no multiple of 16 and covers about a third of the picture, frames 3..4 keep it and move one row of
glyphs. The window is a flat background with rows of two-colour 5x7 glyphs (its 16x16 units hold
2..8 luma values: the palette path) and, on its right, a 16-pixel-wide smooth gradient band (more
than 8 values: the transform intra path)."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
from tests.ltr_util import ref_planes

BLK_FLAGS, BLK_PAL_N, BLK_PAD1 = 3, 10, 11     # bytes of a BlkInfo cell (csrc/codec/av1_core.h)
BG, INK = (232, 236, 236, 255), (30, 30, 40, 255)
WINDOW_FRAME = 2
# 256x128 at 60 fps over the plain wallpaper: the window frame overflows its cap and is coded again
# (CPU encoder: one re-code pass, final QP 38; at 400 kbit/s and above it fits, at 200 and below
# the passes end at QP 51). Over the synthetic desktop no bitrate re-codes it: the key frame there
# costs three times the window frame, and the controller plans for it.
CBR_KBPS = 300


def window_rect(w: int, h: int):
    """(x0, y0, ww, wh) of the window."""
    x0, y0 = (40, 24) if w >= 128 and h >= 96 else (20, 12)
    ww, wh = int(w * 0.6), int(h * 0.55)
    return x0, y0, ww, wh


def band_cols(w: int, h: int):
    """Picture columns [gx0, gx1) of the gradient band (16 wide, near the window's right edge)."""
    x0, _, ww, _ = window_rect(w, h)
    return x0 + ww - 22, x0 + ww - 6


def draw_window(f: np.ndarray, shift: int = 0) -> np.ndarray:
    """Draws the window into the BGRx frame f; `shift` moves its second glyph row to the right."""
    h, w = f.shape[:2]
    x0, y0, ww, wh = window_rect(w, h)
    f[y0:y0 + wh, x0:x0 + ww] = BG
    gx0, gx1 = band_cols(w, h)
    rng = np.random.default_rng(5)
    glyphs = rng.integers(0, 2, (16, 7, 5)).astype(bool)
    for row, gy in enumerate(range(y0 + 4, y0 + wh - 8, 11)):
        dx = shift if row == 1 else 0
        for k, gx in enumerate(range(x0 + 4 + dx, gx0 - 8, 6)):
            g = glyphs[(3 * row + k) % 16]
            f[gy:gy + 7, gx:gx + 5][g] = INK
    yy, xx = np.mgrid[0:wh, 0:gx1 - gx0]
    v = np.clip(40 + (3 * yy) // 2 + 2 * xx, 0, 255).astype(np.uint8)
    f[y0:y0 + wh, gx0:gx1, 0] = v
    f[y0:y0 + wh, gx0:gx1, 1] = v
    f[y0:y0 + wh, gx0:gx1, 2] = 255 - v // 2
    return f


def frames(w: int, h: int, base: np.ndarray | None = None) -> list:
    """The five frames of the sequence; base: the picture under the window (default: the desktop)."""
    if base is None:
        base = SyntheticDesktop(w, h, kind="desktop").frame(0)
    out = [base.copy(), base.copy()]
    for shift in (0, 3, 6):
        out.append(draw_window(base.copy(), shift))
    return out


def wallpaper(w: int, h: int) -> np.ndarray:
    """A plain desktop (one colour with a coarse horizontal ramp): a key frame so cheap that the
    window frame is the costly one for a rate controller (the CBR re-code case)."""
    f = np.empty((h, w, 4), np.uint8)
    f[...] = (120, 80, 40, 255)
    f[:, :, 0] += (np.arange(w) // 8).astype(np.uint8)[None, :]
    return f


def two_colour_mask(w: int, h: int) -> np.ndarray:
    """Luma samples of the window's two-colour part: the window without the gradient band."""
    x0, y0, ww, wh = window_rect(w, h)
    m = np.zeros((h, w), bool)
    m[y0:y0 + wh, x0:band_cols(w, h)[0]] = True
    return m


def cells(enc, w: int, h: int) -> np.ndarray:
    """BlkInfo of every 8x8 cell of the frame just coded, [rows][cols][12 bytes]."""
    return enc.debug_buffer("blk").reshape((h + 7) // 8, (w + 7) // 8, 12)


def intra_cells(enc, w: int, h: int) -> np.ndarray:
    """[rows][cols] bool: cells of intra blocks (flags bit 0 clear)."""
    return (cells(enc, w, h)[:, :, BLK_FLAGS] & 1) == 0


def window_cells(w: int, h: int) -> np.ndarray:
    """[rows][cols] bool: cells whose 16x16 unit meets the window (the decision's granularity)."""
    x0, y0, ww, wh = window_rect(w, h)
    m = np.zeros(((h + 7) // 8, (w + 7) // 8), bool)
    m[(y0 // 16) * 2:((y0 + wh + 15) // 16) * 2, (x0 // 16) * 2:((x0 + ww + 15) // 16) * 2] = True
    return m


def check_intra_cells(enc, w: int, h: int) -> np.ndarray:
    """What every intra cell of an inter frame must satisfy; returns the intra mask."""
    c = cells(enc, w, h)
    intra = intra_cells(enc, w, h)
    assert (c[intra][:, BLK_PAD1] == 0).all(), "an intra block names a reference"
    assert (c[intra][:, 4:8] == 0).all(), "an intra block has a vector"
    assert (c[intra][:, 0] <= 2).all(), "an intra block is larger than 16x16"
    return intra


class Checked:
    """An encoder plus dav1d (where available): every temporal unit must decode to a picture whose
    planes all equal the encoder's reconstruction."""

    def __init__(self, enc, w: int, h: int):
        self.enc, self.w, self.h = enc, w, h
        self.dec = dav1d.Decoder() if dav1d.available() else None
        self.t = 0

    def step(self, frame) -> dict:
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
        return {"bytes": len(pk[0].data), "key": bool(pk[0].key), "data": bytes(pk[0].data), "rec": rec}


def run(enc, w: int, h: int, seq: list, hook=None) -> list:
    """Encodes seq through a Checked encoder; hook(t, enc, result) after each frame."""
    ck = Checked(enc, w, h)
    out = []
    for t, f in enumerate(seq):
        out.append(ck.step(f))
        if hook:
            hook(t, enc, out[-1])
    return out


def src_luma(enc, w: int, h: int) -> np.ndarray:
    sy, ph = ((w + 15) // 16) * 16, ((h + 15) // 16) * 16
    return enc.debug_buffer("src_y").reshape(ph, sy)[:h, :w].copy()
