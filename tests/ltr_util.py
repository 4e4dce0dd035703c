"""Shared helpers of the long-term reference cache tests (test_h264_ltr.py, test_h264_ltr_gpu.py):
window-switch content, and an encode loop that decodes every packet and compares the decoder's
picture with the encoder's reference planes."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.ops.native import ME_DTYPE
from tests.h264_util import StripeDecoder, psnr, synthetic_frames

W, H = 208, 112          # 13 x 7 MBs; with stripe_height 32: four stripes, the last of one MB row
STRIPE = 32


def contents(w: int = W, h: int = H) -> dict:
    """Three full-screen "windows" that differ from each other in every macroblock: different
    synthetic desktops, rolled horizontally, with a colour offset."""
    out = {}
    for name, seed, roll, off in (("A", 11, 0, 0), ("B", 23, 57, 40), ("C", 37, 121, 90)):
        f = next(synthetic_frames(w, h, 1, seed=seed)).copy()
        f = np.roll(f, roll, axis=1)
        f[..., :3] = (f[..., :3].astype(np.int32) + off) % 256
        out[name] = f
    return out


def sequence(spec: str, w: int = W, h: int = H):
    """Frames of e.g. "A10 B10 A3": (label, frame index in its run, BGRx frame) with a 2 x 16 caret
    that blinks every frame inside the first macroblock row."""
    c = contents(w, h)
    t = 0
    for item in spec.split():
        name, n = item[0], int(item[1:])
        for k in range(n):
            f = c[name].copy()
            if t & 1:
                f[0:16, 40:42, :3] = 255
            yield name, k, f
            t += 1


class Checked:
    """An encoder plus its decoders: every packet must decode, and the decoded picture must equal
    the encoder's reference planes."""

    def __init__(self, enc, w: int = W, h: int = H):
        self.enc, self.w, self.h = enc, w, h
        self.dec = StripeDecoder(w, h)
        self.t = 0

    def step(self, frame, src_psnr: bool = False) -> dict:
        pk = self.enc.encode(frame, self.t)
        self.t += 1
        for p in pk:
            self.dec.feed(p.data)
        sy = ((self.w + 15) // 16) * 16
        ph = ((self.h + 15) // 16) * 16
        ry = self.enc.debug_buffer("ref_y").reshape(ph, sy)[:self.h, :self.w]
        ru = self.enc.debug_buffer("ref_u").reshape(ph // 2, sy // 2)[:self.h // 2, :self.w // 2]
        rv = self.enc.debug_buffer("ref_v").reshape(ph // 2, sy // 2)[:self.h // 2, :self.w // 2]
        assert np.array_equal(self.dec.Y, ry), "decoder luma differs from the encoder's reference"
        assert np.array_equal(self.dec.U, ru) and np.array_equal(self.dec.V, rv), "decoder chroma differs"
        me = self.enc.debug_buffer("me", ME_DTYPE)
        out = {"bytes": sum(len(p.data) for p in pk), "key": any(p.key for p in pk), "ref1": int((me["ref"] == 1).sum()),
               "packets": [(p.y, p.key, p.data) for p in pk]}
        if src_psnr:
            sy_ = self.enc.debug_buffer("src_y").reshape(ph, sy)[:self.h, :self.w]
            out["psnr"] = psnr(sy_, ry)
        return out
