"""Shared helpers of the long-term reference cache tests of all three codecs: window-switch content,
the encoder factory's defaults, readers of the cache's debug buffers, and the H.264 encode loop that
decodes every packet and compares the decoder's picture with the encoder's reference planes
(hevc_ltr_util.py and av1_ltr_util.py hold their codec's loop)."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.ops.native import LTR_STATE_DTYPE, LTR_TASK_DTYPE, ME_DTYPE, TASK_DTYPE
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


def make_enc(cls, slots=None, w=W, h=H, backend="cpu", **kw):
    """An encoder of class `cls` with the LTR tests' defaults; slots None: ltr_slots left unset."""
    kw = dict(dict(stripe_height=STRIPE, qp=24, use_paint_over=False), **kw)
    if slots is not None:
        kw["ltr_slots"] = slots
    return cls(w, h, backend=backend, **kw)


def ref_planes(enc, w, h):
    """The encoder's reference picture, cropped to w x h: (Y, U, V)."""
    sy, ph = ((w + 15) // 16) * 16, ((h + 15) // 16) * 16
    ry = enc.debug_buffer("ref_y").reshape(ph, sy)[:h, :w]
    ru = enc.debug_buffer("ref_u").reshape(ph // 2, sy // 2)[:h // 2, :w // 2]
    rv = enc.debug_buffer("ref_v").reshape(ph // 2, sy // 2)[:h // 2, :w // 2]
    return ry, ru, rv


def ltr_tasks(enc) -> np.ndarray:
    """LtrTask of every slice of the frame just coded."""
    return enc.debug_buffer("ltr_task", LTR_TASK_DTYPE)


def ltr_slots_of_tasks(enc) -> list:
    """LtrTask::slot of every slice of the frame just coded."""
    return ltr_tasks(enc)["slot"].tolist()


def ltr_valid(enc) -> int:
    """LtrState::valid of the picture's stream (the last state)."""
    return int(enc.debug_buffer("ltr_state", LTR_STATE_DTYPE)["valid"][-1])


def final_actions(enc) -> list:
    """SliceTask::final_action of every slice of the frame just coded (1 = P, 2 = I, 3 = skip-all)."""
    return enc.debug_buffer("tasks", TASK_DTYPE)["final_action"].tolist()


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
        ry, ru, rv = ref_planes(self.enc, self.w, self.h)
        assert np.array_equal(self.dec.Y, ry), "decoder luma differs from the encoder's reference"
        assert np.array_equal(self.dec.U, ru) and np.array_equal(self.dec.V, rv), "decoder chroma differs"
        me = self.enc.debug_buffer("me", ME_DTYPE)
        out = {"bytes": sum(len(p.data) for p in pk), "key": any(p.key for p in pk), "ref1": int((me["ref"] == 1).sum()),
               "packets": [(p.y, p.key, p.data) for p in pk]}
        if src_psnr:
            sy, ph = ((self.w + 15) // 16) * 16, ((self.h + 15) // 16) * 16
            sy_ = self.enc.debug_buffer("src_y").reshape(ph, sy)[:self.h, :self.w]
            out["psnr"] = psnr(sy_, ry)
        return out
