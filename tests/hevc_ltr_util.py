"""Shared helpers of the HEVC long-term reference cache tests (test_hevc_ltr.py, test_hevc_ltr_gpu.py,
test_hevc_rps_vectors.py): an encode loop that decodes every packet with the test decoder (whose DPB
raises on an RPS that names a missing picture, on slices that disagree, on a list entry out of
range and on an RPS over sps_max_dec_pic_buffering_minus1) and compares the decoded picture with
the encoder's reference planes; the window-switch content is tests/ltr_util.py's."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.models.hevc.decoder import HevcDecoder
from selkies_gstreamer_amd.ops.native import HevcEncoder
from tests.ltr_util import H, STRIPE, W, contents, sequence  # noqa: F401  (re-exported)

LTR_TASK_WORDS = 8     # sizeof(LtrTask) / 4: slot, store_slot, mmco1, flags, ref1_mbs, pad[3]
LTR_STATE_WORDS = 24   # sizeof(LtrState) / 4: quiet_run, cur_slot, clock, valid, stamp[8], n_st, st_fn[9], pad[2]


def hevc_enc(slots=None, w=W, h=H, backend="cpu", **kw):
    kw = dict(dict(stripe_height=STRIPE, qp=24, use_paint_over=False), **kw)
    if slots is not None:
        kw["ltr_slots"] = slots
    return HevcEncoder(w, h, backend=backend, **kw)


def ref_planes(enc, w, h):
    sy, ph = ((w + 15) // 16) * 16, ((h + 15) // 16) * 16
    ry = enc.debug_buffer("ref_y").reshape(ph, sy)[:h, :w]
    ru = enc.debug_buffer("ref_u").reshape(ph // 2, sy // 2)[:h // 2, :w // 2]
    rv = enc.debug_buffer("ref_v").reshape(ph // 2, sy // 2)[:h // 2, :w // 2]
    return ry, ru, rv


def ltr_slots_of_tasks(enc) -> list:
    """LtrTask::slot of every slice of the frame just coded."""
    return enc.debug_buffer("ltr_task", np.int32).reshape(-1, LTR_TASK_WORDS)[:, 0].tolist()


def ltr_valid(enc) -> int:
    """LtrState::valid of the picture's stream (the last state)."""
    return int(enc.debug_buffer("ltr_state", np.int32).reshape(-1, LTR_STATE_WORDS)[-1, 3])


def final_actions(enc) -> list:
    """SliceTask::final_action of every slice of the frame just coded (1 = P, 2 = I, 3 = skip-all)."""
    return enc.debug_buffer("tasks", np.int32).reshape(-1, 12)[:, 10].tolist()


class CheckedHevc:
    """An HEVC encoder plus the test decoder: every packet must decode to exactly one picture that
    equals the encoder's reference planes."""

    def __init__(self, enc, w: int = W, h: int = H):
        self.enc, self.w, self.h = enc, w, h
        self.dec = HevcDecoder()
        self.t = 0

    def step(self, frame, decode: bool = True) -> dict:
        pk = self.enc.encode(frame, self.t)
        self.t += 1
        assert len(pk) == 1
        if decode:
            pics = self.dec.decode(pk[0].data[10:])
            assert len(pics) == 1
            for a, b, n in zip(pics[0], ref_planes(self.enc, self.w, self.h), "YUV"):
                assert np.array_equal(a, b), f"frame {self.t - 1}: decoder {n} differs from the encoder's reference"
        return {"bytes": len(pk[0].data), "key": bool(pk[0].key), "data": pk[0].data,
                "list0": self.dec.last_list0, "rps": self.dec.last_rps}
