"""Shared helpers of the HEVC long-term reference cache tests (test_hevc_ltr.py, test_hevc_ltr_gpu.py,
test_hevc_rps_vectors.py): an encode loop that decodes every packet with the test decoder (whose DPB
raises on an RPS that names a missing picture, on slices that disagree, on a list entry out of
range and on an RPS over sps_max_dec_pic_buffering_minus1) and compares the decoded picture with
the encoder's reference planes; the window-switch content is tests/ltr_util.py's."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.models.hevc.decoder import HevcDecoder
from selkies_gstreamer_amd.ops.native import HevcEncoder
from tests.ltr_util import (H, STRIPE, W, contents, final_actions, ltr_slots_of_tasks, ltr_valid,  # noqa: F401
                            make_enc, ref_planes, sequence)                                       # (re-exported)


def hevc_enc(slots=None, w=W, h=H, backend="cpu", **kw):
    return make_enc(HevcEncoder, slots, w, h, backend, **kw)


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
