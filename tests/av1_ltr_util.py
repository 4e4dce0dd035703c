"""Shared helpers of the AV1 long-term reference cache tests (test_av1_ltr.py, test_av1_ltr_gpu.py):
an encode loop that decodes every temporal unit with dav1d and compares the picture with the
encoder's reference planes, a parser for the reference buffers a frame header names, and an
independent replay of the decoder's buffer map. The window-switch content is tests/ltr_util.py's."""
from __future__ import annotations

import numpy as np

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import Av1Encoder
from tests.ltr_util import (H, STRIPE, W, contents, ltr_slots_of_tasks, ltr_tasks, ltr_valid, make_enc,  # noqa: F401
                            ref_planes, sequence)                                                    # (re-exported)

BLK_REF = 11           # BlkInfo's last byte: the block's reference, 0 = LAST, 1 = LAST2


def av1_enc(slots=None, w=W, h=H, backend="cpu", **kw):
    return make_enc(Av1Encoder, slots, w, h, backend, **kw)


def blk_refs(enc, w, h) -> np.ndarray:
    """The reference byte of every 8x8 cell, [rows][cols]."""
    return enc.debug_buffer("blk").reshape((h + 7) // 8, (w + 7) // 8, 12)[:, :, BLK_REF]


# ---- frame header: the reference buffers --------------------------------------------------------
def _leb128(b: bytes, i: int):
    v = s = 0
    while True:
        v |= (b[i] & 0x7f) << s
        s += 7
        i += 1
        if not b[i - 1] & 0x80:
            return v, i


def parse_refs(tu: bytes) -> dict:
    """{"key", "refresh", "idx"} of a temporal unit's OBU_FRAME: refresh_frame_flags and
    ref_frame_idx[0..6] (a shown key frame refreshes every buffer and names none). The header up to
    there is fixed for these streams: show_existing_frame 1, frame_type 2, show_frame 1,
    error_resilient_mode 1 (inter), disable_cdf_update 1, allow_screen_content_tools 1,
    frame_size_override_flag 1, primary_ref_frame 3."""
    i = 0
    while i < len(tu):
        typ = (tu[i] >> 3) & 15
        assert tu[i] & 2, "obu_has_size_field"
        n, i = _leb128(tu, i + 1)
        if typ == 6:
            bits = int.from_bytes(tu[i:i + 8], "big")

            def take(pos, cnt):
                return (bits >> (64 - pos - cnt)) & ((1 << cnt) - 1)
            assert take(0, 1) == 0
            if take(1, 2) == 0:
                return {"key": True, "refresh": 0xff, "idx": []}
            assert take(1, 2) == 1 and take(3, 1) == 1
            assert take(8, 3) == 7, "primary_ref_frame"
            return {"key": False, "refresh": take(11, 8), "idx": [take(19 + 3 * k, 3) for k in range(7)]}
        i += n
    raise AssertionError("no OBU_FRAME")


class BufferModel:
    """The decoder's eight reference buffers as the issue states them: which one holds the previous
    picture and which one holds each cached slot."""

    def __init__(self):
        self.last, self.slot_buf = 0, {}

    def key(self):
        self.last, self.slot_buf = 0, {}

    def inter(self, store_slot: int, used_slot: int):
        """-> (refresh_frame_flags, ref_frame_idx[0], ref_frame_idx[1]) of an inter frame."""
        idx0 = self.last
        idx1 = self.slot_buf[used_slot] if used_slot >= 0 else self.last
        if store_slot >= 0:
            self.slot_buf.pop(store_slot, None)        # an evicted slot's buffer is free again
            self.slot_buf[store_slot] = self.last      # the previous picture stays where it is
            self.last = min(b for b in range(8) if b not in self.slot_buf.values())
        return 1 << self.last, idx0, idx1


class CheckedAv1:
    """An AV1 encoder plus dav1d: every temporal unit must decode to a picture that equals the
    encoder's reference planes; the header's buffers must equal the replayed model's."""

    def __init__(self, enc, w: int = W, h: int = H, model: bool = True):
        self.enc, self.w, self.h = enc, w, h
        self.dec = dav1d.Decoder()
        self.model = BufferModel() if model else None
        self.t = 0

    def step(self, frame) -> dict:
        pk = self.enc.encode(frame, self.t)
        self.t += 1
        assert len(pk) == 1
        tu = bytes(pk[0].data[10:])
        pic = self.dec.decode(tu)
        assert pic is not None, f"frame {self.t - 1}: dav1d returned no picture"
        for a, b, n in zip(pic, ref_planes(self.enc, self.w, self.h), "YUV"):
            assert np.array_equal(a, b), f"frame {self.t - 1}: dav1d's {n} differs from the encoder's reference"
        out = {"bytes": len(pk[0].data), "key": bool(pk[0].key), "data": bytes(pk[0].data), "refs": parse_refs(tu)}
        assert out["refs"]["key"] == out["key"]
        if self.model is not None:
            lt = ltr_tasks(self.enc)
            out["slots"], out["store"] = lt["slot"].tolist(), int(lt["store_slot"][0])
            out["valid"] = ltr_valid(self.enc)
            used = sorted({s for s in out["slots"] if s >= 0})
            assert len(used) <= 1, f"frame {self.t - 1}: more than one cached picture in a frame: {used}"
            if out["key"]:
                self.model.key()
            else:
                want = self.model.inter(out["store"], used[0] if used else -1)
                r = out["refs"]
                assert (r["refresh"], r["idx"][0], r["idx"][1]) == want, f"frame {self.t - 1}: header {r}, model {want}"
                assert all(i == r["idx"][0] for i in r["idx"][2:])
                cached = set(self.model.slot_buf.values())
                assert not any((r["refresh"] >> b) & 1 for b in cached), "a cached buffer is refreshed"
                if out["store"] >= 0:
                    assert r["refresh"] != 1 << r["idx"][0], "a store must move the new picture to another buffer"
            out["bufs"] = dict(self.model.slot_buf)
        return out


def frames(spec: str, w=W, h=H, caret=True):
    """`sequence` without its labels. caret=False: the plain contents. At 64x64 the caret's
    macroblock is 1/16 of the picture, which is not a quiet frame (ltr.h: fewer than 1/16), so
    a content with it never settles there."""
    if caret:
        return [f for _, _, f in sequence(spec, w, h)]
    c = contents(w, h)
    return [c[item[0]] for item in spec.split() for _ in range(int(item[1:]))]


def run_spec(spec: str, slots, w=W, h=H, hook=None, caret=True, **kw) -> list:
    run = CheckedAv1(av1_enc(slots, w, h, **kw), w, h, model=bool(slots))
    out = []
    for t, f in enumerate(frames(spec, w, h, caret)):
        if hook:
            hook(t, run.enc)
        out.append(run.step(f))
    return out
