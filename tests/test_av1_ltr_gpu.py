"""AV1 long-term reference cache on the HIP backend (k_ltr_match / k_ltr_decide with the tile row as
the decision unit, the per-slice reference planes and the reference byte in k_av1_inter, the LAST2
symbol in k_av1_tokens, the buffer map and header words in k_av1_setup, the slot copy in k_commit,
the LtrState commit in k_plan): byte for byte against the CPU reference encoder on window-switch
sequences: packets, block decisions, levels, the cache's state, per-slice decisions, reference and
slot planes after every frame. The switch frames and their successors are decoded by dav1d."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import hip_device_count
from tests.av1_ltr_util import (H, STRIPE, W, av1_enc, blk_refs, contents, frames, ltr_slots_of_tasks, ltr_valid,
                                parse_refs, ref_planes)

pytestmark = pytest.mark.gpu

SPEC = "A10 B10 A2 B2"
# CBR: window A comes back with new content in it (noise over most of the picture), so the switch-back
# frame 20 predicts from the cache and still exceeds its cap: the CPU model takes two re-code
# passes for it at this bitrate (redos 0 -> 2), every tile row on slot 0
CBR_KBPS = 2000


@pytest.fixture(autouse=True)
def _need_gpu():
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    if not dav1d.available():
        pytest.skip("dav1d (Pillow's libavif) not found")


def _pair(slots, w=W, h=H, **kw):
    return av1_enc(slots, w, h, backend="cpu", **kw), av1_enc(slots, w, h, backend="hip", **kw)


def _same(cpu, gpu, slots, t):
    names = ("blk", "levels", "ref_y", "ref_u", "ref_v", "ltr_state", "ltr_task") + tuple(f"ltr{j}_y" for j in range(slots))
    for name in names:
        a, b = cpu.debug_buffer(name), gpu.debug_buffer(name)
        assert np.array_equal(a, b), f"frame {t}: {name} differs ({np.sum(a != b)} bytes)"


class Run:
    """CPU and HIP encoders in lockstep. dav1d needs every picture since the last key frame, so
    temporal units wait in `pending` until a step asks for decoding: pictures after the last
    checked one are never decoded, and only the checked ones are compared with the reference planes."""

    def __init__(self, slots, w=W, h=H, **kw):
        self.cpu, self.gpu = _pair(slots, w, h, **kw)
        self.slots, self.w, self.h = slots, w, h
        self.dec = dav1d.Decoder()
        self.pending = []
        self.t = 0

    def step(self, f, decode=False):
        t = self.t
        pc, pg = self.cpu.encode(f, t), self.gpu.encode(f, t)
        assert [(p.key, bytes(p.data)) for p in pg] == [(p.key, bytes(p.data)) for p in pc], f"frame {t}: packets differ"
        _same(self.cpu, self.gpu, self.slots, t)
        self.t += 1
        if pg[0].key:         # a key frame refreshes every buffer: nothing before it is needed
            self.pending = []
        self.pending.append(bytes(pg[0].data[10:]))
        if decode:
            for d in self.pending:
                pic = self.dec.decode(d)
            self.pending = []
            for a, b, n in zip(pic, ref_planes(self.gpu, self.w, self.h), "YUV"):
                assert np.array_equal(a, b), f"frame {t}: dav1d's {n} differs from the encoder's reference"
        return pg[0]


def _decode_all_needed(run, seq, frames_to_decode, hook=None):
    out = []
    for t, f in enumerate(seq):
        if hook:
            hook(t, run)
        p = run.step(f, decode=t in frames_to_decode)
        out.append({"key": bool(p.key), "bytes": len(p.data), "slots": ltr_slots_of_tasks(run.gpu),
                    "valid": ltr_valid(run.gpu), "redos": run.gpu.rc_stats()["redos"],
                    "refs": parse_refs(bytes(p.data[10:]))})
    return out


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("w,h,stripe", [(W, H, STRIPE), (264, 136, 64)])
def test_av1_ltr_gpu_matches_cpu(w, h, stripe, slots):
    run = Run(slots, w, h, stripe_height=stripe)
    out = _decode_all_needed(run, frames(SPEC, w, h), {20, 21, 22, 23})
    for t in (20, 22):        # the switches back: every tile row predicts from the cache, no key frame
        assert not out[t]["key"] and all(s >= 0 for s in out[t]["slots"]), out[t]
        assert out[t]["bytes"] < 0.7 * out[10]["bytes"]
        assert out[t]["refs"]["idx"][1] != out[t]["refs"]["idx"][0]
    assert out[-1]["valid"] == (1 if slots == 1 else 3)


def test_av1_ltr_gpu_cbr_recode_reads_the_slot_again():
    """CBR at a bitrate that forces re-code passes on the switch-back frame: the passes reuse the
    decision and read the slot again, the slot copy happens after the last pass."""
    seq = frames("A10 B10 A2")
    rng = np.random.default_rng(5)
    seq[20] = seq[20].copy()
    seq[20][8:104, 16:192, :3] = rng.integers(0, 256, (96, 176, 3), dtype=np.uint8)
    seq[21] = seq[21].copy()
    seq[21][8:104, 16:192, :3] = seq[20][8:104, 16:192, :3]
    run = Run(2, rate_control="cbr", bitrate_kbps=CBR_KBPS)
    out = _decode_all_needed(run, seq, {20, 21})
    assert not out[20]["key"] and all(s >= 0 for s in out[20]["slots"])
    assert out[20]["redos"] > out[19]["redos"], "frame 20 took no re-code pass"
    assert run.gpu.rc_stats()["redos"] == run.cpu.rc_stats()["redos"]


def test_av1_ltr_gpu_mixed_picture():
    c = contents()
    run = Run(2)
    for f in frames("A10 B10"):
        run.step(f)
    mixed = c["B"].copy()
    mixed[:64] = c["A"][:64]
    p = run.step(mixed, decode=True)
    s = ltr_slots_of_tasks(run.gpu)
    assert not p.key and s[0] >= 0 and s[1] >= 0 and s[2] < 0 and s[3] < 0, s
    refs = blk_refs(run.gpu, W, H)
    assert (refs[:8] == 1).all() and (refs[8:] == 0).all()    # tile row 0: LAST2, tile row 1: LAST
    for _ in range(2):
        assert not run.step(mixed, decode=True).key


def test_av1_ltr_gpu_keyframe_request_empties_the_cache():
    def hook(t, run):
        if t == 15:
            run.cpu.request_keyframe()
            run.gpu.request_keyframe()
    run = Run(2)
    out = _decode_all_needed(run, frames("A10 B10 A2"), {20, 21}, hook)
    assert out[15]["key"] and out[14]["valid"] == 1 and out[15]["valid"] == 0
    assert not out[20]["key"] and all(s < 0 for s in out[20]["slots"])


def test_av1_ltr_gpu_state_export_import():
    seq = frames(SPEC)
    cpu, a = _pair(2)
    for t, f in enumerate(seq[:20]):
        a.encode(f, t)
    state = a.export_state()
    b = av1_enc(2, backend="hip")
    b.import_state(state)
    cpu.import_state(state)
    for t, f in enumerate(seq[20:], 20):
        pa, pb, pc = a.encode(f, t), b.encode(f, t), cpu.encode(f, t)
        assert [(p.key, bytes(p.data)) for p in pa] == [(p.key, bytes(p.data)) for p in pb] \
            == [(p.key, bytes(p.data)) for p in pc]
        assert not any(p.key for p in pb)
        _same(cpu, b, 2, t)
    assert ltr_valid(b) == 3
