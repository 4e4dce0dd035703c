"""HEVC long-term reference cache on the HIP backend (k_ltr_match / k_ltr_decide in exclusive mode with
expiry, the per-slice reference-0 planes in k_me / k_subpel / k_hevc_inter, the RPS and list
modification in k_hevc_hdr, the slot copy in k_commit, the LtrState commit in k_plan): byte for byte
against the CPU reference encoder on window-switch sequences: packets, CU decisions, levels, the
cache's state, per-slice decisions, reference and slot planes after every frame. The switch frames
and their successors are decoded too (DPB checked by the test decoder)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.hevc.decoder import HevcDecoder
from selkies_gstreamer_amd.ops.native import hip_device_count
from tests.hevc_ltr_util import (H, STRIPE, W, contents, hevc_enc, ltr_slots_of_tasks, ltr_valid, ref_planes,
                                 sequence)

pytestmark = pytest.mark.gpu

SPEC = "A10 B10 A2 B2"
CBR_KBPS = 1000   # the switch-back frame 20 itself takes re-code passes at this budget (CPU model: redos 2 -> 4)


@pytest.fixture(autouse=True)
def _need_gpu():
    if hip_device_count() < 1:
        pytest.skip("no HIP device")


def _pair(slots, w=W, h=H, **kw):
    return hevc_enc(slots, w, h, backend="cpu", **kw), hevc_enc(slots, w, h, backend="hip", **kw)


def _same(cpu, gpu, slots, t):
    names = ("cus", "coefs", "ref_y", "ref_u", "ref_v", "ltr_state", "ltr_task") + tuple(f"ltr{j}_y" for j in range(slots))
    for name in names:
        a, b = cpu.debug_buffer(name), gpu.debug_buffer(name)
        assert np.array_equal(a, b), f"frame {t}: {name} differs ({np.sum(a != b)} bytes)"


class Run:
    """CPU and HIP encoders in lockstep. The decoder needs every picture since the last key frame for
    its DPB, so packets wait in `pending` until a step asks for decoding: pictures after the last
    checked one are never decoded, and only the checked ones are compared with the reference planes."""

    def __init__(self, slots, w=W, h=H, **kw):
        self.cpu, self.gpu = _pair(slots, w, h, **kw)
        self.slots, self.w, self.h = slots, w, h
        self.dec = HevcDecoder()
        self.pending = []
        self.t = 0

    def step(self, f, decode=False):
        t = self.t
        pc, pg = self.cpu.encode(f, t), self.gpu.encode(f, t)
        assert [(p.key, p.data) for p in pg] == [(p.key, p.data) for p in pc], f"frame {t}: packets differ"
        _same(self.cpu, self.gpu, self.slots, t)
        self.t += 1
        if pg[0].key:         # a key picture restarts the decoder: nothing before it is needed
            self.pending = []
            self.dec = HevcDecoder()
        self.pending.append(pg[0].data[10:])
        if decode:
            for d in self.pending:
                pics = self.dec.decode(d)
            self.pending = []
            for a, b, n in zip(pics[-1], ref_planes(self.gpu, self.w, self.h), "YUV"):
                assert np.array_equal(a, b), f"frame {t}: decoder {n} differs from the encoder's reference"
        return pg[0]


def _decode_all_needed(run, spec, frames_to_decode, hook=None, w=W, h=H):
    out = []
    for t, (name, k, f) in enumerate(sequence(spec, w, h)):
        if hook:
            hook(t, run)
        p = run.step(f, decode=t in frames_to_decode)
        out.append({"key": bool(p.key), "bytes": len(p.data), "slots": ltr_slots_of_tasks(run.gpu),
                    "valid": ltr_valid(run.gpu), "redos": run.gpu.rc_stats()["redos"]})
    return out


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("w,h,stripe", [(W, H, STRIPE), (264, 136, 64)])
def test_hevc_ltr_gpu_matches_cpu(w, h, stripe, slots):
    run = Run(slots, w, h, stripe_height=stripe)
    out = _decode_all_needed(run, SPEC, {20, 21, 22, 23}, w=w, h=h)
    for t in (20, 22):        # the switches back: every slice predicts from the cache, no key packet
        assert not out[t]["key"] and all(s >= 0 for s in out[t]["slots"]), out[t]
        assert out[t]["bytes"] < 0.7 * out[10]["bytes"]
    assert out[-1]["valid"] == (1 if slots == 1 else 3)


def test_hevc_ltr_gpu_cbr_recode_reads_the_slot_again():
    """CBR at a bitrate that forces a re-code pass: the passes reuse the decision and read the slot
    again, the slot copy happens after the last pass."""
    run = Run(2, rate_control="cbr", bitrate_kbps=CBR_KBPS)
    out = _decode_all_needed(run, SPEC, {20, 21})
    assert not out[20]["key"] and all(s >= 0 for s in out[20]["slots"])
    assert out[20]["redos"] > out[19]["redos"], "frame 20 took no re-code pass"
    assert run.gpu.rc_stats()["redos"] == run.cpu.rc_stats()["redos"]


def test_hevc_ltr_gpu_mixed_picture():
    c = contents()
    run = Run(2)
    for _, _, f in sequence("A10 B10"):
        run.step(f)
    mixed = c["B"].copy()
    mixed[:64] = c["A"][:64]
    p = run.step(mixed, decode=True)
    s = ltr_slots_of_tasks(run.gpu)
    assert not p.key and s[0] >= 0 and s[1] >= 0 and s[2] < 0 and s[3] < 0, s
    for _ in range(2):
        assert not run.step(c["B"], decode=True).key


def test_hevc_ltr_gpu_expiry(monkeypatch):
    monkeypatch.setenv("SK_HEVC_LTR_MAX_AGE", "40")
    run = Run(2)
    out = _decode_all_needed(run, "A10 B60 A2", {70, 71})
    assert out[48]["valid"] == 1 and out[49]["valid"] == 0
    assert not out[70]["key"] and all(s < 0 for s in out[70]["slots"])


def test_hevc_ltr_gpu_keyframe_request_empties_the_cache():
    def hook(t, run):
        if t == 15:
            run.cpu.request_keyframe()
            run.gpu.request_keyframe()
    run = Run(2)
    out = _decode_all_needed(run, "A10 B10 A2", {20, 21}, hook)
    assert out[15]["key"] and out[14]["valid"] == 1 and out[15]["valid"] == 0
    assert not out[20]["key"] and all(s < 0 for s in out[20]["slots"])


def test_hevc_ltr_gpu_state_export_import():
    frames = [f for _, _, f in sequence(SPEC)]
    cpu, a = _pair(2)
    for t, f in enumerate(frames[:20]):
        a.encode(f, t)
    state = a.export_state()
    b = hevc_enc(2, backend="hip")
    b.import_state(state)
    cpu.import_state(state)
    for t, f in enumerate(frames[20:], 20):
        pa, pb, pc = a.encode(f, t), b.encode(f, t), cpu.encode(f, t)
        assert [(p.key, p.data) for p in pa] == [(p.key, p.data) for p in pb] == [(p.key, p.data) for p in pc]
        assert not any(p.key for p in pb)
        _same(cpu, b, 2, t)
    assert ltr_valid(b) == 3
