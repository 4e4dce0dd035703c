"""H.264 long-term reference cache on the HIP backend (k_ltr_match / k_ltr_decide, the per-slice
reference-1 planes, the slot copy in k_commit, the LtrState commit in k_plan): byte for byte against
the CPU reference encoder on a window-switch sequence: packets, reference planes, the cache's
state, per-slice decisions and slot planes. The packets are decoded too (marking and DPB bound
checked by the test decoder)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import H264Encoder, LTR_STATE_DTYPE, ME_DTYPE
from tests.h264_util import StripeDecoder
from tests.ltr_util import H, STRIPE, W, sequence

pytestmark = pytest.mark.gpu

SPEC = "A10 B10 A2 B2"


def _pair(w, h, **kw):
    kw = dict(dict(stripe_height=STRIPE, qp=24, use_paint_over=False), **kw)
    return H264Encoder(w, h, backend="cpu", **kw), H264Encoder(w, h, backend="hip", **kw)


def _same(cpu, gpu, slots, t):
    for name in ("ref_y", "ref_u", "ref_v", "ltr_state", "ltr_task") + tuple(f"ltr{j}_y" for j in range(slots)):
        a, b = cpu.debug_buffer(name), gpu.debug_buffer(name)
        assert np.array_equal(a, b), f"frame {t}: {name} differs ({np.sum(a != b)} bytes)"


def _step(cpu, gpu, sd, slots, f, t):
    pc, pg = cpu.encode(f, t), gpu.encode(f, t)
    assert [(p.y, p.key, p.data) for p in pg] == [(p.y, p.key, p.data) for p in pc], f"frame {t}: packets differ"
    _same(cpu, gpu, slots, t)
    for p in pg:
        sd.feed(p.data)
    return pg


def _run(w, h, slots, spec=SPEC, **kw):
    cpu, gpu = _pair(w, h, ltr_slots=slots, **kw)
    sd = StripeDecoder(w, h)
    out = []
    for t, (name, k, f) in enumerate(sequence(spec, w, h)):
        pg = _step(cpu, gpu, sd, slots, f, t)
        out.append((pg, int((gpu.debug_buffer("me", ME_DTYPE)["ref"] == 1).sum())))
    return cpu, gpu, out


@pytest.mark.parametrize("slots", [1, 3])
@pytest.mark.parametrize("fullframe", [False, True])
def test_ltr_gpu_matches_cpu(fullframe, slots):
    cpu, gpu, out = _run(W, H, slots, fullframe=fullframe)
    nmb = 13 * 7
    for t in (20, 22):   # the switches back: predicted from the cache, no key packet
        assert not any(p.key for p in out[t][0]) and 2 * out[t][1] >= nmb
    st = gpu.debug_buffer("ltr_state", LTR_STATE_DTYPE)
    assert np.all((st["valid"][-1:] if fullframe else st["valid"][:-1]) != 0)


def test_ltr_gpu_deblocking_across_references():
    """qp 36: automatic deblocking filters across MBs coded from different references (bS 1)."""
    _run(W, H, 2, qp=36, fullframe=False)
    _run(W, H, 2, qp=36, fullframe=True)


def test_ltr_gpu_split_intra_slice_carries_the_marking():
    """656 x 48, one 48-row stripe: 41 MBs per row exceed kIntraSubMbs, so the first switch (a scene
    cut that also stores A) is a split non-IDR I slice whose every sub-slice NAL carries the MMCOs;
    the decoder raises if they disagree."""
    w, h = 656, 48
    cpu, gpu, out = _run(w, h, 2, stripe_height=48, fullframe=False)
    nals = [n for n in out[10][0][0].data[10:].split(b"\x00\x00\x00\x01") if n]
    assert len(nals) == 4 and all(n[0] == 0x41 for n in nals) and not out[10][0][0].key
    assert 2 * out[20][1] >= 41 * 3


def test_ltr_gpu_state_export_import():
    frames = [f for _, _, f in sequence(SPEC)]
    cpu, a = _pair(W, H, ltr_slots=2)
    for t, f in enumerate(frames[:20]):
        a.encode(f, t)
        cpu.encode(f, t)
    state = a.export_state()
    b = H264Encoder(W, H, backend="hip", stripe_height=STRIPE, qp=24, use_paint_over=False, ltr_slots=2)
    b.import_state(state)
    for t, f in enumerate(frames[20:], 20):
        pa, pb, pc = a.encode(f, t), b.encode(f, t), cpu.encode(f, t)
        assert [(p.y, p.key, p.data) for p in pa] == [(p.y, p.key, p.data) for p in pb] == \
               [(p.y, p.key, p.data) for p in pc]
        assert not any(p.key for p in pb)
        _same(cpu, b, 2, t)
