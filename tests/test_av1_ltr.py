"""AV1 long-term reference cache on the CPU back end (csrc/codec/ltr.h buffer map, av1_cpu.cpp): a
cached picture is a decoder buffer that later frame headers leave alone, a matched tile row
predicts from it as LAST2. Every picture goes through dav1d and must equal the encoder's
reconstruction; every inter frame header's reference buffers must equal an independent replay of
the buffer model (tests/av1_ltr_util.py)."""
import ctypes
import threading

import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import PinnedBuffer
from tests.av1_ltr_util import (H, STRIPE, W, CheckedAv1, av1_enc, blk_refs, contents, ltr_slots_of_tasks, ltr_valid,
                                parse_refs, run_spec, sequence)

pytestmark = pytest.mark.skipif(not dav1d.available(), reason="dav1d (Pillow's libavif) not found")

SPEC = "A10 B10 A2 B2"

_runs = {}


def _run(spec, slots, w=W, h=H, stripe=STRIPE):
    """Each checked run once; the tests share the results and leave them unchanged."""
    k = (spec, slots, w, h, stripe)
    if k not in _runs:
        _runs[k] = run_spec(spec, slots, w, h, caret=w > 64, stripe_height=stripe)
    return _runs[k]


def _switch_checks(out, slots):
    for t in (20, 22):        # the switches back: every tile row predicts from the cache, no key frame
        assert not out[t]["key"] and all(s >= 0 for s in out[t]["slots"]), out[t]["slots"]
    assert out[20]["bytes"] < 0.7 * out[10]["bytes"], (out[20]["bytes"], out[10]["bytes"])
    assert out[-1]["valid"] == (1 if slots == 1 else 3)


@pytest.mark.parametrize("slots", [1, 2])
def test_av1_ltr_switch_sequence(slots):
    """208x112, stripe 32: 4 x 2 tiles of 64x64, two slices per tile row, the last slice one MB row."""
    out = _run(SPEC, slots)
    assert [o["key"] for o in out] == [True] + [False] * (len(out) - 1)
    _switch_checks(out, slots)
    off = _run(SPEC, 0)
    print(f"frame 20: {out[20]['bytes']} bytes with the cache, {off[20]['bytes']} without, frame 10: {out[10]['bytes']}")
    assert out[20]["bytes"] < off[20]["bytes"]


@pytest.mark.parametrize("w,h,stripe", [(264, 136, 64), (64, 64, 32)])
def test_av1_ltr_other_shapes(w, h, stripe):
    """5 x 3 one-superblock tiles with partial right and bottom ones; one tile (no neighbour
    outside the block's own tile: the no-neighbour reference contexts; without the caret, which
    covers too much of this picture for a quiet frame)."""
    _switch_checks(_run(SPEC, 2, w, h, stripe), 2)


def test_av1_ltr_mixed_picture():
    c = contents()
    run = CheckedAv1(av1_enc(2))
    for _, _, f in sequence("A10 B10"):
        run.step(f)
    mixed = c["B"].copy()
    mixed[:64] = c["A"][:64]
    o = run.step(mixed)
    assert not o["key"] and o["slots"][0] >= 0 and o["slots"][1] >= 0 and o["slots"][2] < 0 and o["slots"][3] < 0, o["slots"]
    refs = blk_refs(run.enc, W, H)
    assert (refs[:8] == 1).all() and (refs[8:] == 0).all()    # tile row 0: LAST2, tile row 1: LAST
    for _ in range(2):
        assert not run.step(mixed)["key"]


def test_av1_ltr_two_matched_slots_use_one():
    """A, B and C cached and C on screen; a frame with A on top and B below matches two slots. The
    frame reads the one matched by more units (the top tile row: 4 of 7 MB rows), the other row
    falls back to LAST."""
    c = contents()
    run = CheckedAv1(av1_enc(3))
    for _, _, f in sequence("A10 B10 C10 A10 C10"):
        o = run.step(f)
    assert o["valid"] == 7
    mixed = c["B"].copy()
    mixed[:64] = c["A"][:64]
    o = run.step(mixed)
    assert not o["key"] and o["slots"] == [0, 0, -1, -1], o["slots"]
    assert ltr_slots_of_tasks(run.enc) == [0, 0, -1, -1]
    run.step(mixed)


def test_av1_ltr_headers_follow_the_buffer_model():
    """CheckedAv1.step compares every header with the replayed model; here: what the model did."""
    out = _run(SPEC, 2)
    stores = [t for t, o in enumerate(out) if not o["key"] and o["store"] >= 0]
    assert stores == [10, 20], stores
    assert out[9]["refs"]["refresh"] == 1 and out[10]["refs"]["refresh"] == 2 and out[20]["refs"]["refresh"] == 4
    assert out[20]["refs"]["idx"][:2] == [1, 0]      # LAST: B in buffer 1, LAST2: A in buffer 0
    assert out[22]["refs"]["idx"][:2] == [2, 1] and out[22]["refs"]["refresh"] == 4   # no store: in place
    one = _run("A10 B10 C10 A2", 1)
    # one slot: the evicted slot's buffer is free again and the next picture reuses it
    assert [one[t]["refs"]["refresh"] for t in (10, 20, 30)] == [2, 1, 2]
    assert {o["refs"]["refresh"] for o in one if not o["key"]} == {1, 2}


def test_av1_ltr_keyframe_request_empties_the_cache():
    def hook(t, enc):
        if t == 15:
            enc.request_keyframe()
    out = run_spec("A10 B10 A2", 2, hook=hook)
    assert out[15]["key"] and out[14]["valid"] == 1 and out[15]["valid"] == 0
    assert not out[20]["key"] and all(s < 0 for s in out[20]["slots"])


def test_av1_ltr_one_slot_is_evicted_and_reused():
    out = _run("A10 B10 C10 A2", 1)
    assert [out[t]["store"] for t in (10, 20, 30)] == [0, 0, 0]
    assert not any(o["key"] for o in out[1:]) and out[-1]["valid"] == 1


def test_av1_ltr_off_is_the_default():
    frames = [f for _, _, f in sequence("A3 B3")]
    a, b = av1_enc(0), av1_enc(None)
    for t, f in enumerate(frames):
        assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)]


def test_av1_ltr_validation():
    with pytest.raises(RuntimeError, match="eight reference buffers"):
        av1_enc(8)
    with pytest.raises(RuntimeError, match="tile height"):
        av1_enc(1, 200, 120, stripe_height=48)
    run = CheckedAv1(av1_enc(1, 200, 120, stripe_height=64), 200, 120)
    for _, _, f in sequence("A2 B1", 200, 120):
        run.step(f)


def test_av1_ltr_state_export_import():
    frames = [f for _, _, f in sequence(SPEC)]
    a = CheckedAv1(av1_enc(2))
    for f in frames[:20]:
        a.step(f)
    state = a.enc.export_state()
    b = av1_enc(2)
    b.import_state(state)
    for t, f in enumerate(frames[20:], 20):
        pb = b.encode(f, t)
        o = a.step(f)                       # decoded and checked against the buffer model
        assert [bytes(p.data) for p in pb] == [o["data"]] and not o["key"]
        assert np.array_equal(b.debug_buffer("ltr_state"), a.enc.debug_buffer("ltr_state"))
    assert ltr_valid(b) == 3


def test_av1_ltr_capture_session():
    """pixelflux capture session (CPU backend, AV1) over a frame pool that switches A -> B -> A."""
    import pixelflux
    frames = [f for _, _, f in sequence("A10 B10 A2")]
    pool = PinnedBuffer((len(frames), H, W, 4))
    for i, f in enumerate(frames):
        pool.array[i] = f
    got = []
    lock = threading.Lock()

    def on_frame(res, n, user):
        with lock:
            got.append([ctypes.string_at(res[i].data, res[i].size) for i in range(n)])

    s = pixelflux.default_settings(W, H, use_cpu=1, source=pixelflux.SOURCE_POOL, step_mode=1, pool_frames=len(frames),
                                   pool_stride=W * 4, stripe_height=STRIPE, use_paint_over_quality=0, h264_crf=24,
                                   h264_rc_mode=0, h264_ltr_slots=2, output_mode=3)
    s.pool = pool.array.ctypes.data
    cap = pixelflux.ScreenCapture()
    cb = pixelflux.FrameCallback(on_frame)
    cap.start_frame_capture(s, cb)
    cap.run(len(frames))
    assert cap.wait(120_000) == 0
    cap.close()
    assert len(got) == len(frames) and all(len(fr) == 1 for fr in got)
    dec = dav1d.Decoder()
    for fr in got:
        assert dec.decode(fr[0][10:]) is not None
    r = parse_refs(got[20][0][10:])
    assert not r["key"] and r["idx"][1] != r["idx"][0]          # the switch back reads a cached buffer
    assert len(got[20][0]) < 0.7 * len(got[10][0])


def test_server_reads_the_av1_variable_for_av1_only(monkeypatch):
    from selkies_gstreamer_amd.server.data_server import _ltr_slots_from_env
    monkeypatch.delenv("SELKIES_H264_LTR_SLOTS", raising=False)
    monkeypatch.delenv("SELKIES_HEVC_LTR_SLOTS", raising=False)
    monkeypatch.setenv("SELKIES_AV1_LTR_SLOTS", "11")
    assert _ltr_slots_from_env("SELKIES_AV1_LTR_SLOTS") == 7
    assert _ltr_slots_from_env() == 0 and _ltr_slots_from_env("SELKIES_HEVC_LTR_SLOTS") == 0
    monkeypatch.setenv("SELKIES_AV1_LTR_SLOTS", "x")
    assert _ltr_slots_from_env("SELKIES_AV1_LTR_SLOTS") == 0
