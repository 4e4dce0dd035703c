"""Session dynamics with frames in flight, every codec, HIP back end against the CPU reference.

Production keeps two frames in flight (upload / launch / finish, per-parity slots and graphs, the
key / QP / rate snapshot taken at launch, overlay placement copied ahead of the graph) while the
session changes under way: key-frame requests, set_qp, set_rate (graphs re-captured with / without
the CBR guard), input kind and stride changes (recapture and dropped upload buffers), damage-driven
uploads, a state export for a live move. tests/dynamics_util.py drives one scripted run through any
codec, back end and pacing; the CPU back end run serially defines what is right, once per run
(`reference`), and everything is compared by exact equality.

Cases (208 x 112: 13 x 7 units, the last stripe one unit row; stripe_height 32):
  a  control script: key request at 3, set_qp(36) at 5, set_rate("cbr") at 8, set_rate("crf") at 12,
     set_qp(20) at 14; plain, with ltr_slots=2, H.264 also with num_refs=2
  b  overlays on HEVC and AV1: image at 0, moved at 2 and 3, disabled at 5, second image at 7
  c  input kind and stride: I420 at 5..8, NV12 at 9..11, padded BGRx rows from 12, plain from 15;
     also at 200 x 120 (a last unit column 8 wide, a last unit row 8 high)
  d  damage rows on every upload from frame 1 on HEVC and AV1, two frames uploaded and replaced
  e  state export with frame 8 in flight, continued by a fresh HIP and a fresh CPU encoder
  f  one session per codec from one thread, created with shared_copy
  g  call-order errors raise and change nothing
  h  an encoder closed with a frame in flight

Frames: "A10 B3 A3 C2 B2" where the case needs the long-term cache or the CBR guard (a window has
to stay for kLtrSettle = 8 quiet frames before it is cached, and the cut to B falls into the CBR
stretch), else the 16 frames of "A4 B4 A3 C2 B3".

CBR rate of the control script, chosen on the CPU back end so that the guard codes a frame again
inside the stretch (rc_stats()["redos"] after frame 11; set_rate() to another mode starts the
statistics again, so the figure is read there and not at the end of the run):
  H.264 stripes 300 kbit/s: 1    H.264 full frame 300 kbit/s: 1    HEVC 300 kbit/s: 1
  AV1 100 kbit/s: 1 (none at 200 .. 500 kbit/s: its 120 ms buffer takes the cut)
"""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import convert_bgrx
from tests import dynamics_util as du
from tests import extremes_util as xu

W, H = 208, 112
LONG, SHORT = "A10 B3 A3 C2 B2", "A4 B4 A3 C2 B3"
BASE = dict(stripe_height=32, use_paint_over=False)
VARIANTS = {"h264": ("h264", {}), "h264ff": ("h264", dict(fullframe=True)), "hevc": ("hevc", {}), "av1": ("av1", {})}
CBR_KBPS = dict(h264=300, hevc=300, av1=100)
KEY_AT, QP_AT, CBR_AT, CRF_AT, CUT = 3, 5, 8, 12, 9
SWITCH_BACK = 13   # the first frame of "A3" in LONG


def control(codec):
    return ((KEY_AT, "key", ()), (QP_AT, "qp", (36,)), (CBR_AT, "rate", ("cbr", CBR_KBPS[codec])),
            (CRF_AT, "rate", ("crf", 0)), (14, "qp", (20,)))


OVERLAYS = ((0, "overlay_image", (0, 1, 24, 40)), (0, "overlay_pos", (0, 20, 10, 1)), (2, "overlay_pos", (0, 90, 60, 1)),
            (3, "overlay_pos", (0, 190, 100, 1)),   # clipped at the right and the lower edge
            (5, "overlay_pos", (0, 190, 100, 0)), (7, "overlay_image", (0, 2, 30, 70)), (7, "overlay_pos", (0, 10, 5, 1)))
INPUTS = ((5, "input", ("i420",)), (9, "input", ("nv12",)), (12, "input", ("bgrx_padded",)), (15, "input", ("bgrx",)))
DAMAGE = tuple((t, "rows", ()) for t in range(1, 16)) + ((2, "replaced", ()), (5, "replaced", ()))


def _run(v, spec, script, w=W, h=H, **kw):
    codec, opts = VARIANTS[v]
    return du.run(codec, w, h, spec, script, **dict(BASE, **opts), **kw)


CASES = {}
for v, (codec, _) in VARIANTS.items():
    CASES[f"a-{v}"] = _run(v, LONG, control(codec))
    CASES[f"a-{v}-ltr"] = _run(v, LONG, control(codec), ltr_slots=2)
    if codec == "h264":
        CASES[f"a-{v}-refs2"] = _run(v, LONG, control(codec), num_refs=2)
    CASES[f"c-{v}"] = _run(v, SHORT, INPUTS)
    CASES[f"c-{v}-200x120"] = _run(v, SHORT, INPUTS, 200, 120)
    CASES[f"e-{v}"] = _run(v, LONG, control(codec) + ((CUT, "handover", ()),), ltr_slots=2)
    CASES[f"f-{v}"] = _run(v, LONG, control(codec), shared_copy=True)
for v in ("hevc", "av1"):
    CASES[f"b-{v}"] = _run(v, SHORT, OVERLAYS)
    CASES[f"d-{v}"] = _run(v, SHORT, DAMAGE)
HIP_CASES = [n for n in CASES if n[0] in "abcd"]
HANDOVER = [n for n in CASES if n[0] == "e"]
SHARED = [n for n in CASES if n[0] == "f"]


def _plain(r):
    """The CPU reference of the run without its handover: the uninterrupted stream."""
    return du.reference(du.without(r, "handover"))


def _skip_without_decoder(name):
    if "av1" in name and not dav1d.available():
        pytest.skip("dav1d (Pillow libavif) not available")


# ---- CPU tier ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pacing", ["overlapped", "two"])
@pytest.mark.parametrize("name", list(CASES))
def test_cpu_pacing_equals_serial(name, pacing):
    """The queued default submit() / finish() of encoder_iface.h: the CPU back end gives the same
    packets through upload / launch / finish as serially; a handover gives the uninterrupted stream."""
    r = CASES[name]
    ref = _plain(r)
    got = du.drive(r, "cpu", pacing)
    if name in HANDOVER:
        heir = got["heirs"]["cpu"]
        du.assert_packets_equal(got["packets"], ref["packets"][:CUT], f"{name} {pacing} donor")
        du.assert_packets_equal(heir["packets"], ref["packets"][CUT:], f"{name} {pacing} heir", CUT)
        du.assert_end_state_equal(heir, ref, f"{name} {pacing} heir")
    else:
        du.assert_packets_equal(got["packets"], ref["packets"], f"{name} {pacing}")
        du.assert_end_state_equal(got, ref, f"{name} {pacing}")


@pytest.mark.parametrize("name", HANDOVER)
def test_cpu_handover_serial_equals_uninterrupted(name):
    r = CASES[name]
    got, ref = du.reference(r), _plain(r)
    du.assert_packets_equal(got["packets"], ref["packets"][:CUT], f"{name} donor")
    du.assert_packets_equal(got["heirs"]["cpu"]["packets"], ref["packets"][CUT:], f"{name} heir", CUT)


@pytest.mark.parametrize("name", [n for n in CASES if n not in HANDOVER])
def test_reference_decodes(name):
    """The independent decoder returns the reference's reconstruction of every frame (the handover
    cases are the streams of a-*-ltr)."""
    _skip_without_decoder(name)
    r = CASES[name]
    xu.assert_decodes(r, du.reference(r)["snaps"], f"{name}: CPU")


def _coded_qps(snap):
    return snap["tasks"]["qp"][snap["tasks"]["final_action"] != 0]


@pytest.mark.parametrize("name", list(CASES))
def test_reference_reaches_its_case(name):
    """Asserted on the CPU reference, so that a case cannot quietly stop exercising its path."""
    r = CASES[name]
    ref = _plain(r)
    snaps, opts = ref["snaps"], dict(r[4])
    assert all(len(s["packets"]) > 0 for s in snaps), "a frame without packets carries no frame id"
    if name[0] in "aef":
        assert all(p[2] for p in snaps[KEY_AT]["packets"]) and not any(p[2] for p in snaps[KEY_AT - 1]["packets"])
        # the QP change shows in the frame it was made before, not one later
        assert set(_coded_qps(snaps[QP_AT - 1]).tolist()) == {25} and set(_coded_qps(snaps[QP_AT]).tolist()) == {36}
        if r[0] == "h264":   # deblock "auto": slice QPs on both sides of 34, post and post_short in one run
            assert "deblock" not in opts
            qps = np.concatenate([_coded_qps(s) for s in snaps])
            assert qps.min() < 34 <= qps.max(), (int(qps.min()), int(qps.max()))
            lo = [t for t, s in enumerate(snaps) if _coded_qps(s).max() < 34]
            assert lo and min(lo) < CBR_AT and max(lo) > CRF_AT, lo   # post_short before and after the long graph
        assert [s["rc"]["mode"] for s in snaps[CBR_AT - 1:CRF_AT + 1]] == [0, 2, 2, 2, 2, 1]
        assert snaps[CRF_AT - 1]["rc"]["redos"] >= 1, snaps[CRF_AT - 1]["rc"]
        assert snaps[0]["rc"]["mode"] == 0 and ref["stats"]["mode"] == 1   # ends in another mode than it began in
        if opts.get("ltr_slots"):
            assert max(snaps[SWITCH_BACK]["ltr_slot"]) >= 0, [s["ltr_slot"] for s in snaps]
    if name[0] == "b":   # the overlay changes what is coded: every event frame differs from the run without it
        bare = du.reference(du.run(r[0], r[1], r[2], r[3], (), **opts))
        for t in (0, 2, 3, 5, 7):
            assert snaps[t]["packets"] != bare["snaps"][t]["packets"], f"frame {t}: the overlay event changed nothing"
    if name[0] == "c":   # planar and BGRx frames alternate, each switch on a coded frame
        assert all((s["tasks"]["final_action"] != 0).any() for s in snaps)
    if name[0] == "d":
        n = r[2]
        partial = [t for t, rows in ref["rows"].items() if rows is not None and len(rows) < n]
        assert 2 * len(partial) >= len(snaps), (partial, len(snaps))
        assert any(rows is not None and len(rows) == n for rows in ref["rows"].values())   # and a full one (a cut)


def _refused(s, t, f):
    """encode() and encode_yuv() of frame t while an earlier frame is uncollected: both raise. One that
    goes through instead has to return frame t at least (the frame-id check), which it cannot:
    finish() hands out the oldest frame in flight."""
    fid = du.FIRST_ID + t
    for name, call in (("encode()", lambda: s.enc.encode(f, fid)),
                       ("encode_yuv()", lambda: s.enc.encode_yuv("i420", *convert_bgrx(f, "i420"), frame_id=fid))):
        try:
            packets = call()
        except RuntimeError as e:
            assert f"{name}: a frame is in flight" in str(e), str(e)
            continue
        du.check_frame_id(packets, t)
        pytest.fail(f"{name} of frame {t} with {list(s.pending)} in flight was not refused")


@pytest.mark.parametrize("v", list(VARIANTS))
def test_cpu_call_order_errors(v):
    """encode() and encode_yuv() with a submitted frame uncollected, and finish() with nothing
    submitted, raise and change nothing on the CPU back end: the stream continues as the reference."""
    r = CASES[f"a-{v}"]
    ref = du.reference(r)
    frames = du.frames_of(r[3], r[1], r[2])
    s = du.Session(r, "cpu", "two")
    with pytest.raises(RuntimeError, match="finish\\(\\) without"):
        s.enc.finish()
    for t, f in enumerate(frames):
        for tt, ev, args in r[5]:
            if tt == t:
                du.apply_event(s.enc, s.st, ev, args)
        if t in (4, 10):   # frame t - 1 is queued
            assert list(s.pending) == [t - 1]
            _refused(s, t, f)
        s.hand_over(t, f)
    res = {}
    s.close(res)
    du.assert_packets_equal([s.packets[t] for t in range(len(frames))], ref["packets"], f"cpu {v}")
    du.assert_end_state_equal(res, ref, f"cpu {v}")


def test_cpu_several_sessions_from_one_thread():
    runs = [CASES[n] for n in SHARED]
    for r, got in zip(runs, du.drive_many(runs, "cpu")):
        du.assert_packets_equal(got, du.reference(r)["packets"], f"cpu {r[0]} {dict(r[4])}")


# ---- GPU tier ------------------------------------------------------------------------------------
def _assert_serial_same(r, got, ref, who):
    """Per frame: extremes_util.assert_same, the whole SliceTask array and the controller's state."""
    for t, (g, c) in enumerate(zip(got["snaps"], ref["snaps"])):
        xu.assert_same(r, t, g, c)
        assert du.rc_state(g["rc"]) == du.rc_state(c["rc"]), f"{who} frame {t}: rc_stats {g['rc']} against {c['rc']}"
        if "ltr_slot" in c:
            assert g["ltr_slot"] == c["ltr_slot"], f"{who} frame {t}: cache decisions {g['ltr_slot']} against {c['ltr_slot']}"


@pytest.mark.gpu
@pytest.mark.parametrize("pacing", du.PACINGS)
@pytest.mark.parametrize("name", HIP_CASES)
def test_hip_matches_cpu(name, pacing):
    """Cases a to d: the HIP back end in every pacing against the cached CPU serial run: every packet
    (with its frame id), and after the last finish() the reference picture and rc_stats()."""
    xu.need_gpu()
    r = CASES[name]
    ref = du.reference(r)
    got = du.drive(r, "hip", pacing)
    who = f"{name} {pacing}"
    if pacing == "serial":
        _assert_serial_same(r, got, ref, who)
    du.assert_packets_equal(got["packets"], ref["packets"], who)
    du.assert_end_state_equal(got, ref, who)


@pytest.mark.gpu
@pytest.mark.parametrize("pacing", du.PACINGS)
@pytest.mark.parametrize("name", HANDOVER)
def test_hip_handover_with_a_frame_in_flight(name, pacing):
    """Case e: export_state() after launch(8) and before finish(8). The donor's frame 8, and frames
    9.. of a fresh HIP and a fresh CPU encoder that imported the blob, equal the uninterrupted run."""
    xu.need_gpu()
    r = CASES[name]
    ref = _plain(r)
    got = du.drive(r, "hip", pacing, heirs=("hip", "cpu"), want_snaps=False)
    du.assert_packets_equal(got["packets"], ref["packets"][:CUT], f"{name} {pacing} donor")
    for b, heir in got["heirs"].items():
        du.assert_packets_equal(heir["packets"], ref["packets"][CUT:], f"{name} {pacing} heir on {b}", CUT)
        du.assert_end_state_equal(heir, ref, f"{name} {pacing} heir on {b}")


@pytest.mark.gpu
def test_hip_several_sessions_from_one_thread():
    """Case f: one encoder per codec with shared_copy (the device's one copy stream, as
    parallel/multi.py creates them); per frame upload + launch on each, then finish on each."""
    xu.need_gpu()
    runs = [CASES[n] for n in SHARED]
    for r, got in zip(runs, du.drive_many(runs, "hip")):
        du.assert_packets_equal(got, du.reference(r)["packets"], f"hip {r[0]} {dict(r[4])}")


@pytest.mark.gpu
@pytest.mark.parametrize("v", list(VARIANTS))
def test_hip_call_order_errors(v):
    """Case g: launch() with nothing staged, finish() with nothing launched, encode() / encode_yuv()
    with one and with two frames uncollected, a third upload() and a launch() with two frames in
    flight: each raises and changes nothing, the stream continues as the reference."""
    xu.need_gpu()
    r = CASES[f"a-{v}"]
    ref = du.reference(r)
    frames = du.frames_of(r[3], r[1], r[2])
    s = du.Session(r, "hip", "two")
    enc = s.enc

    with pytest.raises(RuntimeError, match="launch\\(\\) needs"):
        enc.launch()
    with pytest.raises(RuntimeError, match="finish\\(\\) without"):
        enc.finish()
    for t, f in enumerate(frames):
        for tt, ev, args in r[5]:
            if tt == t:
                du.apply_event(enc, s.st, ev, args)
        if t in (4, CBR_AT + 2):   # frame t - 1 is in flight
            assert list(s.pending) == [t - 1]
            _refused(s, t, f)
        if t in (6, CBR_AT + 1):   # frames t - 1 and t in flight
            enc.upload(f, du.FIRST_ID + t)
            enc.launch()
            s.pending.append(t)
            s.st["prev"] = f
            nxt = frames[t + 1]
            with pytest.raises(RuntimeError, match="two frames in flight"):
                enc.upload(nxt, du.FIRST_ID + t + 1)
            with pytest.raises(RuntimeError, match="launch\\(\\) needs"):
                enc.launch()
            _refused(s, t + 1, nxt)
            s.collect()
            continue
        s.hand_over(t, f)
    res = {}
    s.close(res)
    du.assert_packets_equal([s.packets[t] for t in range(len(frames))], ref["packets"], f"hip {v}")
    du.assert_end_state_equal(res, ref, f"hip {v}")


@pytest.mark.gpu
@pytest.mark.parametrize("v", list(VARIANTS))
def test_hip_close_with_a_frame_in_flight(v):
    """Case h: an encoder closed with one frame launched and uncollected and the next one uploaded
    (the destructor waits for its streams before it frees what they use); a new encoder on the same
    device then codes the whole sequence as the reference."""
    xu.need_gpu()
    r = CASES[f"a-{v}"]
    frames = du.frames_of(r[3], r[1], r[2])
    enc = du.encoder(r, "hip")
    enc.upload(frames[0], du.FIRST_ID)
    enc.launch()
    enc.upload(frames[1], du.FIRST_ID + 1)
    enc.close()
    ref = du.reference(r)
    got = du.drive(r, "hip", "two")
    du.assert_packets_equal(got["packets"], ref["packets"], f"after close {v}")
    du.assert_end_state_equal(got, ref, f"after close {v}")
