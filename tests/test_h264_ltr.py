"""H.264 long-term reference cache (csrc/codec/ltr.h, EncoderConfig::ltr_slots), CPU reference encoder.

Window-switch content on 208 x 112 with 32-pixel stripes (13 x 7 MBs, four stripes, the last of one
MB row): three "windows" A, B, C that differ in every macroblock and a caret that blinks every
frame. Every packet of every frame is decoded with the independent decoder, whose reference
marking (models/h264/decoder.py RefMarking) raises on any MMCO / list modification that names a
missing picture and on a DPB over max_num_ref_frames, and the decoded picture must equal the
encoder's reference planes. Switching back to a window seen before must predict from the cached
picture: no key packet, at least half the MBs from reference 1 and under 0.7x the bytes the same
frame costs without the cache (measured: profiles/ltr_switch.md).
"""
import ctypes
import threading

import numpy as np
import pytest

from selkies_gstreamer_amd.models.h264.decoder import BitReader, H264Decoder, parse_sps, split_annexb, unescape
from selkies_gstreamer_amd.ops.native import H264Encoder, LTR_STATE_DTYPE, RC_FIELDS, PinnedBuffer
from tests.ltr_util import H, STRIPE, W, Checked, sequence

SPEC = "A10 B10 A3 B3 C10 A3"
NMB = 13 * 7
# Table A-1 MaxDpbMbs
MAX_DPB_MBS = {10: 396, 9: 396, 11: 900, 12: 2376, 13: 2376, 20: 2376, 21: 4752, 22: 8100, 30: 8100, 31: 18000,
               32: 20480, 40: 32768, 41: 32768, 42: 34816, 50: 110400, 51: 184320, 52: 184320}


def _enc(fullframe, slots, **kw):
    return H264Encoder(W, H, stripe_height=STRIPE, fullframe=fullframe, qp=24, use_paint_over=False, backend="cpu",
                       ltr_slots=slots, **kw)


def _run(fullframe, slots, spec=SPEC, **kw):
    ck = Checked(_enc(fullframe, slots, **kw))
    return [(name, k, ck.step(f, src_psnr=True)) for name, k, f in sequence(spec)], ck


_baseline = {}


def _base(fullframe):
    """The same sequence without the cache (the parent behaviour), once per mode."""
    if fullframe not in _baseline:
        _baseline[fullframe] = _run(fullframe, 0)[0]
    return _baseline[fullframe]


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("fullframe", [False, True])
def test_switch_back_predicts_from_the_cache(fullframe, slots):
    out, ck = _run(fullframe, slots)          # every packet decoded, decoder == encoder reference (Checked.step)
    base = _base(fullframe)
    # frame 20: first A after B; frame 23: first B after A
    for t in (20, 23):
        r, b = out[t][2], base[t][2]
        assert out[t][1] == 0 and out[t][0] == base[t][0]
        assert not r["key"]
        assert 2 * r["ref1"] >= NMB, f"frame {t}: {r['ref1']} of {NMB} MBs from the cached picture"
        print(f"frame {t} fullframe={fullframe} slots={slots}: {r['bytes']} bytes (Y-PSNR {r['psnr']:.2f}) vs "
              f"{b['bytes']} bytes (Y-PSNR {b['psnr']:.2f}) without the cache, ratio {r['bytes'] / b['bytes']:.3f}")
        assert r["bytes"] < 0.7 * b["bytes"]
    # the first switch codes new content: in striped mode a non-IDR I picture, so the cache survives it
    assert not out[10][2]["key"]
    st = ck.enc.debug_buffer("ltr_state", LTR_STATE_DTYPE)
    streams = st[-1:] if fullframe else st[:-1]
    if slots == 1:
        # A after C: the only long-term index was occupied (by B) and now holds C; the switch decoded above
        assert all(int(s["valid"]) == 1 for s in streams)
        assert out[36][2]["ref1"] == 0
    else:
        # two slots still hold A after the C phase: the last switch predicts from it again
        assert all(int(s["valid"]) == 3 for s in streams)
        assert 2 * out[36][2]["ref1"] >= NMB and out[36][2]["bytes"] < 0.7 * base[36][2]["bytes"]


@pytest.mark.parametrize("fullframe,slots", [(False, 3), (True, 8)])
def test_sps_announces_the_dpb(fullframe, slots):
    pk = _enc(fullframe, slots).encode(next(sequence("A1"))[2], 0)
    for p in pk:
        assert p.key
        nal = [n for n in split_annexb(p.data[10:]) if n[0] & 31 == 7][0]
        _, sps = parse_sps(BitReader(unescape(nal[1:])))
        assert sps.max_num_ref_frames == 1 + slots
        assert sps.max_num_ref_frames * sps.mb_w * sps.mb_h <= MAX_DPB_MBS[sps.level_idc]
    # without the cache the parameter sets are the parent's
    nal = [n for n in split_annexb(_enc(fullframe, 0).encode(next(sequence("A1"))[2], 0)[0].data[10:]) if n[0] & 31 == 7][0]
    assert parse_sps(BitReader(unescape(nal[1:])))[1].max_num_ref_frames == 1


@pytest.mark.parametrize("fullframe", [False, True])
def test_requested_keyframe_empties_the_cache(fullframe):
    ck = Checked(_enc(fullframe, 2))
    res, valid = [], {}
    for t, (name, k, f) in enumerate(sequence("A10 B10 A3")):
        if t == 15:                       # in the middle of B, after A was stored
            ck.enc.request_keyframe()
        res.append(ck.step(f))
        st = ck.enc.debug_buffer("ltr_state", LTR_STATE_DTYPE)
        valid[t] = [int(v) for v in (st["valid"][-1:] if fullframe else st["valid"][:-1])]
    assert res[15]["key"]
    assert all(v == 1 for v in valid[14]) and not any(valid[15])   # A was cached; the IDR emptied the cache
    assert res[20]["ref1"] == 0 and not res[20]["key"]             # the switch back finds nothing, and decodes


def test_ltr_with_two_sliding_references_is_refused():
    with pytest.raises(RuntimeError, match="num_refs"):
        _enc(False, 2, num_refs=2)
    with pytest.raises(RuntimeError, match="ltr_slots"):
        _enc(False, 9)


@pytest.mark.parametrize("fullframe", [False, True])
def test_state_blob_carries_the_cache(fullframe):
    frames = [f for _, _, f in sequence("A10 B10 A3")]
    a = _enc(fullframe, 2)
    for t, f in enumerate(frames[:20]):
        a.encode(f, t)
    state = a.export_state()
    b = _enc(fullframe, 2)
    b.import_state(state)
    ra = [[(p.y, p.key, p.data) for p in a.encode(f, 20 + i)] for i, f in enumerate(frames[20:])]
    rb = [[(p.y, p.key, p.data) for p in b.encode(f, 20 + i)] for i, f in enumerate(frames[20:])]
    assert ra == rb and not any(key for fr in rb for _, key, _ in fr)
    # version 3 without the cache: the blob keeps its size (StateHeader 64, StripeState 44 per stripe + the
    # picture's, RcState, ref / ref1 / last source planes, MV field); version 4 appends LtrState[] (96 bytes
    # each) and the slot planes
    off = _enc(fullframe, 0)
    ns = 4
    planes = W * H * 3 // 2
    assert off.state_bytes() == 64 + 44 * (ns + 1) + 4 * len(RC_FIELDS) + 3 * planes + 4 * NMB == 105632
    assert int(off.export_state()[4:8].view(np.int32)[0]) == 3
    assert a.state_bytes() == off.state_bytes() + 96 * (ns + 1) + 2 * planes
    assert int(state[4:8].view(np.int32)[0]) == 4
    with pytest.raises(RuntimeError):
        off.import_state(np.resize(state, off.state_bytes()))


def test_capture_session_with_the_cache():
    """pixelflux capture session (CPU backend) over a frame pool that switches A -> B -> A."""
    import pixelflux
    frames = [f for _, _, f in sequence("A10 B10 A2")]
    pool = PinnedBuffer((len(frames), H, W, 4))
    for i, f in enumerate(frames):
        pool.array[i] = f
    got = []
    lock = threading.Lock()

    def on_frame(res, n, user):
        with lock:
            got.append([(res[i].stripe_y_start, ctypes.string_at(res[i].data, res[i].size)) for i in range(n)])

    s = pixelflux.default_settings(W, H, use_cpu=1, source=pixelflux.SOURCE_POOL, step_mode=1, pool_frames=len(frames),
                                   pool_stride=W * 4, stripe_height=STRIPE, use_paint_over_quality=0, h264_crf=24,
                                   h264_rc_mode=0, h264_ltr_slots=2)
    s.pool = pool.array.ctypes.data
    cap = pixelflux.ScreenCapture()
    cb = pixelflux.FrameCallback(on_frame)
    cap.start_frame_capture(s, cb)
    cap.run(len(frames))
    assert cap.wait(120_000) == 0
    cap.close()
    assert len(got) == len(frames)
    decs = {}
    for fr in got:
        for y, data in fr:
            if data[1] == 1:
                decs[y] = H264Decoder()
            assert len(decs[y].decode(data[10:])) == 1
    assert len(got[20]) == 4 and not any(data[1] for _, data in got[20])      # the switch back: no key packet
    assert sum(len(d) for _, d in got[20]) < 0.7 * sum(len(d) for _, d in got[10])
    assert all(len(d.marking.long) >= 1 for d in decs.values())               # the decoders hold long-term pictures
