"""HEVC long-term reference cache (csrc/codec/ltr.h exclusive mode, EncoderConfig::ltr_slots with
codec HEVC), CPU reference encoder.

Window-switch content on 208 x 112 with 32-pixel stripes: 13 x 7 units, so a partial CTB column and
row, and four slices, the last half a CTB row high. Every packet is decoded with the test decoder,
whose DPB (models/hevc/decoder.py) raises on an RPS entry that names a missing picture, on slices
of a picture that disagree, on a list entry out of range and on an RPS over
sps_max_dec_pic_buffering_minus1; the decoded picture must equal the encoder's reference planes.
Switching back to a window seen before must predict from the cached picture: no key packet, every
P slice matched to a slot, under 0.7x the bytes the frame costs without the cache (measured:
profiles/hevc_ltr_switch.md; no third-party decoder has seen these streams).
"""
import ctypes
import threading

import numpy as np
import pytest

from selkies_gstreamer_amd.models.hevc.decoder import HevcDecoder, split_annexb, unescape
from selkies_gstreamer_amd.ops.native import HevcEncoder, PinnedBuffer, RC_FIELDS
from tests.hevc_ltr_util import (H, STRIPE, W, CheckedHevc, contents, final_actions, hevc_enc, ltr_slots_of_tasks,
                                 ltr_valid, sequence)

SPEC = "A10 B10 A3 B3 C10 A3"
# Table A.8 MaxLumaPs per general_level_idc, and A.4.2 MaxDpbSize (maxDpbPicBuf 6)
MAX_LUMA_PS = {30: 36864, 60: 122880, 63: 245760, 90: 552960, 93: 983040, 120: 2228224, 123: 2228224,
               150: 8912896, 153: 8912896, 156: 8912896, 180: 35651584, 183: 35651584, 186: 35651584}


def max_dpb_size(ps, level_idc):
    m = MAX_LUMA_PS[level_idc]
    return 16 if 4 * ps <= m else 12 if 2 * ps <= m else 8 if 4 * ps <= 3 * m else 6


def _run(slots, spec=SPEC, hook=None, **kw):
    ck = CheckedHevc(hevc_enc(slots, **kw))
    out = []
    for t, (name, k, f) in enumerate(sequence(spec)):
        if hook:
            hook(t, ck.enc)
        r = ck.step(f)
        r.update(name=name, k=k, slots=ltr_slots_of_tasks(ck.enc) if slots else None, actions=final_actions(ck.enc),
                 valid=ltr_valid(ck.enc) if slots else 0)
        out.append(r)
    return out, ck


_cache = {}


def _shared(slots):
    """SPEC with `slots` slots (0: the parent behaviour), once per module."""
    if slots not in _cache:
        _cache[slots] = _run(slots)
    return _cache[slots]


@pytest.mark.parametrize("slots", [1, 2])
def test_switch_back_predicts_from_the_cache(slots):
    out, ck = _shared(slots)                  # every packet decoded, decoder == encoder reference (CheckedHevc.step)
    base, _ = _shared(0)
    for t in (20, 23):                        # first A after B, first B after A
        r, b = out[t], base[t]
        assert r["k"] == 0 and not r["key"]
        p = [s for s, a in zip(r["slots"], r["actions"]) if a == 1]
        assert len(p) == 4 and all(s >= 0 for s in p), f"frame {t}: slots {r['slots']}, actions {r['actions']}"
        print(f"frame {t} slots={slots}: {r['bytes']} bytes vs {b['bytes']} without the cache, "
              f"ratio {r['bytes'] / b['bytes']:.3f}")
        assert r["bytes"] < 0.7 * b["bytes"]
        # the decoder's list 0 of the last slice is one long-term picture
        assert r["list0"] is not None and r["list0"][0] in r["rps"]["lt_curr"]
    assert not out[10]["key"]
    if slots == 1:
        # frame 20 stored B into slot 0 while its slices predicted from the A it held; by frame 36 the
        # only slot holds B, then C: A is gone, nothing useful is found, and the picture decodes
        assert out[20]["valid"] == 1 and ltr_valid(ck.enc) == 1
        assert not out[36]["key"] and out[36]["bytes"] >= 0.7 * base[36]["bytes"]
    else:
        assert ltr_valid(ck.enc) == 3         # two slots still hold A after the C phase
        assert all(s >= 0 for s in out[36]["slots"]) and out[36]["bytes"] < 0.7 * base[36]["bytes"]
        print(f"frame 36 slots=2: ratio {out[36]['bytes'] / base[36]['bytes']:.3f}")


def test_mixed_picture_matches_per_slice():
    """After A10 B10 one frame whose rows 0..63 are A and the rest B: slices 0 and 1 predict from the
    cached A, slices 2 and 3 from the previous picture, in one picture with one RPS."""
    c = contents()
    ck = CheckedHevc(hevc_enc(2))
    for _, _, f in sequence("A10 B10"):
        ck.step(f)
    mixed = c["B"].copy()
    mixed[:64] = c["A"][:64]
    r = ck.step(mixed)
    assert not r["key"]
    s = ltr_slots_of_tasks(ck.enc)
    assert s[0] >= 0 and s[1] >= 0 and s[2] < 0 and s[3] < 0, s
    assert final_actions(ck.enc)[:2] == [1, 1]   # the unchanged B rows below are skip-all slices
    assert len(r["rps"]["lt_curr"]) == 1 and len(r["rps"]["st_curr_before"]) == 1
    for _ in range(2):
        assert not ck.step(c["B"])["key"]


def _sps_of(data):
    dec = HevcDecoder()
    level = None
    for nal in split_annexb(data):
        if (nal[0] >> 1) & 63 == 33:
            r = unescape(nal[2:])
            dec._parse_sps(r)
            level = r[1 + 11]   # 4 + 3 + 1 bits, then 88 bits of profile_tier_level before general_level_idc
    return dec.sps, level


@pytest.mark.parametrize("slots", [3, 8])
def test_parameter_sets_announce_the_dpb(slots):
    pk = hevc_enc(slots).encode(next(sequence("A1"))[2], 0)
    assert pk[0].key
    sps, level = _sps_of(pk[0].data[10:])
    assert sps.max_dec_pic_buffering_minus1 == 1 + slots and sps.long_term is True
    assert 2 + slots <= max_dpb_size(sps.width * sps.height, level)
    dec = HevcDecoder()
    dec.decode(pk[0].data[10:])
    assert dec.pps.lists_modification


def test_level_holds_the_dpb():
    """A.4.2 worked examples through the parameter sets: 1080p60 keeps level 4.1 up to 4 slots and
    needs level 5 from 5; the level always satisfies MaxDpbSize."""
    f = np.zeros((1080, 1920, 4), np.uint8)
    for slots, want in ((0, 123), (4, 123), (5, 150)):
        e = HevcEncoder(1920, 1080, stripe_height=64, backend="cpu", **({"ltr_slots": slots} if slots else {}))
        sps, level = _sps_of(e.encode(f, 0)[0].data[10:])
        assert level == want
        if slots:
            assert 2 + slots <= max_dpb_size(sps.width * sps.height, level)


def test_without_the_cache_the_stream_is_the_parents():
    f = [fr for _, _, fr in sequence("A2")]
    a, b = hevc_enc(0), hevc_enc(None)
    for t in range(2):
        assert a.encode(f[t], t)[0].data == b.encode(f[t], t)[0].data
    sps, _ = _sps_of(hevc_enc(0).encode(f[0], 0)[0].data[10:])
    assert sps.max_dec_pic_buffering_minus1 == 1 and sps.long_term is False


def test_requested_keyframe_empties_the_cache():
    def hook(t, enc):
        if t == 15:                           # in the middle of B, after A was stored
            enc.request_keyframe()
    out, ck = _run(2, "A10 B10 A3", hook)
    assert out[15]["key"]
    assert out[14]["valid"] == 1 and out[15]["valid"] == 0
    assert not out[20]["key"] and all(s < 0 for s in out[20]["slots"])   # the switch back finds nothing, and decodes
    assert out[20]["rps"]["lt_curr"] == []


def test_expiry(monkeypatch):
    """SK_HEVC_LTR_MAX_AGE=40: A's picture (POC 9, stored at frame 10) leaves the cache at age 40, the
    switch back at frame 70 finds nothing; at the default age it matches."""
    monkeypatch.setenv("SK_HEVC_LTR_MAX_AGE", "40")
    out, ck = _run(2, "A10 B60 A3")
    assert out[48]["valid"] == 1 and out[49]["valid"] == 0      # (49 - 9) >= 40
    assert not out[70]["key"] and all(s < 0 for s in out[70]["slots"])
    assert out[50]["rps"]["lt_curr"] == [] and out[48]["rps"]["lt_curr"] == [9]
    monkeypatch.delenv("SK_HEVC_LTR_MAX_AGE")
    enc = hevc_enc(2)
    for t, (_, _, f) in enumerate(sequence("A10 B60 A1")):
        pk = enc.encode(f, t)
    assert not pk[0].key and all(s >= 0 for s in ltr_slots_of_tasks(enc))
    assert len(pk[0].data) < 0.7 * out[70]["bytes"]


def test_state_blob_carries_the_cache():
    frames = [f for _, _, f in sequence("A10 B10 A3")]
    a = hevc_enc(2)
    for t, f in enumerate(frames[:20]):
        a.encode(f, t)
    state = a.export_state()
    b = hevc_enc(2)
    b.import_state(state)
    ra = [[(p.key, p.data) for p in a.encode(f, 20 + i)] for i, f in enumerate(frames[20:])]
    rb = [[(p.key, p.data) for p in b.encode(f, 20 + i)] for i, f in enumerate(frames[20:])]
    assert ra == rb and not any(key for fr in rb for key, _ in fr)
    off = hevc_enc(0)
    ns, planes, nmb = 4, W * H * 3 // 2, 13 * 7
    assert off.state_bytes() == 64 + 44 * (ns + 1) + 4 * len(RC_FIELDS) + 3 * planes + 4 * nmb == 105632
    assert int(off.export_state()[4:8].view(np.int32)[0]) == 3
    assert a.state_bytes() == off.state_bytes() + 96 * (ns + 1) + 2 * planes
    assert int(state[4:8].view(np.int32)[0]) == 4
    with pytest.raises(RuntimeError):
        off.import_state(np.resize(state, off.state_bytes()))


def test_refusals():
    with pytest.raises(RuntimeError, match="ltr_slots"):
        hevc_enc(9)
    # 8K holds at most 4 slots at level 6.x (MaxDpbSize 6); refused before any plane is allocated
    with pytest.raises(RuntimeError, match="ltr_slots"):
        HevcEncoder(7680, 4320, stripe_height=64, backend="cpu", ltr_slots=8)


def test_capture_session_with_the_cache():
    """pixelflux capture session (CPU backend, HEVC) over a frame pool that switches A -> B -> A."""
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
                                   h264_rc_mode=0, h264_ltr_slots=2, output_mode=2)
    s.pool = pool.array.ctypes.data
    cap = pixelflux.ScreenCapture()
    cb = pixelflux.FrameCallback(on_frame)
    cap.start_frame_capture(s, cb)
    cap.run(len(frames))
    assert cap.wait(120_000) == 0
    cap.close()
    assert len(got) == len(frames) and all(len(fr) == 1 for fr in got)
    dec = HevcDecoder()
    for fr in got:
        assert len(dec.decode(fr[0][10:])) == 1
    assert got[20][0][1] == 0                                   # the switch back: no key packet
    assert len(got[20][0]) < 0.7 * len(got[10][0])
    assert dec.sps.long_term and len(dec.last_rps["lt_curr"]) >= 1   # the decoder holds long-term pictures


def test_server_reads_the_hevc_variable_for_hevc_only(monkeypatch):
    from selkies_gstreamer_amd.server.data_server import _ltr_slots_from_env
    monkeypatch.delenv("SELKIES_H264_LTR_SLOTS", raising=False)
    monkeypatch.setenv("SELKIES_HEVC_LTR_SLOTS", "11")
    assert _ltr_slots_from_env("SELKIES_HEVC_LTR_SLOTS") == 8 and _ltr_slots_from_env() == 0
    monkeypatch.setenv("SELKIES_HEVC_LTR_SLOTS", "x")
    assert _ltr_slots_from_env("SELKIES_HEVC_LTR_SLOTS") == 0
