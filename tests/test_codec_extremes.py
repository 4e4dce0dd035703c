"""The codecs at their extremes, HIP back end against the CPU reference: the quantiser rails (QP 0
and 51), the smallest pictures the front end accepts (one 16 x 16 unit; less than a CTB, a
superblock or a search window; a last unit column two samples wide; odd chroma sizes; one partial
CTB row) and CBR pinned at either end of the QP range. The lane-parallel entropy paths of the HIP
back end (k_av1_tokens, k_hevc_bins) share no code with the serial CPU coders and work in
fixed-capacity slots, and mid-QP desktop content reaches neither their long codes nor their caps.

Every run (tests/extremes_util.py) is encoded once on the CPU back end and cached. A test without
the gpu mark checks per case that an independent decoder returns the reference's reconstruction and
that the sequence really reaches its case there; the gpu test compares the HIP back end with that
reference, everything by exact equality, and decodes the HIP stream.

What the CPU runs show, and the reach checks therefore assert: new noise at a constant QP 51 is a
scene cut on HEVC (intra pictures without a skipped CU), so CU_SKIP dominates only where the rate
controller holds QP 51 (CBR at 40 kbit/s) and the constant-QP runs check their levels and packet
sizes instead; two-level noise and saturated tiles keep small levels even at QP 51."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from tests import extremes_util as xu
from tests.extremes_util import CU_SKIP, cbr, rail, run

SIZES = [(16, 16), (18, 18), (34, 34), (66, 18), (72, 40)]
RAILS = (0, 51)
HEVC_ESCAPE = 3 << 4   # coeff_abs_level_remaining takes the escape prefix from here at rice 4 (and sooner below)


def _h264(W, H, fullframe, content, qp):
    return run("h264", W, H, content, stripe_height=16, fullframe=fullframe, qp=qp, paint_qp=qp, use_paint_over=False)


def _jpeg(W, H, content, quality):
    return run("jpeg", W, H, content, stripe_height=16, quality=quality, paint_quality=quality)


# name -> the runs of the case (each a short sequence through one encoder)
CASES = {}
for codec in ("hevc", "av1"):
    for content in xu.CONTENT:   # 1. quantiser rails, every content at 96 x 64
        CASES[f"{codec}_rails_{content}"] = [rail(codec, 96, 64, content, q) for q in RAILS]
    for W, H in SIZES:           # 1. + 2. rails at the geometry floor
        CASES[f"{codec}_floor_{W}x{H}"] = [rail(codec, W, H, c, q) for c in ("noise", "binary") for q in RAILS]
    for kbps in (40, 400000):    # 3. CBR on the rails
        CASES[f"{codec}_cbr_{kbps}"] = [cbr(codec, kbps)]
for W, H in SIZES:               # 2. geometry floor, H.264 (a 2-row last stripe at 18 and 34) and JPEG
    for fullframe in (False, True):
        CASES[f"h264_floor_{W}x{H}_{'picture' if fullframe else 'stripes'}"] = \
            [_h264(W, H, fullframe, c, q) for c in ("noise", "binary") for q in RAILS]
    CASES[f"jpeg_floor_{W}x{H}"] = [_jpeg(W, H, c, q) for c in ("noise", "primaries") for q in (1, 100)]


def _skip_without_decoder(name):
    if name.startswith("av1") and not dav1d.available():
        pytest.skip("dav1d (Pillow libavif) not available")


def _opt(r, key):
    return dict(r[5]).get(key)


def _levels(snaps, key):
    return np.concatenate([np.abs(s[key].astype(np.int32)) for s in snaps])


def _payload(snap):
    return sum(len(p[3]) - 10 for p in snap["packets"])


def _check_rail_reach(r, snaps):
    """The facts that make a constant-QP run a rail case, on the CPU reference. The thresholds are
    relations the CPU run shows with a wide margin (the figures are in profiles/extremes_headroom.md)."""
    codec, W, H, content = r[:4]
    qp = _opt(r, "qp")
    key = "coefs" if codec == "hevc" else "levels"
    lev = _levels(snaps, key)
    inter = snaps[1:]
    for s in snaps:
        coded = s["tasks"]["final_action"] != 0
        assert coded.all() and (s["tasks"]["qp"] == qp).all(), s["tasks"]
    if codec == "av1":
        assert all(s["av1_qidx"] == (1 if qp == 0 else 254) for s in snaps), [s["av1_qidx"] for s in snaps]
    if qp == 0 and content in ("noise", "binary"):
        if codec == "av1":   # Golomb remainders (|level| > 14): more than one for every 16 pixels coded
            assert (lev > 14).sum() > W * H * len(snaps) // 16, int((lev > 14).sum())
        else:
            # |level| - base >= 3 << 4 takes the escape prefix of coeff_abs_level_remaining at any rice
            # parameter (base <= 3): at least one such level per unit; and the fullest bin slot holds
            # more than the same content fills at QP 26 (noise: about 1640 against 1300 of 4096)
            units = ((W + 15) // 16) * ((H + 15) // 16)
            assert (lev - 3 >= HEVC_ESCAPE).sum() >= units, (int(lev.max()), int((lev - 3 >= HEVC_ESCAPE).sum()))
            mid = xu.reference(rail(codec, W, H, content, 26))[1]
            assert _max_bin_n(snaps) > _max_bin_n(mid), (_max_bin_n(snaps), _max_bin_n(mid))
    if qp == 0 and content == "flat_steps":
        assert np.count_nonzero(lev) <= 64 and lev.max() > 1000, int(lev.max())   # a few long codes, nothing else
    if content == "binary" and codec == "av1":
        # BlkInfo's palette size is readable: the key frame codes two-colour palettes, inter frames none.
        # At QP 0 the palette key frame is exact and several times smaller than an inter frame.
        pal = snaps[0]["blk"][:, 10]
        assert set(pal.tolist()) <= {0, 2} and (pal == 2).sum() > 0.8 * len(pal), np.bincount(pal).tolist()
        assert not any(s["blk"][:, 10].any() for s in inter)
        if qp == 0:
            assert 3 * _payload(snaps[0]) < min(_payload(s) for s in inter), [_payload(s) for s in snaps]
    if qp == 51:
        assert lev.max() < 32, int(lev.max())   # nothing near the long codes of QP 0
        if content in ("noise", "flat_steps", "checker"):
            # (two-level noise and saturated tiles keep levels in a fifth of the positions even here)
            assert np.count_nonzero(lev) < lev.size // 50, int(np.count_nonzero(lev))
            assert max(_payload(s) for s in inter) < 128, [_payload(s) for s in inter]
    if content == "checker":
        if qp == 0:   # the inter frames find their exact match: no levels
            assert not any(s[key].any() for s in inter)
        if codec == "hevc":   # and skipped CUs (new noise is a scene cut instead: intra pictures, no skips)
            assert sum(int((s["cus"][:, 0] == CU_SKIP).sum()) for s in inter) > 0


def _max_bin_n(snaps):
    return max(int(s["bin_n"].max()) for s in snaps)


def _check_cbr_reach(r, snaps, stats):
    """The controller reaches its rail (tasks["qp"] of every frame). rc_stats counts the frames coded
    again in `redos`: at 40 kbit/s at least one was. There the HEVC inter pictures are mostly CU_SKIP."""
    kbps = _opt(r, "bitrate_kbps")
    qps = [int(s["tasks"]["qp"].max()) for s in snaps]
    if kbps == 40:
        assert max(qps) == 51 and min(qps) >= 44 and qps.count(51) >= 4, qps
        assert stats["redos"] >= 1, stats
        if r[0] == "hevc":
            modes = np.concatenate([s["cus"][:, 0] for s in snaps[1:]])
            assert (modes == CU_SKIP).sum() > len(modes) // 2, np.bincount(modes).tolist()
    else:
        assert set(qps[3:]) == {0}, qps
        assert stats["redos"] == 0, stats
    if r[0] == "av1":
        assert snaps[-1]["av1_qidx"] == (254 if kbps == 40 else 1), snaps[-1]["av1_qidx"]


def _check_geometry_reach(r, snaps):
    """Every frame of a floor run codes every stripe of the picture (JPEG: one packet per 16 rows)."""
    codec, W, H = r[:3]
    if codec == "jpeg":
        stripes = (H + 15) // 16
        assert all(len(s["packets"]) == stripes for s in snaps), [len(s["packets"]) for s in snaps]
        assert sum(p[1] for p in snaps[0]["packets"]) == H
    else:
        assert all((s["tasks"]["final_action"] != 0).all() for s in snaps)
        if codec == "h264" and not _opt(r, "fullframe"):   # one stream per 16 rows; 18 and 34 end in a 2-row stripe
            assert len(snaps[0]["tasks"]) == (H + 15) // 16


@pytest.mark.parametrize("name", list(CASES))
def test_reference_decodes_and_reaches_its_case(name):
    _skip_without_decoder(name)
    for r in CASES[name]:
        frames, snaps, stats = xu.reference(r)
        xu.assert_decodes(r, snaps, f"{name} {r}: CPU")
        if r[0] in ("hevc", "av1"):
            if _opt(r, "rate_control") == "cbr":
                _check_cbr_reach(r, snaps, stats)
            else:
                _check_rail_reach(r, snaps)
            if r[0] == "hevc":   # slot headroom of the CPU back end (profiles/extremes_headroom.md)
                print(f"headroom cpu {name} {r[3]} {dict(r[5])}: bin_n {_max_bin_n(snaps)} of {xu.K_CU_BIN_CAP}")
                assert _max_bin_n(snaps) < xu.K_CU_BIN_CAP
        if "floor" in name:
            _check_geometry_reach(r, snaps)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_matches_cpu(name):
    xu.need_gpu()
    _skip_without_decoder(name)
    for r in CASES[name]:
        codec, W, H = r[:3]
        frames, ref, _ = xu.reference(r)
        gpu = xu.encoder(r, "hip")
        got, top = [], {}
        for t, f in enumerate(frames):
            got.append(xu.snapshot(gpu, r, gpu.encode(f, t)))
            # slot headroom, before anything is compared: bins per unit and substream bytes per CTB row
            # (HEVC), tokens per unit (AV1; a write past the cap would be dropped without an error)
            for n in dict(hevc=("bin_n", "sub_size"), av1=("tok_n",)).get(codec, ()):
                top[n] = max(top.get(n, 0), int(gpu.debug_buffer(n, np.int32).max()))
            if codec == "h264":
                from tests.test_h264_gpu import _compare_state
                _compare_state(xu.Recorded(ref[t]), xu.Recorded(got[t]), W, t)
            xu.assert_same(r, t, got[t], ref[t])
        gpu.close()
        if top:
            print(f"headroom hip {name} {r[3]} {dict(r[5])}: {top}")
        room = dict(bin_n=xu.K_CU_BIN_CAP, tok_n=xu.K_TOK_CAP, sub_size=(W + 31) // 32 * 4 * xu.K_SUBSTREAM_CTB_BYTES)
        for n, v in top.items():
            assert v < room[n], f"{n}: {v} of {room[n]}"
        xu.assert_decodes(r, got, f"{name} {r}: HIP")
