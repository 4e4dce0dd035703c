"""The front end of every encoder against BT.709 and an independent numpy model
(tests/frontend_model.py): colour conversion in both ranges, resampling, the overlay composite,
edge padding, damage detection, planar input, the stand-alone converter, and the colour
description the streams announce.

Every sequence runs once on the CPU back end (`cpu_run`, cached) and the model computes its planes
and damage once (`model_run`, cached). The tests without the gpu mark hold the CPU back end to the
model and check that a case reaches the path it is meant for; the gpu tests hold the HIP back end
to the model (source planes, per-macroblock damage) and to the CPU back end (packets). Every
comparison is exact except the two against real numbers: the integer arithmetic against the
BT.709 definition, and the decoded colours of the round trip."""
from __future__ import annotations

import collections
import functools

import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, H264Encoder, HevcEncoder, convert_bgrx, hip_device_count
from tests import frontend_model as fm
from tests.extremes_util import primaries

CODECS = ("h264", "h264ff", "hevc", "av1")     # H.264 in stripes of 16 rows and as one picture
STREAMS = ("h264", "hevc", "av1")
RANGES = (False, True)

Case = collections.namedtuple("Case", "kind codec W H full_range extra")
Frame = collections.namedtuple("Frame", "packets planes dirty")


def need_gpu():
    if hip_device_count() < 1:
        pytest.skip("no HIP device")


def case_id(v):
    if isinstance(v, bool):
        return "full" if v else "limited"
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return str(v)


# ---- content -------------------------------------------------------------------------------------
def _seed(*key):
    return np.random.default_rng([int(k) for k in key])


def capture(w, h, pad, n=3):
    """n frames of a w x h capture inside rows of w + pad pixels: ((h, w, 4) pixel view, the 2-D
    row array handed to encode(), whose row stride is (w + pad) * 4). Two frames of noise, then
    saturated primaries; the pixels are the same for every pad, the padding is noise of its own."""
    rng, junk = _seed(w, h), _seed(w, h, pad)
    out = []
    for t in range(n):
        a = junk.integers(0, 256, (h, w + pad, 4), dtype=np.uint8)
        a[:, :w] = primaries(w, h, 1, seed=w + h)[0] if t == n - 1 else rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        out.append((a[:, :w], a.reshape(h, -1)))
    return out


def premul(rng, h, w):
    """A premultiplied BGRA overlay image, a fifth of it fully transparent."""
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((h, w)) < 0.2, 0, img[..., 3])
    img[..., :3] = (img[..., :3].astype(np.uint32) * img[..., 3:4] // 255).astype(np.uint8)
    return img


OVERLAY = premul(_seed(7), 20, 24)


def overlay_pos(W, H, t):
    """The overlay crosses the right and the bottom edge of the picture, and moves."""
    return (W - 14 - t, H - 12 - 2 * t)


@functools.lru_cache(maxsize=None)
def equal_luma_pair():
    """Two colours (b, g, r) of equal Y and different Cb as uniform quads, limited range, found by
    searching the model: all (r, b) at g = 128."""
    r, b = np.mgrid[0:256, 0:256]
    pic = np.zeros((256, 256, 4), np.uint8)
    pic[..., 0], pic[..., 1], pic[..., 2] = b, 128, r
    y, u, _ = fm.convert_int(np.repeat(np.repeat(pic, 2, 0), 2, 1), False)
    y, u = y[0::2, 0::2].astype(int), u.astype(int)
    best = None
    for level in np.unique(y):
        idx = np.argwhere(y == level)
        cb = u[idx[:, 0], idx[:, 1]]
        lo, hi = idx[cb.argmin()], idx[cb.argmax()]
        if best is None or cb.max() - cb.min() > best[0]:
            best = (cb.max() - cb.min(), (int(lo[1]), 128, int(lo[0])), (int(hi[1]), 128, int(hi[0])))
    assert best[0] > 0
    return best[1], best[2]


@functools.lru_cache(maxsize=None)
def damage_script(W, H):
    """[(name, frame, the macroblocks (row, column) that must be dirty, or None: all)]: frame 0 is
    noise, then one change per frame."""
    mb_w, mb_h = (W + 15) // 16, (H + 15) // 16
    f = _seed(W, H, 3).integers(0, 256, (H, W, 4), dtype=np.uint8)
    steps = [("first", f.copy(), None)]

    def step(name, dirty):
        steps.append((name, f.copy(), frozenset(dirty)))

    def poke(y, x):
        f[y, x, 1] ^= 0x80
        return (y // 16, x // 16)
    f[::3, ::5, 3] ^= 0xFF
    f[H - 1, W - 1, 3] ^= 0x55
    step("x_byte", [])
    step("corners", [poke(0, 0), poke(0, W - 1), poke(H - 1, 0), poke(H - 1, W - 1)])
    step("last_column", [poke(H // 2, W - 1)])
    a, b = equal_luma_pair()
    f[4:6, 20:22, :3] = a
    step("paint", [(0, 1)])
    f[4:6, 20:22, :3] = b
    step("equal_luma", [(0, 1)])
    row = min(20, H - 2)
    for x in (7, 8) + ((255, 256) if W > 256 else ()):
        step(f"x{x}", [poke(row, x)])
    step("same", [])
    assert all(r < mb_h and c < mb_w for _, _, d in steps if d for r, c in d)
    return steps


@functools.lru_cache(maxsize=None)
def planar_script(W, H):
    """[(fmt, (y, u, v), device planes on the HIP back end?, dirty macroblocks or None: all)]"""
    cw, ch = (W + 1) // 2, (H + 1) // 2
    mb_w, mb_h = (W + 15) // 16, (H + 15) // 16
    rng = _seed(W, H, 5)
    y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (ch, cw), (ch, cw)))
    steps = []

    def step(fmt, dev, dirty):
        steps.append((fmt, (y.copy(), u.copy(), v.copy()), dev, None if dirty is None else frozenset(dirty)))
    last = (mb_h - 1, mb_w - 1)
    step("i420", False, None)
    y[H - 1, W - 1] ^= 0x40           # the luma corner: its padding row, column and corner follow
    step("i420", True, [last])
    u[ch - 1, cw - 1] ^= 0x40         # the last Cb sample alone
    step("i420", False, [last])
    step("nv12", False, [])           # the same samples in the other layout
    v[0, 0] ^= 0x40
    step("nv12", True, [(0, 0)])
    y[:], u[:], v[:] = (rng.integers(0, 256, a.shape, dtype=np.uint8) for a in (y, u, v))
    step("nv12", False, None)
    return steps


def as_fmt(fmt, planes):
    y, u, v = planes
    if fmt == "nv12":
        return y, np.ascontiguousarray(np.stack([u, v], axis=2).reshape(u.shape[0], -1))
    return y, u, v


PATCHES = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (255, 0, 255),
           (0, 255, 255), (64, 64, 64), (128, 128, 128), (192, 192, 192), (128, 128, 128))   # (r, g, b)
PATCH, PATCH_COLS = 32, 4


def patch_frame():
    """Flat 32x32 patches, four to a row: black, white, the six saturated primaries, three greys
    (the twelfth cell repeats the middle grey)."""
    rows = len(PATCHES) // PATCH_COLS
    f = np.zeros((rows * PATCH, PATCH_COLS * PATCH, 4), np.uint8)
    for i, (r, g, b) in enumerate(PATCHES):
        f[i // PATCH_COLS * PATCH:, i % PATCH_COLS * PATCH:, :3] = (b, g, r)
    return f


# ---- cases ---------------------------------------------------------------------------------------
def steps_of(c):
    """The frames of a case: dicts with `rows` (the array for encode()) and `pixels` (its (h, w, 4)
    view), or `yuv` (fmt, planes) and `dev`; `pos`: where the overlay goes before the frame."""
    if c.kind == "planes":
        return [dict(pixels=p, rows=r) for p, r in capture(c.W, c.H, c.extra)]
    if c.kind in ("scale", "noscale"):
        sw, sh, pad, ov = c.extra
        return [dict(pixels=p, rows=r, **(dict(pos=overlay_pos(c.W, c.H, t)) if ov else {}))
                for t, (p, r) in enumerate(capture(sw, sh, pad))]
    if c.kind == "damage":
        return [dict(pixels=f, rows=f) for _, f, _ in damage_script(c.W, c.H)]
    if c.kind == "planar":
        return [dict(yuv=(fmt, as_fmt(fmt, p)), dev=dev) for fmt, p, dev, _ in planar_script(c.W, c.H)]
    if c.kind == "patches":
        return [dict(pixels=patch_frame(), rows=patch_frame())]
    raise KeyError(c.kind)


def stripe_height(c):
    return 32 if c.kind == "patches" else 16


def encoder_of(c, backend):
    cls, kw = dict(h264=(H264Encoder, dict(stripe_height=stripe_height(c))),
                   h264ff=(H264Encoder, dict(fullframe=True)), hevc=(HevcEncoder, {}), av1=(Av1Encoder, {}))[c.codec]
    kw = dict(kw, full_range=c.full_range, use_paint_over=False, backend=backend)
    if c.kind == "scale":
        kw.update(src_width=c.extra[0], src_height=c.extra[1])
    if c.kind == "patches":
        kw.update(qp=4, paint_qp=4, rate_control="cqp")
    enc = cls(c.W, c.H, **kw)
    if c.kind in ("scale", "noscale") and c.extra[3]:
        enc.set_overlay(0, OVERLAY)
    return enc


@functools.lru_cache(maxsize=None)
def _model_run(kind, W, H, full_range, extra):
    c = Case(kind, "", W, H, full_range, extra)
    out, prev = [], None
    for t, st in enumerate(steps_of(c)):
        if "yuv" in st:
            planes = fm.planes_planar(st["yuv"][0], st["yuv"][1], W, H)
        else:
            ov = [(OVERLAY,) + st["pos"] + (None,)] if "pos" in st else []
            src = (extra[0], extra[1]) if kind in ("scale", "noscale") else None
            planes = fm.planes_int(st["pixels"], W, H, full_range, src_size=src, overlays=ov)
        dirty = fm.damage(prev, planes, t == 0)
        for a in planes + (dirty,):
            a.setflags(write=False)
        out.append((planes, dirty))
        prev = planes
    return out


def model_run(c):
    """[(padded planes, dirty macroblocks)] of every frame of the case, by the model: the same for
    every codec."""
    return _model_run(c.kind, c.W, c.H, c.full_range, c.extra)


def drive(c, backend):
    """Runs the case through one encoder: per frame the packets, the padded source planes and the
    damage map (None where the back end exposes none)."""
    from selkies_gstreamer_amd.ops.native import DevicePlane
    enc = encoder_of(c, backend)
    pw, ph = fm.padded_size(c.W, c.H)
    out = []
    for t, st in enumerate(steps_of(c)):
        if "pos" in st:
            enc.set_overlay_pos(0, *st["pos"])
        if "yuv" in st:
            fmt, planes = st["yuv"]
            dev = [DevicePlane(p) for p in planes] if st["dev"] and backend == "hip" else None
            pk = enc.encode_yuv(fmt, *(dev or planes), frame_id=t)
            for d in dev or ():
                d.close()
        else:
            pk = enc.encode(st["rows"], t)
        planes = tuple(enc.debug_buffer(n).reshape(s).copy()
                       for n, s in (("src_y", (ph, pw)), ("src_u", (ph // 2, pw // 2)), ("src_v", (ph // 2, pw // 2))))
        try:
            dirty = enc.debug_buffer("mb_dirty").reshape(ph // 16, pw // 16).astype(bool)
        except KeyError:   # the CPU HEVC and AV1 back ends keep no map of their own
            dirty = None
        out.append(Frame([(p.y, p.h, p.key, p.data) for p in pk], planes, dirty))
    enc.close()
    return out


@functools.lru_cache(maxsize=None)
def cpu_run(c):
    return drive(c, "cpu")


def assert_planes(got, want, what):
    for name, a, b in zip("YUV", got, want):
        assert a.shape == b.shape, f"{what}: plane {name} is {a.shape}, the model's {b.shape}"
        bad = np.argwhere(a != b)
        assert len(bad) == 0, (f"{what}: plane {name} differs from the model in {len(bad)} samples, first (row, column) "
                               f"{bad[:4].tolist()}: {[int(a[tuple(i)]) for i in bad[:4]]} for {[int(b[tuple(i)]) for i in bad[:4]]}")


def assert_dirty(got, want, what):
    assert np.array_equal(got, want), f"{what}: dirty macroblocks {np.argwhere(got).tolist()}, the model's {np.argwhere(want).tolist()}"


def check_against_model(c, frames, who, need_dirty):
    for t, (fr, (planes, dirty)) in enumerate(zip(frames, model_run(c))):
        what = f"{who} {c.codec} {c.kind} {c.W}x{c.H} {case_id(c.full_range)} {c.extra} frame {t}"
        assert_planes(fr.planes, planes, what)
        if need_dirty:
            assert fr.dirty is not None, f"{what}: no damage map"
        if fr.dirty is not None:
            assert_dirty(fr.dirty, dirty, what)
        if c.codec == "h264":   # a stripe sends a packet exactly when one of its macroblocks is dirty
            sh = stripe_height(c)
            rows = np.flatnonzero(dirty.any(axis=1)) * 16 // sh
            assert sorted(p[0] for p in fr.packets) == sorted({sh * int(r) for r in rows}), what


def check_hip(c, need_dirty=True):
    need_gpu()
    frames = drive(c, "hip")
    check_against_model(c, frames, "hip", need_dirty)
    for t, (g, r) in enumerate(zip(frames, cpu_run(c))):
        assert g.packets == r.packets, f"{c}: frame {t}: the HIP packets differ from the CPU back end's"
    return frames


# ---- a. the integer arithmetic against BT.709 ----------------------------------------------------
BT709_BOUND = 1.2   # half a level of rounding plus the rounding of three 8-bit coefficients


def _quads(colours):
    """(n, m, 3) b, g, r -> a BGRx picture of uniform 2x2 quads."""
    pic = np.zeros(colours.shape[:2] + (4,), np.uint8)
    pic[..., :3] = colours
    return np.repeat(np.repeat(pic, 2, 0), 2, 1)


@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
def test_integer_conversion_within_bt709(full_range):
    """All 2^24 colours as uniform quads, then 10^5 random mixed quads: every Y, Cb and Cr of the
    integer model is within 1.2 of the unrounded BT.709 value. (Worst: limited Y 0.88, Cb 1.17,
    Cr 0.93; full Y 1.02, Cb 0.80, Cr 0.73.)"""
    worst = np.zeros(3)
    g, b = np.mgrid[0:256, 0:256]
    for r in range(256):
        pic = _quads(np.stack([b, g, np.full_like(g, r)], axis=2).astype(np.uint8))
        got, want = fm.planes_int(pic, 512, 512, full_range), fm.bt709_float(pic, full_range)
        worst = np.maximum(worst, [np.abs(a - w).max() for a, w in zip(got, want)])
    mixed = _seed(24).integers(0, 256, (400, 1000, 4), dtype=np.uint8)   # 200 x 500 quads
    got, want = fm.planes_int(mixed, 1000, 400, full_range), fm.bt709_float(mixed, full_range)
    pw, ph = fm.padded_size(1000, 400)
    assert got[0].shape == (ph, pw)
    worst = np.maximum(worst, [np.abs(a[:w.shape[0], :w.shape[1]] - w).max() for a, w in zip(got, want)])
    print(f"full_range={full_range}: worst |integer - BT.709| Y {worst[0]:.3f} Cb {worst[1]:.3f} Cr {worst[2]:.3f}")
    assert (worst <= BT709_BOUND).all(), worst


@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
def test_integer_conversion_anchors(full_range):
    v = np.arange(256, dtype=np.uint8)
    grey = _quads(np.stack([v, v, v], axis=1)[None])
    y, u, w = fm.convert_int(grey, full_range)
    assert (u == 128).all() and (w == 128).all(), "a grey has no colour"
    assert (int(y[0, 0]), int(y[0, -1])) == ((0, 255) if full_range else (16, 235)), "black and white"
    assert (np.diff(y[0].astype(int)) >= 0).all()
    # Y is monotone in each of R, G and B, for every value of the other two on a grid of 18
    grid = np.array(sorted(set(range(0, 256, 15)) | {255}), np.uint8)
    for ch in range(3):
        a, b = np.meshgrid(grid, grid, indexing="ij")
        cols = np.zeros((len(grid) ** 2, 256, 3), np.uint8)
        cols[..., ch] = v[None, :]
        cols[..., (ch + 1) % 3] = a.reshape(-1, 1)
        cols[..., (ch + 2) % 3] = b.reshape(-1, 1)
        yy = fm.convert_int(_quads(cols), full_range)[0][0::2, 0::2].astype(int)
        assert (np.diff(yy, axis=1) >= 0).all(), f"Y falls as channel {ch} rises"
    if not full_range:   # the limited range is kept by every colour
        g, b = np.mgrid[0:256, 0:256]
        for r in range(0, 256, 5):
            y, u, w = fm.convert_int(_quads(np.stack([b, g, np.full_like(g, r)], axis=2).astype(np.uint8)), False)
            assert y.min() >= 16 and y.max() <= 235
            assert min(u.min(), w.min()) >= 16 and max(u.max(), w.max()) <= 240


# ---- b. source planes ----------------------------------------------------------------------------
# (W, H, extra pixels per capture row): the row stride is (W + extra) * 4 bytes. Of the 8-pixel items of
# a padded row: how many load 16-byte vectors, how many load pixel by pixel with the column clamped;
# and the workgroups of 256 columns across. A tight row of 18 or 66 pixels is not a multiple of 16
# bytes, so those pictures load pixel by pixel throughout; 18 pixels in rows of 20 have vector items
# and a partly clamped per-pixel item side by side.
PLANE_PATHS = {
    (16, 16, 0): (2, 0, 1),       # one item pair
    (18, 18, 0): (0, 4, 1),       # stride 72: per-pixel, the third item clamps from column 18, chroma 9 wide
    (18, 18, 2): (2, 2, 1),       # stride 80: two vector items, then the clamping one
    (24, 16, 0): (3, 1, 1),       # stride 96: vectors; the fourth item is padding only
    (24, 16, 1): (0, 4, 1),       # stride 100: the same pixels, pixel by pixel
    (24, 16, 4): (3, 1, 1),       # stride 112: vectors with a padded stride
    (264, 16, 0): (33, 1, 2),     # second workgroup, of two items
    (272, 34, 0): (34, 0, 2),     # second workgroup; a last stripe of 2 rows, a partial CTB row
    (66, 18, 0): (0, 10, 1),
}
PLANE_SHAPES = tuple(PLANE_PATHS)


def load_paths(W, stride):
    """(vector items, per-pixel items, workgroups across) of the conversion kernel for a picture W
    wide whose capture rows are `stride` bytes apart: an item is 8 columns of the padded row, and
    loads vectors when all 8 lie in the picture and the rows keep 16-byte alignment."""
    pw = (W + 15) // 16 * 16
    vec = sum(1 for x0 in range(0, pw, 8) if x0 + 7 < W and stride % 16 == 0)
    return vec, pw // 8 - vec, (pw + 255) // 256


def plane_case(codec, full_range, shape):
    return Case("planes", codec, shape[0], shape[1], full_range, shape[2])


@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=case_id)
def test_plane_cases_reach_their_paths(shape):
    W, H, pad = shape
    rows = steps_of(plane_case("h264", False, shape))[0]["rows"]
    assert rows.flags["C_CONTIGUOUS"] and rows.strides[0] == (W + pad) * 4, "encode() must see this stride"
    assert load_paths(W, rows.strides[0]) == PLANE_PATHS[shape]
    if pad:   # the same pixels as the tight capture, so the same planes
        tight = steps_of(plane_case("h264", False, (W, H, 0)))
        padded = steps_of(plane_case("h264", False, shape))
        assert all(np.array_equal(a["pixels"], b["pixels"]) for a, b in zip(padded, tight))


@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", CODECS)
def test_source_planes_cpu(codec, full_range):
    for shape in PLANE_SHAPES:
        c = plane_case(codec, full_range, shape)
        check_against_model(c, cpu_run(c), "cpu", codec.startswith("h264"))
    tight = cpu_run(plane_case(codec, full_range, (24, 16, 0)))
    for pad in (1, 4):
        for a, b in zip(cpu_run(plane_case(codec, full_range, (24, 16, pad))), tight):
            assert a.packets == b.packets


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PLANE_SHAPES, ids=case_id)
@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", CODECS)
def test_source_planes_hip(codec, full_range, shape):
    check_hip(plane_case(codec, full_range, shape))


# ---- c. resampling -------------------------------------------------------------------------------
# capture (w, h) -> picture (W, H)
SCALE_SHAPES = (((97, 53), (64, 48)), ((130, 70), (192, 112)), ((2, 2), (16, 16)), ((64, 64), (16, 16)),
                ((40, 20), (272, 32)))
EQUAL = (48, 32)
OVERLAID = ((97, 53), (66, 50), 3)   # and 3 pixels of row padding in the capture


def scale_case(codec, full_range, src, dst, pad=0, ov=False, kind="scale"):
    return Case(kind, codec, dst[0], dst[1], full_range, (src[0], src[1], pad, ov))


def scale_cases(codec, full_range):
    return [scale_case(codec, full_range, s, d) for s, d in SCALE_SHAPES] + \
        [scale_case(codec, full_range, EQUAL, EQUAL), scale_case(codec, full_range, *OVERLAID, ov=True)]


def test_scale_cases_reach_their_paths():
    for c in scale_cases("h264", False):
        sw, sh, pad, ov = c.extra
        plain = fm.planes_int(steps_of(c)[0]["pixels"][:min(sh, c.H), :min(sw, c.W)], min(sw, c.W), min(sh, c.H), False)
        resampled = model_run(c)[0][0]
        if (sw, sh) == (c.W, c.H):
            assert all(np.array_equal(a, b) for a, b in zip(plain, resampled)), "equal sizes resample nothing"
        else:
            assert resampled[0].shape != plain[0].shape or not np.array_equal(resampled[0], plain[0])
        if ov:
            bare = model_run(scale_case("h264", False, (sw, sh), (c.W, c.H), pad))
            x, y = steps_of(c)[0]["pos"]
            assert x + OVERLAY.shape[1] > c.W and y + OVERLAY.shape[0] > c.H, "the overlay crosses both edges"
            diff = bare[0][0][0] != resampled[0]
            assert diff[:c.H, :c.W].any() and diff[:, c.W:].any() and diff[c.H:].any(), \
                "the overlay shows in the picture and in the padding beside and below it"
            assert steps_of(c)[0]["rows"].strides[0] == (sw + pad) * 4 and pad
    up = scale_case("h264", False, (40, 20), (272, 32))
    assert load_paths(up.W, 160)[2] == 2, "two workgroups across"
    clamp = model_run(scale_case("h264", False, (2, 2), (16, 16)))[0][0][0]
    assert len(np.unique(clamp)) > 1


@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_resampling_cpu(codec, full_range):
    for c in scale_cases(codec, full_range):
        check_against_model(c, cpu_run(c), "cpu", codec == "h264")
    same = cpu_run(scale_case(codec, full_range, EQUAL, EQUAL, kind="noscale"))
    for a, b in zip(cpu_run(scale_case(codec, full_range, EQUAL, EQUAL)), same):
        assert a.packets == b.packets, "src_width equal to the width must change nothing"


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(SCALE_SHAPES) + 2))
@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_resampling_hip(codec, full_range, which):
    c = scale_cases(codec, full_range)[which]
    frames = check_hip(c)
    if c.extra[:2] == EQUAL:
        for a, b in zip(frames, cpu_run(scale_case(codec, full_range, EQUAL, EQUAL, kind="noscale"))):
            assert a.packets == b.packets, "src_width equal to the width must change nothing"


# ---- d. damage -----------------------------------------------------------------------------------
DAMAGE_SHAPES = ((48, 32), (272, 32), (66, 18))


@pytest.mark.parametrize("shape", DAMAGE_SHAPES, ids=case_id)
def test_damage_script_reaches_its_cases(shape):
    """The model's damage of every scripted change is the set of macroblocks written by hand."""
    W, H = shape
    c = Case("damage", "h264", W, H, False, None)
    script, model = damage_script(W, H), model_run(c)
    names = [s[0] for s in script]
    for (name, _, want), (_, dirty) in zip(script, model):
        got = frozenset((int(r), int(k)) for r, k in np.argwhere(dirty))
        assert dirty.all() if want is None else got == want, f"{name}: {sorted(got)}"
    i = names.index("equal_luma")
    (y0, u0, _), (y1, u1, _) = model[i - 1][0], model[i][0]
    assert np.array_equal(y0, y1) and not np.array_equal(u0, u1), "luma the same, Cb not"
    i = names.index("last_column")
    if W % 16:   # the replicated columns change with the last pixel
        assert (model[i - 1][0][0][:, W:] != model[i][0][0][:, W:]).any()
    assert ("x256" in names) == (W > 256)
    i = names.index("x_byte")
    assert not np.array_equal(script[i][1], script[i - 1][1])


@pytest.mark.parametrize("shape", DAMAGE_SHAPES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_damage_cpu(codec, shape):
    c = Case("damage", codec, shape[0], shape[1], False, None)
    check_against_model(c, cpu_run(c), "cpu", codec == "h264")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DAMAGE_SHAPES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_damage_hip(codec, shape):
    check_hip(Case("damage", codec, shape[0], shape[1], False, None))


# ---- e. planar input -----------------------------------------------------------------------------
PLANAR_SHAPES = ((18, 18), (66, 18), (200, 90))


@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=case_id)
def test_planar_script_reaches_its_cases(shape):
    W, H = shape
    c = Case("planar", "h264", W, H, False, None)
    script, model = planar_script(W, H), model_run(c)
    assert {(s[0], s[2]) for s in script} == {(f, d) for f in ("i420", "nv12") for d in (False, True)}
    for (_, _, _, want), (_, dirty) in zip(script, model):
        got = frozenset((int(r), int(k)) for r, k in np.argwhere(dirty))
        assert dirty.all() if want is None else got == want
    (y0, u0, _), (y1, u1, _), (_, u2, _) = model[0][0], model[1][0], model[2][0]
    assert (y0 != y1)[H:, W:].all(), "the padding corner repeats the last luma sample"
    cw, ch = (W + 1) // 2, (H + 1) // 2
    assert (u1 != u2)[ch - 1:, cw - 1:].all() and (u1 != u2).sum() == (u1.shape[0] - ch + 1) * (u1.shape[1] - cw + 1)


@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_planar_input_cpu(codec, shape):
    c = Case("planar", codec, shape[0], shape[1], False, None)
    check_against_model(c, cpu_run(c), "cpu", codec == "h264")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PLANAR_SHAPES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_planar_input_hip(codec, shape):
    check_hip(Case("planar", codec, shape[0], shape[1], False, None))


# ---- f. the stand-alone converter ----------------------------------------------------------------
CONVERT_SIZES = ((2, 2), (3, 3), (17, 5), (514, 4), (130, 66))   # 514: quad column 256 is the second block's first


def check_converter(backend):
    for W, H in CONVERT_SIZES:
        f = _seed(W, H, 9).integers(0, 256, (H, W, 4), dtype=np.uint8)
        for full_range in RANGES:
            y, u, v = fm.planes_unpadded(f, full_range)
            assert y.shape == (H, W) and u.shape == ((H + 1) // 2, (W + 1) // 2)
            gy, gu, gv = convert_bgrx(f, "i420", backend=backend, full_range=full_range)
            ny, nuv = convert_bgrx(f, "nv12", backend=backend, full_range=full_range)
            what = f"{backend} {W}x{H} {case_id(full_range)}"
            assert_planes((gy, gu, gv), (y, u, v), what + " i420")
            assert_planes((ny, nuv[:, 0::2], nuv[:, 1::2]), (y, u, v), what + " nv12")


def test_converter_cpu():
    assert (CONVERT_SIZES[3][0] + 1) // 2 > 256
    check_converter("cpu")


@pytest.mark.gpu
def test_converter_hip():
    need_gpu()
    check_converter("hip")


# ---- g. signalling and colour round trip ---------------------------------------------------------
def patch_case(codec, full_range):
    f = patch_frame()
    return Case("patches", codec, f.shape[1], f.shape[0], full_range, None)


def rgb_of(y, cb, cr, full_range):
    """The float64 inverse of bt709_float for one sample: (r, g, b) on the 0..255 scale, neither
    rounded nor clipped."""
    ey, ecb, ecr = (y / 255.0, (cb - 128.0) / 255.0, (cr - 128.0) / 255.0) if full_range else \
        ((y - 16.0) / 219.0, (cb - 128.0) / 224.0, (cr - 128.0) / 224.0)
    r = ey + 2.0 * (1.0 - fm.KR) * ecr
    b = ey + 2.0 * (1.0 - fm.KB) * ecb
    g = (ey - fm.KR * r - fm.KB * b) / fm.KG
    return np.array([r, g, b]) * 255.0


def decode(codec, W, H, packets):
    if codec == "h264":
        from tests.h264_util import StripeDecoder
        dec = StripeDecoder(W, H)
        for _, _, _, data in packets:
            dec.feed(data)
        return dec.Y, dec.U, dec.V
    (_, _, _, data), = packets
    if codec == "hevc":
        from selkies_gstreamer_amd.models.hevc.decoder import HevcDecoder
        pic, = HevcDecoder().decode(data[10:])
        return tuple(pic)
    from selkies_gstreamer_amd.models.av1 import dav1d
    return tuple(dav1d.Decoder().decode(data[10:]))


@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", CODECS)
def test_colour_signalling(codec, full_range):
    """Every sequence header announces the requested range and BT.709 (1, 1, 1): the first packet of
    the picture, and for H.264 in stripes the SPS of every stripe."""
    stream = "h264" if codec == "h264ff" else codec
    cases = [patch_case(codec, full_range), plane_case(codec, full_range, (66, 18, 0))]
    for c in cases:
        packets = cpu_run(c)[0].packets
        stripes = (c.H + stripe_height(c) - 1) // stripe_height(c) if codec == "h264" else 1
        assert len(packets) == stripes
        for y, _, key, data in packets:
            assert key, "the first frame starts every stream"
            assert fm.colour_signal(stream, data) == (full_range, 1, 1, 1), f"{codec} stripe at {y}"
    if stream == "h264":   # the project's decoder reads the same flag
        from selkies_gstreamer_amd.models.h264.decoder import BitReader, parse_sps, split_annexb, unescape
        sps = next(n for n in split_annexb(packets[0][3][10:]) if n[0] & 31 == 7)
        assert parse_sps(BitReader(unescape(sps[1:])))[1].full_range == int(full_range)


@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_colour_round_trip(codec, full_range):
    """Flat patches coded at QP 4 and decoded by the codec's independent decoder come back, through
    the float64 inverse BT.709 of the range the stream announces, within 3 levels of the source in
    every channel; read with the other range, black or white is more than 10 levels off.
    Measured on the CPU back end, the same for all three codecs (at QP 4 the flat patches are coded
    without loss, so what remains is the rounding of the conversion): limited range, worst patch
    1.22, black / white read as full range 16.00 / 20.00 off; full range, worst patch 1.70, black /
    white read as limited range 18.63 / 23.29 off."""
    if codec == "av1":
        from selkies_gstreamer_amd.models.av1 import dav1d
        if not dav1d.available():
            pytest.skip("dav1d (Pillow's libavif) not available")
    c = patch_case(codec, full_range)
    packets = cpu_run(c)[0].packets
    signalled = fm.colour_signal(codec, packets[0][3])[0]
    Y, U, V = decode(codec, c.W, c.H, packets)
    right, wrong = [], []
    for i, (r, g, b) in enumerate(PATCHES):
        cy, cx = i // PATCH_COLS * PATCH + PATCH // 2, i % PATCH_COLS * PATCH + PATCH // 2
        s = (float(Y[cy, cx]), float(U[cy // 2, cx // 2]), float(V[cy // 2, cx // 2]))
        right.append(np.abs(rgb_of(*s, signalled) - (r, g, b)).max())
        wrong.append(np.abs(rgb_of(*s, not signalled) - (r, g, b)).max())
    print(f"{codec} {case_id(full_range)}: worst patch {max(right):.2f}, black / white in the other range "
          f"{wrong[0]:.2f} / {wrong[1]:.2f}")
    assert max(right) <= 3.0, [round(float(e), 2) for e in right]
    assert max(wrong[0], wrong[1]) > 10.0, wrong[:2]


@pytest.mark.gpu
@pytest.mark.parametrize("full_range", RANGES, ids=case_id)
@pytest.mark.parametrize("codec", STREAMS)
def test_colour_patches_hip(codec, full_range):
    """The HIP back end's stream of the patch frame is the CPU back end's, byte for byte: what the
    two tests above establish holds for it."""
    check_hip(patch_case(codec, full_range))
