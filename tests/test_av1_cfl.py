"""AV1 chroma from luma on intra blocks (Av1Encoder(cfl=True); av1_core.h cfl_px / code_cfl_alphas,
av1_cpu.cpp intra_code) on the CPU back end. Every temporal unit goes through dav1d and must equal
the encoder's reconstruction in all planes (Checked of tests/av1_chroma_palette_util.py)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import Av1Encoder, H264Encoder
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
from tests import av1_cfl_util as K
from tests import av1_chroma_palette_util as C
from tests import av1_intra_inter_util as U
from tests.av1_ltr_util import contents, sequence
from tests.ltr_util import STRIPE

pytestmark = pytest.mark.skipif(not dav1d.available(), reason="dav1d (Pillow's libavif) not found")

QP = 25
# The alpha picture's conditions hold on the CPU encoder at qp 12: every designed unit keeps a chroma
# level under UV_DC_PRED (the magnitude-1 units swing +-12 about 128), and the luma reconstruction is
# close enough to the source for the search to find the designed alphas.
ALPHA_QP = 12
CBR_KBPS = 600   # the hue-texture window frame overflows its cap at this rate and is coded again
_runs = {}


def _run(key, make):
    if key not in _runs:
        _runs[key] = make()
    return _runs[key]


def _alpha(on):
    W, H = K.ALPHA_W, K.ALPHA_H
    return _run(("alpha", on), lambda: C.run(Av1Encoder(W, H, backend="cpu", qp=ALPHA_QP, cfl=on), W, H,
                                             [K.alpha_picture()])[0])


def _hue(w, h, on):
    return _run(("hue", w, h, on), lambda: C.run(Av1Encoder(w, h, backend="cpu", qp=QP, intra_inter=True, cfl=on), w, h,
                                                 [K.hue_texture(w, h, 0), K.hue_texture(w, h, 1)]))


def test_default_is_off():
    W, H = 256, 128
    for kind in ("desktop", "motion"):
        src = SyntheticDesktop(W, H, kind=kind)
        a, b = Av1Encoder(W, H, backend="cpu"), Av1Encoder(W, H, backend="cpu", cfl=False)
        for t in range(3):   # a key frame and two inter frames
            f = src.frame(t)
            assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], (kind, t)
            assert np.array_equal(C.cells(a, W, H), C.cells(b, W, H)), (kind, t)
            assert not K.is_cfl(C.cells(a, W, H)).any()


def test_alpha_picture():
    """Every designed unit takes CfL with the designed joint sign; magnitudes 1 and 16 occur; flat chroma
    and flat luma stay UV_DC_PRED; fewer bytes and less chroma error than with the option off."""
    on, off = _alpha(True), _alpha(False)
    assert on["key"]
    au, av = K.alphas(on["cells"])
    mode = K.uv_mode(on["cells"])
    mags = set()
    for (r, c), (du, dv, _) in K.DESIGN.items():
        cell = (2 * r, 2 * c)
        print(f"unit {(r, c)}: designed {(du, dv)}, coded mode {mode[cell]} alphas {(au[cell], av[cell])}")
        assert (mode[2 * r:2 * r + 2, 2 * c:2 * c + 2] == K.UV_CFL_PRED).all(), (r, c)
        assert (np.sign(au[cell]), np.sign(av[cell])) == (np.sign(du), np.sign(dv)), (r, c, au[cell], av[cell])
        mags |= {abs(int(au[cell])) - 1, abs(int(av[cell])) - 1}
    assert {(int(np.sign(u)), int(np.sign(v))) for u, v, _ in K.DESIGN.values()} == \
        {(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)} - {(0, 0)}     # all eight joint signs are designed
    assert 0 in mags and 15 in mags, mags
    for r, c in (K.ZERO_UNIT, K.FLAT_LUMA_UNIT):
        assert (mode[2 * r:2 * r + 2, 2 * c:2 * c + 2] == K.UV_DC_PRED).all(), (r, c)
    assert not K.is_cfl(off["cells"]).any()
    e_on, e_off = C.chroma_sse(on["src"], on["rec"]), C.chroma_sse(off["src"], off["rec"])
    print(f"bytes {on['bytes']} on, {off['bytes']} off; chroma SSE {e_on} on, {e_off} off")
    assert on["bytes"] < off["bytes"] and e_on < e_off


# 72x72 and 200x120: 8x8 blocks with 4x4 chroma in the last column and row. 204x124 is no multiple of
# 8: the encoder accepts it (the last cells hang over the picture edge).
@pytest.mark.parametrize("w,h", [(72, 72), (200, 120), (204, 124)])
def test_hue_texture_edge_blocks(w, h):
    on, off = _hue(w, h, True), _hue(w, h, False)
    assert [o["key"] for o in on] == [True, False]
    for t in (0, 1):
        c = on[t]["cells"]
        cfl = K.is_cfl(c)
        bsl = c[:, :, C.BLK_BSL]
        assert cfl.any(), t
        assert cfl[:, -1].any() and cfl[-1, :].any(), t   # the edge blocks
        if w % 16 == 8:     # 8x8 blocks there; at 204x124 the last blocks are 16x16 and hang over the edge
            assert (cfl[:, -1] & (bsl[:, -1] == 1)).any() and (cfl[-1, :] & (bsl[-1, :] == 1)).any(), t
        assert not K.is_cfl(off[t]["cells"]).any()
        print(f"{w}x{h} frame {t}: {on[t]['bytes']} bytes on, {off[t]['bytes']} off, {int(cfl.sum())} CfL cells")
        assert on[t]["bytes"] < off[t]["bytes"]
    inter = (on[1]["cells"][:, :, K.BLK_FLAGS] & 1) == 1
    assert (K.uv_mode(on[1]["cells"])[inter] != K.UV_CFL_PRED).all()


def test_inter_frames():
    """The window sequence with the window filled by hue texture: the window frame holds intra blocks
    with CfL; no inter cell has UV_CFL_PRED."""
    W, H = 256, 128
    out = C.run(Av1Encoder(W, H, backend="cpu", qp=QP, intra_inter=True, cfl=True), W, H, K.window_frames(W, H))
    assert [o["key"] for o in out] == [True, False, False, False, False]
    c = out[U.WINDOW_FRAME]["cells"]
    intra = (c[:, :, K.BLK_FLAGS] & 1) == 0
    assert intra.any() and (intra & U.window_cells(W, H)).sum() == intra.sum()
    assert K.is_cfl(c).any()
    for o in out[1:]:
        inter = (o["cells"][:, :, K.BLK_FLAGS] & 1) == 1
        assert (K.uv_mode(o["cells"])[inter] != K.UV_CFL_PRED).all()


def test_with_chroma_palette():
    """Glyph field in one half, hue texture in the other: both tools occur, never in one cell."""
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", qp=QP, intra_inter=True, chroma_palette=True, cfl=True)
    out = C.run(enc, W, H, [K.combined_picture(W, H, 0), K.combined_picture(W, H, 1)])
    for t, o in enumerate(out):
        c = o["cells"]
        cfl, pal = K.is_cfl(c), (c[:, :, K.BLK_PAL_N] >> 4) >= 2
        assert cfl.any() and pal.any(), t
        assert not (pal & (K.uv_mode(c) == K.UV_CFL_PRED)).any(), t


def test_tiles():
    """512x320 in 4x2 tiles: blocks at tile borders predict from dc 128 (dav1d in C.run)."""
    W, H = 512, 320
    enc = Av1Encoder(W, H, backend="cpu", qp=QP, intra_inter=True, cfl=True, tile_cols_log2=2, tile_rows_log2=1)
    out = C.run(enc, W, H, [K.hue_texture(W, H, 0), K.hue_texture(W, H, 1)])
    for o in out:
        cfl = K.is_cfl(o["cells"])
        rows, cols = cfl.shape
        for y in range(2):
            for x in range(4):
                assert cfl[y * rows // 2:(y + 1) * rows // 2, x * cols // 4:(x + 1) * cols // 4].any(), (x, y)


def cbr_frames(w, h):
    """The hue-texture window sequence over the plain wallpaper: a key frame so cheap that the window
    frame is the costly one for the rate controller."""
    return K.window_frames(w, h, U.wallpaper(w, h))


def test_recode_under_cbr():
    """CBR at a rate the window frame overflows: the re-code passes redo the CfL decision from clean
    cells, and the stream still decodes exactly."""
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", intra_inter=True, cfl=True, rate_control="cbr", bitrate_kbps=CBR_KBPS, fps=60.0)
    redos = []
    out = C.run(enc, W, H, cbr_frames(W, H), lambda t, e, r: redos.append(e.rc_stats()["redos"]))
    assert not out[U.WINDOW_FRAME]["key"]
    assert redos[U.WINDOW_FRAME] > redos[U.WINDOW_FRAME - 1], redos
    assert redos[-1] > 0
    assert any(K.is_cfl(o["cells"]).any() for o in out)


def ltr_frames(w, h):
    """A -> B -> A with a hue texture opening in the top tile row of the switch back."""
    seq = [f for _, _, f in sequence("A10 B10", w, h)]
    back = contents(w, h)["A"].copy()
    back[8:48, 48:144] = K.hue_texture(96, 40)
    return seq + [back, back]


def test_with_ltr_slots():
    """ltr_slots = 2: intra blocks with CfL next to blocks that read the cached picture."""
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", qp=24, stripe_height=STRIPE, use_paint_over=False, ltr_slots=2,
                     intra_inter=True, cfl=True)
    out = C.run(enc, W, H, ltr_frames(W, H))
    o = out[20]
    assert not o["key"]
    c = o["cells"]
    assert K.is_cfl(c)[:8].any()
    assert (c[:, :, 11][(c[:, :, K.BLK_FLAGS] & 1) == 1] == 1).any(), "no block reads the cached picture"


def _capture(frame, output_mode, av1_cfl):
    """The first frame's packets of a pixelflux capture session (CPU backend) over a one-frame pool."""
    import ctypes
    import threading

    import pixelflux
    from selkies_gstreamer_amd.ops.native import PinnedBuffer
    H, W = frame.shape[:2]
    pool = PinnedBuffer((1, H, W, 4))
    pool.array[0] = frame
    got, lock = [], threading.Lock()

    def on_frame(res, n, user):
        with lock:
            got.append([ctypes.string_at(res[i].data, res[i].size) for i in range(n)])

    s = pixelflux.default_settings(W, H, use_cpu=1, source=pixelflux.SOURCE_POOL, step_mode=1, pool_frames=1,
                                   pool_stride=W * 4, use_paint_over_quality=0, h264_crf=QP, h264_rc_mode=0,
                                   output_mode=output_mode, av1_cfl=av1_cfl)
    s.pool = pool.array.ctypes.data
    cap = pixelflux.ScreenCapture()
    cb = pixelflux.FrameCallback(on_frame)
    cap.start_frame_capture(s, cb)
    cap.run(1)
    assert cap.wait(120_000) == 0
    cap.close()
    assert len(got) == 1 and len(got[0]) >= 1
    return got[0]


def test_capture_session_carries_the_option():
    """AV1 capture session over the hue texture: the key frame with CaptureSettings.av1_cfl is the bare
    encoder's with cfl=True, and smaller than the session's without it."""
    W, H = 200, 120
    data = {on: _capture(K.hue_texture(W, H), 3, on) for on in (0, 1)}
    for on in (0, 1):
        assert len(data[on]) == 1 and dav1d.Decoder().decode(data[on][0][10:]) is not None
    assert len(data[1][0]) < len(data[0][0])
    assert data[1][0][10:] == _hue(W, H, True)[0]["data"][10:]


@pytest.mark.parametrize("output_mode", [1, 2], ids=["h264", "hevc"])
def test_other_sessions_ignore_the_option(output_mode):
    f = K.hue_texture(128, 64)
    assert _capture(f, output_mode, 1) == _capture(f, output_mode, 0)


def test_server_reads_the_variable(monkeypatch):
    from selkies_gstreamer_amd.server.data_server import _av1_cfl_from_env
    monkeypatch.delenv("SELKIES_AV1_CFL", raising=False)
    assert _av1_cfl_from_env() == 0
    monkeypatch.setenv("SELKIES_AV1_CFL", "1")
    assert _av1_cfl_from_env() == 1
    monkeypatch.setenv("SELKIES_AV1_CFL", "off")
    assert _av1_cfl_from_env() == 0


@pytest.mark.parametrize("codec", ["h264", "hevc"])
def test_other_codecs_ignore_the_option(codec):
    W, H = 128, 64
    a = H264Encoder(W, H, backend="cpu", codec=codec, av1_cfl=True)
    b = H264Encoder(W, H, backend="cpu", codec=codec)
    for t in range(2):
        f = K.hue_texture(W, H, t)
        assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], t
