"""AV1 chroma palettes on intra blocks (Av1Encoder(chroma_palette=True); av1_core.h
code_palette_mode_info / code_palette_tokens_uv, av1_cpu.cpp intra_code) on the CPU back end. Every
temporal unit goes through dav1d and must equal the encoder's reconstruction in all planes
(tests/av1_chroma_palette_util.py)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import Av1Encoder
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
from tests import av1_chroma_palette_util as C
from tests import av1_intra_inter_util as U
from tests.av1_ltr_util import CheckedAv1, av1_enc, contents, sequence
from tests.ltr_util import H as LH, W as LW

pytestmark = pytest.mark.skipif(not dav1d.available(), reason="dav1d (Pillow's libavif) not found")

QP = 25   # the premise of test_gain_in_inter_frames holds at qp 25 (asserted there)
_runs = {}


def _window_run(w, h, on):
    """The window sequence (av1_intra_inter_util.frames) with intra_inter, chroma palettes on or off,
    coded once and shared."""
    if (w, h, on) not in _runs:
        enc = Av1Encoder(w, h, backend="cpu", qp=QP, intra_inter=True, chroma_palette=on)
        _runs[(w, h, on)] = C.run(enc, w, h, U.frames(w, h))
    return _runs[(w, h, on)]


def test_option_off_equals_absence():
    W, H = 256, 128
    for kind in ("desktop", "motion"):
        src = SyntheticDesktop(W, H, kind=kind)
        a, b = Av1Encoder(W, H, backend="cpu", chroma_palette=False), Av1Encoder(W, H, backend="cpu")
        for t in range(4):
            f = src.frame(t)
            assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], (kind, t)


def test_pairs_picture():
    """The designed pair sets of the key frame: a, b, c, d and the g / h neighbours carry their pair
    count, their pairs sorted by (U, V) in the palette cells, and reconstruct chroma exactly; nine
    pairs and one pair carry no palette."""
    W, H = C.PAIRS_W, C.PAIRS_H
    o = C.run(Av1Encoder(W, H, backend="cpu", qp=QP, chroma_palette=True), W, H, [C.pairs_picture()])[0]
    n = o["cells"][:, :, C.BLK_PAL_N] >> 4
    assert o["key"] and (o["cells"][:, :, C.BLK_PAL_N] & 15 == 0).all()   # flat luma: no luma palette
    expect = np.zeros_like(n)
    for (r, c), (name, pairs) in C.PAIR_SETS.items():
        k = len(pairs) if 2 <= len(pairs) <= 8 else 0
        expect[2 * r:2 * r + 2, 2 * c:2 * c + 2] = k
        got = n[2 * r:2 * r + 2, 2 * c:2 * c + 2]
        assert (got == k).all(), f"set {name}: PaletteSizeUV {got.tolist()}, expected {k}"
        if not k:
            continue
        for p in (1, 2):
            assert np.array_equal(o["rec"][p][8 * r:8 * r + 8, 8 * c:8 * c + 8],
                                  o["src"][p][8 * r:8 * r + 8, 8 * c:8 * c + 8]), f"set {name}: plane {p} is not exact"
        cell = o["pal_uv"][2 * r, 2 * c]
        assert list(zip(cell[:k].tolist(), cell[8:8 + k].tolist())) == sorted(pairs), name
    assert np.array_equal(n, expect)   # and no palette in the flat units
    names = {name: len(p) for name, p in C.PAIR_SETS.values()}
    assert (names["a"], names["b"], names["c"], names["d"], names["e"], names["f"]) == (2, 4, 2, 8, 9, 1)


def test_glyph_field_edge_blocks():
    """72x72: the last column and row are 8x8 blocks whose chroma palettes have 4x4 index maps."""
    W = H = 72
    o = C.run(Av1Encoder(W, H, backend="cpu", qp=QP, chroma_palette=True), W, H, [C.glyph_field(W, H)])[0]
    n = o["cells"][:, :, C.BLK_PAL_N] >> 4
    bsl = o["cells"][:, :, C.BLK_BSL]
    assert (bsl[:, 8] == 1).all() and (bsl[8, :] == 1).all() and (bsl[:8, :8] == 2).all()
    assert (n[:8, 8] >= 2).all() and (n[8, :] >= 2).all(), n.tolist()
    assert (n[:8, :8] >= 2).all() and n.max() <= 5     # two RGB colours: at most five pairs per block
    for p in (1, 2):
        assert np.array_equal(o["rec"][p], o["src"][p])


@pytest.mark.parametrize("w,h,kw", [(200, 120, {}), (512, 320, dict(tile_cols_log2=2, tile_rows_log2=1))])
def test_tiles(w, h, kw):
    """A key frame and an inter frame (intra_inter) of the glyph field: chroma palettes in every tile,
    the cache and the colour contexts bounded by the tiles (dav1d in C.run)."""
    enc = Av1Encoder(w, h, backend="cpu", qp=QP, intra_inter=True, chroma_palette=True, **kw)
    out = C.run(enc, w, h, [C.glyph_field(w, h), C.glyph_field(w, h, 2)])
    assert [o["key"] for o in out] == [True, False]
    geo = enc.debug_buffer("av1_geo", np.int32)
    n = out[0]["cells"][:, :, C.BLK_PAL_N] >> 4
    tc, tr = 1 << kw.get("tile_cols_log2", 0), 1 << kw.get("tile_rows_log2", 0)
    if kw:
        assert int((geo == tc).sum()) >= 1 and int((geo == tr).sum()) >= 1
    rows, cols = n.shape
    for y in range(tr):
        for x in range(tc):
            tile = n[y * rows // tr:(y + 1) * rows // tr, x * cols // tc:(x + 1) * cols // tc]
            assert (tile >= 2).any(), (x, y)
    c1 = out[1]["cells"]
    intra = (c1[:, :, C.BLK_FLAGS] & 1) == 0
    assert intra.any() and (c1[intra][:, C.BLK_PAL_N] >> 4 >= 2).any()
    assert (c1[~intra][:, C.BLK_PAL_N] == 0).all()


@pytest.mark.parametrize("w,h", [(256, 128), (640, 360)])
def test_gain_in_inter_frames(w, h):
    """The window sequence with intra_inter: the window frame holds intra cells with a chroma palette,
    inter cells none; the window frame and the key frame are smaller with the option and their chroma
    error over the window's two-colour part (key frame: the same region of the desktop) is not larger.
    Premise, asserted first: without the option that chroma error is above zero at qp 25."""
    on, off = _window_run(w, h, True), _window_run(w, h, False)
    m = U.two_colour_mask(w, h)
    assert [o["key"] for o in on] == [True, False, False, False, False]
    for t in (U.WINDOW_FRAME, 0):
        e_on, e_off = C.chroma_sse(on[t]["src"], on[t]["rec"], m), C.chroma_sse(off[t]["src"], off[t]["rec"], m)
        print(f"{w}x{h} frame {t}: {on[t]['bytes']} bytes on, {off[t]['bytes']} off; chroma SSE {e_on} on, {e_off} off")
        assert e_off > 0, "premise: the DCT chroma of the off encoder is lossy at qp 25"
        assert (off[t]["cells"][:, :, C.BLK_PAL_N] >> 4 == 0).all()
        assert on[t]["bytes"] < off[t]["bytes"]
        assert e_on <= e_off
    c = on[U.WINDOW_FRAME]["cells"]
    intra = (c[:, :, C.BLK_FLAGS] & 1) == 0
    assert (c[intra][:, C.BLK_PAL_N] >> 4 >= 2).any()
    assert (c[~intra][:, C.BLK_PAL_N] == 0).all()
    for o in on[1:]:
        inter = (o["cells"][:, :, C.BLK_FLAGS] & 1) == 1
        assert (o["cells"][inter][:, C.BLK_PAL_N] == 0).all()


def cbr_frames(w, h, content):
    """(frames, kbit/s): the window sequence over the plain wallpaper at U.CBR_KBPS. The grey window's
    chroma stays DCT at the QP its re-code ends at, so content "glyphs" adds a 64x32 patch of the
    strongly coloured glyph field in the window's corner, at a rate with one re-code pass after
    which chroma palettes still pay (CPU encoder: final qindex 150)."""
    seq = U.frames(w, h, U.wallpaper(w, h))
    if content == "glyphs":
        x0, y0, _, _ = U.window_rect(w, h)
        for k, f in enumerate(seq[U.WINDOW_FRAME:]):
            f[y0:y0 + 32, x0:x0 + 64] = C.glyph_field(64, 32, 3 * k)
    return seq, U.CBR_KBPS if content == "window" else 450


@pytest.mark.parametrize("content", ["window", "glyphs"])
def test_recode_under_cbr(content):
    """CBR at a rate the window frame overflows: the re-code passes redo the chroma decision from
    clean cells, and the stream still decodes exactly. The glyph patch keeps chroma palettes at the
    QP the passes end at."""
    W, H = 256, 128
    seq, kbps = cbr_frames(W, H, content)
    enc = Av1Encoder(W, H, backend="cpu", intra_inter=True, chroma_palette=True, rate_control="cbr",
                     bitrate_kbps=kbps, fps=60.0)
    redos = []
    out = C.run(enc, W, H, seq, lambda t, e, r: redos.append(e.rc_stats()["redos"]))
    assert not out[U.WINDOW_FRAME]["key"]
    assert redos[U.WINDOW_FRAME] > redos[U.WINDOW_FRAME - 1], redos
    if content == "glyphs":
        assert (out[U.WINDOW_FRAME]["cells"][:, :, C.BLK_PAL_N] >> 4 >= 2).any()


def test_with_ltr_slots():
    """ltr_slots = 2 on A -> B -> A with a glyph field opening in the top tile row of the switch
    back: intra blocks with chroma palettes next to blocks that read the cached picture."""
    run = CheckedAv1(av1_enc(2, intra_inter=True, chroma_palette=True))
    for _, _, f in sequence("A10 B10"):
        run.step(f)
    back = contents()["A"].copy()
    back[8:48, 48:144] = C.glyph_field(96, 40)
    o = run.step(back)
    assert not o["key"] and o["slots"][0] >= 0, o["slots"]
    intra = U.check_intra_cells(run.enc, LW, LH)
    n = C.uv_count(run.enc, LW, LH)
    assert intra[:8].any() and (n[intra] >= 2).any() and (n[~intra] == 0).all()
    for _ in range(2):
        assert not run.step(back)["key"]


def test_capture_session_carries_the_option():
    """pixelflux capture session (CPU backend, AV1) over a pool of the glyph field: the key frame with
    CaptureSettings.av1_chroma_palette equals the bare encoder's with chroma_palette=True and is smaller
    than the session's without it."""
    import ctypes
    import threading

    import pixelflux
    from selkies_gstreamer_amd.ops.native import PinnedBuffer
    W, H = 200, 120
    pool = PinnedBuffer((1, H, W, 4))
    pool.array[0] = C.glyph_field(W, H)
    sizes = {}
    for on in (0, 1):
        got, lock = [], threading.Lock()

        def on_frame(res, n, user):
            with lock:
                got.append([ctypes.string_at(res[i].data, res[i].size) for i in range(n)])

        s = pixelflux.default_settings(W, H, use_cpu=1, source=pixelflux.SOURCE_POOL, step_mode=1, pool_frames=1,
                                       pool_stride=W * 4, use_paint_over_quality=0, h264_crf=QP, h264_rc_mode=0,
                                       output_mode=3, av1_chroma_palette=on)
        s.pool = pool.array.ctypes.data
        cap = pixelflux.ScreenCapture()
        cb = pixelflux.FrameCallback(on_frame)
        cap.start_frame_capture(s, cb)
        cap.run(1)
        assert cap.wait(120_000) == 0
        cap.close()
        assert len(got) == 1 and len(got[0]) == 1
        assert dav1d.Decoder().decode(got[0][0][10:]) is not None
        sizes[on] = len(got[0][0])
    assert sizes[1] < sizes[0], sizes


def test_server_reads_the_variable(monkeypatch):
    from selkies_gstreamer_amd.server.data_server import _av1_chroma_palette_from_env
    monkeypatch.delenv("SELKIES_AV1_CHROMA_PALETTE", raising=False)
    assert _av1_chroma_palette_from_env() == 0
    monkeypatch.setenv("SELKIES_AV1_CHROMA_PALETTE", "1")
    assert _av1_chroma_palette_from_env() == 1
    monkeypatch.setenv("SELKIES_AV1_CHROMA_PALETTE", "off")
    assert _av1_chroma_palette_from_env() == 0
