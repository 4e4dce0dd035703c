"""AV1 intra blocks and luma palettes in inter frames (Av1Encoder(intra_inter=True); av1_core.h
code_block, av1_cpu.cpp intra_trial) on the CPU back end: a window that opens over a desktop is
coded as intra / palette blocks where that is cheaper than the inter residual. Every temporal
unit goes through dav1d and must equal the encoder's reconstruction in all planes
(tests/av1_intra_inter_util.py)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import Av1Encoder
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
from tests import av1_intra_inter_util as U
from tests.av1_ltr_util import CheckedAv1, av1_enc, blk_refs, contents, sequence
from tests.ltr_util import H as LH, W as LW

pytestmark = pytest.mark.skipif(not dav1d.available(), reason="dav1d (Pillow's libavif) not found")

SIZES = [(64, 64, {}), (200, 120, {}), (512, 320, dict(tile_cols_log2=2, tile_rows_log2=1)), (640, 360, {})]

_runs = {}


def _run(w, h, on, **kw):
    """Each checked CQP run of the sequence once: per frame the packet, the reconstruction, the
    cells and the source luma. The tests share the results and leave them unchanged."""
    k = (w, h, on, tuple(sorted(kw.items())))
    if k not in _runs:
        enc = Av1Encoder(w, h, backend="cpu", qp=25, intra_inter=on, **kw)

        def hook(t, e, r):
            r["cells"] = U.cells(e, w, h).copy()
            r["src_y"] = U.src_luma(e, w, h)
            if on and not r["key"]:
                U.check_intra_cells(e, w, h)
        _runs[k] = U.run(enc, w, h, U.frames(w, h), hook)
    return _runs[k]


def test_option_off_equals_absence():
    W, H = 256, 128
    for kind in ("desktop", "motion"):
        src = SyntheticDesktop(W, H, kind=kind)
        a, b = Av1Encoder(W, H, backend="cpu", intra_inter=False), Av1Encoder(W, H, backend="cpu")
        for t in range(4):
            f = src.frame(t)
            assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], (kind, t)


@pytest.mark.parametrize("w,h,kw", SIZES)
def test_window_frame_cells(w, h, kw):
    """Frame 2 is an inter frame with intra blocks inside the window and none outside it, palette
    blocks and transform blocks among them; no intra cell names a reference, has a vector or lies
    in a merged block (U.check_intra_cells, in _run's hook)."""
    out = _run(w, h, True, **kw)
    assert [o["key"] for o in out] == [True, False, False, False, False]
    c = out[U.WINDOW_FRAME]["cells"]
    intra = (c[:, :, U.BLK_FLAGS] & 1) == 0
    assert intra.any() and not (intra & ~U.window_cells(w, h)).any()
    assert (c[intra][:, U.BLK_PAL_N] > 0).any() and (c[intra][:, U.BLK_PAL_N] == 0).any()
    assert (c[intra][:, U.BLK_PAD1] == 0).all() and (c[intra][:, 4:8] == 0).all()
    assert not (intra & (c[:, :, 0] >= 3)).any()


@pytest.mark.parametrize("w,h,kw", SIZES)
def test_gain_on_the_window_frame(w, h, kw):
    """At CQP the window frame is smaller with the option and its luma error over the window's
    two-colour part is not larger: a palette block is luma-lossless, the off encoder's inter
    residual at qp 25 is neither lossless nor a skip there (the premise, checked first)."""
    on, off = _run(w, h, True, **kw)[U.WINDOW_FRAME], _run(w, h, False, **kw)[U.WINDOW_FRAME]
    m = U.two_colour_mask(w, h)

    def sse(o):
        return int((((o["src_y"].astype(np.int32) - o["rec"][0].astype(np.int32)) ** 2)[m]).sum())
    cells_m = U.window_cells(w, h)
    off_flags = off["cells"][:, :, U.BLK_FLAGS]
    assert (off_flags & 1).all(), "the off encoder coded an intra block"
    assert sse(off) > 0 and ((off_flags[cells_m] & 2) == 0).any(), "premise: off is lossy and not a skip in the window"
    print(f"{w}x{h} window frame: {on['bytes']} bytes on, {off['bytes']} bytes off; "
          f"two-colour luma SSE {sse(on)} on, {sse(off)} off")
    assert on["bytes"] < off["bytes"]
    assert sse(on) <= sse(off)


def test_with_ltr_slots():
    """ltr_slots = 2 on A -> B -> A: the switch back reads the cached picture (LAST2) in both tile
    rows while a window opens in the top one: intra blocks next to LAST2 blocks (BlkInfo.pad1 is the
    inter block's reference and must be 0 in an intra block)."""
    run = CheckedAv1(av1_enc(2, intra_inter=True))
    for _, _, f in sequence("A10 B10"):
        run.step(f)
    back = contents()["A"].copy()
    ww, wh = 84, 34
    win = U.draw_window(np.zeros((int(wh / 0.55) + 1, int(ww / 0.6) + 1, 4), np.uint8))
    x0, y0, w2, h2 = U.window_rect(win.shape[1], win.shape[0])
    back[10:10 + h2, 52:52 + w2] = win[y0:y0 + h2, x0:x0 + w2]
    o = run.step(back)
    assert not o["key"] and o["slots"][0] >= 0, o["slots"]
    intra = U.check_intra_cells(run.enc, LW, LH)
    refs = blk_refs(run.enc, LW, LH)
    assert intra[:8].any() and not intra[8:].any()
    assert (refs[:8][~intra[:8]] == 1).all(), "the top tile row's inter blocks read LAST2"
    assert (U.cells(run.enc, LW, LH)[intra][:, U.BLK_PAL_N] > 0).any()
    for _ in range(2):
        assert not run.step(back)["key"]


def test_recode_under_cbr():
    """CBR at a rate the window frame overflows: the K10 re-code passes redo the decision from
    clean cells, and the stream still decodes exactly."""
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", intra_inter=True, rate_control="cbr", bitrate_kbps=U.CBR_KBPS, fps=60.0)
    redos, intra = [], []

    def hook(t, e, r):
        redos.append(e.rc_stats()["redos"])
        intra.append(0 if r["key"] else int(U.check_intra_cells(e, W, H).sum()))
    out = U.run(enc, W, H, U.frames(W, H, U.wallpaper(W, H)), hook)
    assert not out[U.WINDOW_FRAME]["key"] and intra[U.WINDOW_FRAME] > 0, intra
    assert redos[U.WINDOW_FRAME] > redos[U.WINDOW_FRAME - 1], redos


def _tile_payloads(tu: bytes) -> bytes:
    """The payload of a temporal unit's OBU_FRAME: frame header, then the tiles."""
    i = 0
    while i < len(tu):
        typ = (tu[i] >> 3) & 15
        n, j, s = 0, i + 1, 0
        while True:
            n |= (tu[j] & 0x7f) << s
            s += 7
            j += 1
            if not tu[j - 1] & 0x80:
                break
        if typ == 6:
            return tu[j:j + n]
        i = j + n
    raise AssertionError("no OBU_FRAME")


def test_static_content():
    """Four identical frames: no candidates, so no intra cell in any inter frame, and the frames
    equal the option-off ones except for the header's allow_screen_content_tools bit."""
    W, H = 256, 128
    f = SyntheticDesktop(W, H, kind="desktop").frame(0)
    on, off = Av1Encoder(W, H, backend="cpu", intra_inter=True), Av1Encoder(W, H, backend="cpu")
    for t in range(4):
        a, b = bytes(on.encode(f, t)[0].data), bytes(off.encode(f, t)[0].data)
        if t == 0:
            assert a == b
            continue
        assert not U.intra_cells(on, W, H).any()
        pa, pb = _tile_payloads(a[10:]), _tile_payloads(b[10:])
        # inter frame header: show_existing_frame, frame_type (2), show_frame, error_resilient_mode,
        # disable_cdf_update, allow_screen_content_tools: bit 6 of the first payload byte
        assert len(a) == len(b) and pa[0] == pb[0] | 0x02 and pa[1:] == pb[1:], t
