"""AV1 clustered luma palettes with a residual (Av1Encoder(palette_cluster=True); av1_core.h
palette_cluster / palette_nearest, av1_cpu.cpp intra_code) on the CPU back end. Every temporal unit
goes through dav1d and must equal the encoder's reconstruction in all planes (Checked of
tests/av1_chroma_palette_util.py)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import Av1Encoder, H264Encoder
from tests import av1_chroma_palette_util as C
from tests import av1_intra_inter_util as U
from tests import av1_palette_cluster_util as P
from tests.av1_ltr_util import contents, sequence
from tests.ltr_util import STRIPE

pytestmark = pytest.mark.skipif(not dav1d.available(), reason="dav1d (Pillow's libavif) not found")

QP = 20
CBR_KBPS = 600   # the anti-aliased window frame overflows its cap at this rate and is coded again
_runs = {}


def _run(key, make):
    if key not in _runs:
        _runs[key] = make()
    return _runs[key]


def _qidx(enc) -> int:
    return int(enc.debug_buffer("av1_qidx").view(np.int32)[0])


def step(ck: C.Checked, frame) -> dict:
    """One frame through a Checked encoder, with the luma palette cells and the frame's qindex."""
    o = ck.step(frame)
    o["pal"] = P.pal_y(ck.enc, ck.w, ck.h).copy()
    o["qidx"] = _qidx(ck.enc)
    return o


def run(enc, w, h, seq, hook=None) -> list:
    ck = C.Checked(enc, w, h)
    out = []
    for t, f in enumerate(seq):
        out.append(step(ck, f))
        if hook:
            hook(t, enc, out[-1])
    return out


def clustered(o) -> np.ndarray:
    """Cells of luma palette blocks whose source holds more than eight values."""
    return P.clustered(o["src"][0], o["cells"])


def check_palettes(o):
    """Every luma palette of the frame: 2..8 strictly ascending colours; a clustered block's colours are
    the model's, an exact block's the source values."""
    cells, pal, sy = o["cells"], o["pal"], o["src"][0]
    n = P.pal_n(cells)
    cl = clustered(o)
    for r, c in np.argwhere(n > 0):
        k = int(n[r, c])
        col = pal[r, c, :k].astype(int).tolist()
        assert 2 <= k <= P.PAL_MAX and all(a < b for a, b in zip(col, col[1:])), (r, c, col)
        if cells[r, c, 0] >= 2:
            blk = sy[(r & ~1) * 8:(r & ~1) * 8 + 16, (c & ~1) * 8:(c & ~1) * 8 + 16]
        else:
            blk = sy[r * 8:r * 8 + 8, c * 8:c * 8 + 8]
        if cl[r, c]:
            assert col == P.model_colours(blk, o["qidx"]), (r, c, col, P.model_colours(blk, o["qidx"]))
        else:
            assert col == np.unique(blk).tolist(), (r, c)


def _designed(on):
    W, H = P.DESIGN_W, P.DESIGN_H
    return _run(("designed", on), lambda: run(Av1Encoder(W, H, backend="cpu", qp=QP, palette_cluster=on), W, H,
                                              [P.designed_picture()])[0])


def test_designed_picture():
    on, off = _designed(True), _designed(False)
    assert on["key"]
    check_palettes(on)
    n, cl = P.pal_n(on["cells"]), clustered(on)
    for (r, c), (name, vals) in P.UNITS.items():
        unit = (slice(2 * r, 2 * r + 2), slice(2 * c, 2 * c + 2))
        print(f"unit {(r, c)} {name}: pal_n {n[2 * r, 2 * c]} colours {on['pal'][2 * r, 2 * c].tolist()}")
        if (r, c) in P.CLUSTERED:
            assert cl[unit].all(), (r, c, name)
        elif name == "eight":
            assert (n[unit] == 8).all() and on["pal"][2 * r, 2 * c].tolist() == vals
        else:    # the gradient and the flat unit
            assert (n[unit] == 0).all(), (r, c, name)
    two = 2 * np.array([u for u, (nm, _) in P.UNITS.items() if nm.startswith("two")])
    assert (n[two[:, 0], two[:, 1]] == 2).all()     # two tight groups: two colours
    assert not clustered(off).any()
    assert on["bytes"] < off["bytes"]


def _aa72(on):
    return _run(("aa72", on), lambda: run(Av1Encoder(72, 72, backend="cpu", qp=QP, intra_inter=True, palette_cluster=on),
                                          72, 72, [P.aa_field(72, 72, 0), P.aa_field(72, 72, 3)]))


def test_aa_field_edge_blocks():
    """72x72, a key frame and an inter frame: 8x8 blocks in the last column and row."""
    on, off = _aa72(True), _aa72(False)
    assert [o["key"] for o in on] == [True, False]
    for t in (0, 1):
        check_palettes(on[t])
        cl = clustered(on[t])
        assert cl.any(), t
        assert not clustered(off[t]).any()
    bsl = on[0]["cells"][:, :, C.BLK_BSL]
    edge = (clustered(on[0]) | clustered(on[1])) & (bsl == 1)
    print(f"clustered 8x8 cells: {int(edge.sum())}")
    assert edge[:, -1].any() or edge[-1, :].any()


def test_two_colour_window_is_unchanged():
    """The window sequence of av1_intra_inter_util: no block outside the gradient band has more than
    eight values, and the band stays off, so every byte is the option-off encoder's."""
    W, H = 256, 128
    a = Av1Encoder(W, H, backend="cpu", qp=25, intra_inter=True, palette_cluster=True)
    b = Av1Encoder(W, H, backend="cpu", qp=25, intra_inter=True)
    for t, f in enumerate(U.frames(W, H)):
        assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], t
        assert np.array_equal(C.cells(a, W, H), C.cells(b, W, H)), t


def test_default_is_off():
    W, H = 128, 64
    a, b = Av1Encoder(W, H, backend="cpu", qp=QP), Av1Encoder(W, H, backend="cpu", qp=QP, palette_cluster=False)
    for t in range(2):
        f = P.aa_field(W, H, 3 * t)
        assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], t


@pytest.mark.parametrize("content", ["aa", "soft"])
def test_fewer_bytes_and_higher_psnr(content):
    """A key frame and two shifted frames at 256x128, qp 20: strictly fewer bytes and strictly higher
    luma PSNR than with the option off."""
    W, H = 256, 128
    seq = P.shifted_frames(P.CONTENTS[content], W, H)
    res = {}
    for on in (False, True):
        out = run(Av1Encoder(W, H, backend="cpu", qp=QP, intra_inter=True, palette_cluster=on), W, H, seq)
        res[on] = (sum(o["bytes"] for o in out), float(np.mean([P.luma_psnr(o["src"], o["rec"]) for o in out])))
        if on:
            assert all(clustered(o).any() for o in out)
    print(f"{content}: off {res[False][0]} bytes / {res[False][1]:.2f} dB, on {res[True][0]} bytes / {res[True][1]:.2f} dB")
    assert res[True][0] < res[False][0] and res[True][1] > res[False][1]


def test_with_chroma_tools():
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", qp=QP, intra_inter=True, chroma_palette=True, cfl=True, palette_cluster=True)
    out = run(enc, W, H, P.shifted_frames(P.aa_field, W, H))
    for t, o in enumerate(out):
        check_palettes(o)
        assert clustered(o).any(), t
    c = out[0]["cells"]
    assert ((c[:, :, C.BLK_PAL_N] >> 4) >= 2).any() or (c[:, :, 2] == 13).any()   # a chroma palette or CfL occurs too


def ltr_frames(w, h):
    """A -> B -> A with an anti-aliased opening in the top tile row of the switch back."""
    seq = [f for _, _, f in sequence("A10 B10", w, h)]
    back = contents(w, h)["A"].copy()
    back[8:48, 48:144] = P.aa_field(96, 40)
    return seq + [back, back]


def test_with_ltr_slots():
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", qp=QP, stripe_height=STRIPE, use_paint_over=False, ltr_slots=2,
                     intra_inter=True, palette_cluster=True)
    out = run(enc, W, H, ltr_frames(W, H))
    o = out[20]
    assert not o["key"]
    check_palettes(o)
    assert clustered(o)[:8].any()
    c = o["cells"]
    assert (c[:, :, 11][(c[:, :, P.BLK_FLAGS] & 1) == 1] == 1).any(), "no block reads the cached picture"


def cbr_frames(w, h):
    return P.window_frames(w, h, U.wallpaper(w, h))


def test_recode_under_cbr():
    """CBR at a rate the window frame overflows: the re-code passes cluster again at their own qindex
    from clean cells, and the stream still decodes exactly."""
    W, H = 256, 128
    enc = Av1Encoder(W, H, backend="cpu", intra_inter=True, palette_cluster=True, rate_control="cbr",
                     bitrate_kbps=CBR_KBPS, fps=60.0)
    redos = []
    out = run(enc, W, H, cbr_frames(W, H), lambda t, e, r: redos.append(e.rc_stats()["redos"]))
    assert redos[-1] > 0, redos
    for o in out:
        check_palettes(o)
    assert any(clustered(o).any() for o in out)


def _capture(frame, output_mode, on):
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
                                   output_mode=output_mode, av1_palette_cluster=on)
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
    """CaptureSettings.av1_palette_cluster reaches the encoder through both C ABI structs: the session's
    key frame is the bare encoder's with palette_cluster=True, and differs from the session's without."""
    W, H = 200, 120
    f = P.aa_field(W, H)
    data = {on: _capture(f, 3, on) for on in (0, 1)}
    for on in (0, 1):
        assert len(data[on]) == 1 and dav1d.Decoder().decode(data[on][0][10:]) is not None
    bare = Av1Encoder(W, H, backend="cpu", qp=QP, palette_cluster=True).encode(f, 0)
    assert data[1][0][10:] == bytes(bare[0].data)[10:]
    assert len(data[1][0]) < len(data[0][0])


@pytest.mark.parametrize("output_mode", [1, 2], ids=["h264", "hevc"])
def test_other_sessions_ignore_the_option(output_mode):
    f = P.aa_field(128, 64)
    assert _capture(f, output_mode, 1) == _capture(f, output_mode, 0)


def test_server_reads_the_variable(monkeypatch):
    from selkies_gstreamer_amd.server.data_server import _av1_palette_cluster_from_env
    monkeypatch.delenv("SELKIES_AV1_PALETTE_CLUSTER", raising=False)
    assert _av1_palette_cluster_from_env() == 0
    monkeypatch.setenv("SELKIES_AV1_PALETTE_CLUSTER", "1")
    assert _av1_palette_cluster_from_env() == 1
    monkeypatch.setenv("SELKIES_AV1_PALETTE_CLUSTER", "off")
    assert _av1_palette_cluster_from_env() == 0


@pytest.mark.parametrize("codec", ["h264", "hevc"])
def test_other_codecs_ignore_the_option(codec):
    W, H = 128, 64
    a = H264Encoder(W, H, backend="cpu", codec=codec, av1_palette_cluster=True)
    b = H264Encoder(W, H, backend="cpu", codec=codec)
    for t in range(2):
        f = P.aa_field(W, H, 3 * t)
        assert [p.data for p in a.encode(f, t)] == [p.data for p in b.encode(f, t)], t


def test_shared_functions_clean_under_asan_ubsan(tmp_path):
    """palette_cluster, palette_nearest and palette_has_ramp (av1_core.h) in a stand-alone host program
    (tests/native/palette_cluster_harness.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer."""
    import os
    import shutil
    import subprocess
    from pathlib import Path
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not installed")
    root = Path(__file__).resolve().parents[1]
    exe = tmp_path / "palette_cluster_harness"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", f"-I{root / 'csrc'}", f"-I{root / 'csrc' / 'codec'}",
                        str(root / "tests" / "native" / "palette_cluster_harness.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "sanitized run ok" in r.stdout, (r.stdout + r.stderr)[-4000:]
