"""AV1 intra blocks and luma palettes in inter frames on the HIP back end (k_av1_inter with the
inter coding's J, k_av1_cand_modes, k_av1_inter_intra) against the CPU reference encoder with the
option on: identical cells, reconstruction and temporal units byte for byte, and dav1d decodes
the GPU stream to the GPU's reconstruction (all planes)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, hip_device_count
from tests import av1_intra_inter_util as U
from tests.av1_ltr_util import contents, sequence
from tests.av1_ltr_util import blk_refs
from tests.ltr_util import STRIPE, ref_planes

pytestmark = pytest.mark.gpu


def _pair(W, H, **kw):
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    kw = dict(dict(intra_inter=True), **kw)
    return Av1Encoder(W, H, backend="hip", **kw), Av1Encoder(W, H, backend="cpu", **kw)


def _check(W, H, seq, want_intra=(U.WINDOW_FRAME,), **kw):
    """HIP == CPU on every frame of seq; want_intra: frames that must hold intra cells.
    Returns the rate-control statistics of both encoders."""
    gpu, cpu = _pair(W, H, **kw)
    ck = U.Checked(gpu, W, H)      # dav1d on the GPU stream
    top = (H // 2 + 7) // 8 if kw.get("ltr_slots") else 0    # cell rows of the first of two tile rows
    for t, f in enumerate(seq):
        og = ck.step(f)
        pc = cpu.encode(f, t)
        bg = gpu.debug_buffer("blk").reshape(-1, 12)
        bc = cpu.debug_buffer("blk").reshape(-1, 12)
        bad = np.argwhere((bg != bc).any(axis=1))
        assert len(bad) == 0, f"frame {t}: {len(bad)} cells differ, first {bad[:3].ravel().tolist()} " \
                              f"gpu {bg[bad[0][0]].tolist()} cpu {bc[bad[0][0]].tolist()}"
        for a, b, n in zip(og["rec"], ref_planes(cpu, W, H), "YUV"):
            assert np.array_equal(a, b), f"frame {t}: {n} reconstruction differs at {np.argwhere(a != b)[:3].tolist()}"
        assert og["data"] == bytes(pc[0].data), f"frame {t}: bitstream differs"
        if not og["key"]:
            intra = U.check_intra_cells(gpu, W, H)
            if t in want_intra:
                assert intra.any(), f"frame {t}: no intra cell"
                if top:   # the window's tile row reads the cached picture: intra blocks among LAST2 blocks
                    refs = blk_refs(gpu, W, H)
                    assert intra[:top].any() and (refs[:top][~intra[:top]] == 1).all()
    return gpu.rc_stats(), cpu.rc_stats()


@pytest.mark.parametrize("W,H,kw", [(64, 64, {}), (200, 120, {}),
                                    (512, 320, dict(tile_cols_log2=2, tile_rows_log2=1)), (640, 360, {})])
def test_gpu_matches_cpu(W, H, kw):
    _check(W, H, U.frames(W, H), qp=25, **kw)


def test_gpu_with_ltr_slots():
    """256x128, ltr_slots = 2: A -> B -> A with a window in the tile row that reads LAST2."""
    W, H = 256, 128
    seq = [f for _, _, f in sequence("A10 B10", W, H)]
    back = contents(W, H)["A"].copy()
    win = U.draw_window(np.zeros((64, 142, 4), np.uint8))
    x0, y0, w2, h2 = U.window_rect(142, 64)
    back[10:10 + h2, 52:52 + w2] = win[y0:y0 + h2, x0:x0 + w2]
    seq += [back, back]
    _check(W, H, seq, want_intra=(20,), qp=24, stripe_height=STRIPE, use_paint_over=False, ltr_slots=2)


def test_gpu_recode_under_cbr():
    """256x128 CBR over the plain wallpaper: the gated re-code passes redo k_av1_inter,
    k_av1_cand_modes and k_av1_inter_intra; the same passes as the CPU encoder's."""
    W, H = 256, 128
    sg, sc = _check(W, H, U.frames(W, H, U.wallpaper(W, H)), rate_control="cbr", bitrate_kbps=U.CBR_KBPS, fps=60.0)
    assert sg == sc and sg["redos"] > 0, (sg, sc)


def test_gpu_1080p():
    """Frames 1..3 at 1080p (frame 0 of the run is the key frame): tiles hold more units on an
    anti-diagonal than the workgroup of k_av1_inter_intra has waves."""
    W, H = 1920, 1080
    _check(W, H, U.frames(W, H)[1:4], want_intra=(1,), qp=25)
