"""AV1 chroma from luma on the HIP back end (the CfL pass of intra_rec_block, the alphas' syntax in
k_av1_tokens) against the CPU reference encoder with the option on: identical cells, reconstruction
and temporal units byte for byte (so the levels, through the bitstream), and dav1d decodes the GPU
stream to the GPU's reconstruction (all planes)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, hip_device_count
from tests import av1_cfl_util as K
from tests import av1_chroma_palette_util as C
from tests import av1_intra_inter_util as U
from tests.ltr_util import STRIPE, ref_planes
from tests.test_av1_cfl import ALPHA_QP, CBR_KBPS, QP, cbr_frames, ltr_frames

pytestmark = pytest.mark.gpu


def _pair(W, H, **kw):
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    kw = dict(dict(cfl=True), **kw)
    return Av1Encoder(W, H, backend="hip", **kw), Av1Encoder(W, H, backend="cpu", **kw)


def _check(W, H, seq, want_cfl=(0,), **kw):
    """HIP == CPU on every frame of seq (BGRx arrays or (Y, U, V) tuples); want_cfl: frames that must
    hold CfL blocks. Returns the rate-control statistics of both encoders."""
    gpu, cpu = _pair(W, H, **kw)
    ck = C.Checked(gpu, W, H)      # dav1d on the GPU stream
    for t, f in enumerate(seq):
        og = ck.step(f)
        pc = cpu.encode_yuv("i420", *f, frame_id=t) if isinstance(f, tuple) else cpu.encode(f, t)
        bg, bc = og["cells"].reshape(-1, 12), cpu.debug_buffer("blk").reshape(-1, 12)
        bad = np.argwhere((bg != bc).any(axis=1))
        assert len(bad) == 0, f"frame {t}: {len(bad)} cells differ, first {bad[:3].ravel().tolist()} " \
                              f"gpu {bg[bad[0][0]].tolist()} cpu {bc[bad[0][0]].tolist()}"
        for a, b, n in zip(og["rec"], ref_planes(cpu, W, H), "YUV"):
            assert np.array_equal(a, b), f"frame {t}: {n} reconstruction differs at {np.argwhere(a != b)[:3].tolist()}"
        assert og["data"] == bytes(pc[0].data), f"frame {t}: bitstream differs"
        cfl = K.is_cfl(bg)
        if t in want_cfl:
            assert cfl.any(), f"frame {t}: no CfL block"
        assert (bg[:, K.BLK_UV_MODE][(bg[:, K.BLK_FLAGS] & 1) == 1] != K.UV_CFL_PRED).all()
    return gpu.rc_stats(), cpu.rc_stats()


def test_gpu_alpha_picture():
    _check(K.ALPHA_W, K.ALPHA_H, [K.alpha_picture()], qp=ALPHA_QP)


def test_gpu_hue_texture_72():
    """72x72: 8x8 blocks with 4x4 chroma in the last column and row (16 active lanes in the CfL pass)."""
    _check(72, 72, [K.hue_texture(72, 72, 0), K.hue_texture(72, 72, 1)], want_cfl=(0, 1), qp=QP, intra_inter=True)


@pytest.mark.parametrize("W,H,kw", [(200, 120, {}), (512, 320, dict(tile_cols_log2=2, tile_rows_log2=1))])
def test_gpu_tiles(W, H, kw):
    _check(W, H, [K.hue_texture(W, H, 0), K.hue_texture(W, H, 1)], want_cfl=(0, 1), qp=QP, intra_inter=True, **kw)


def test_gpu_inter_frames():
    _check(256, 128, K.window_frames(256, 128), want_cfl=(U.WINDOW_FRAME,), qp=QP, intra_inter=True)


def test_gpu_recode_under_cbr():
    """256x128 CBR over the plain wallpaper: the gated re-code passes redo the CfL decisions; the same
    passes as the CPU encoder's."""
    W, H = 256, 128
    sg, sc = _check(W, H, cbr_frames(W, H), want_cfl=(), intra_inter=True, rate_control="cbr", bitrate_kbps=CBR_KBPS,
                    fps=60.0)
    assert sg == sc and sg["redos"] > 0, (sg, sc)


def test_gpu_with_ltr_slots():
    """256x128, ltr_slots = 2: A -> B -> A with a hue texture in the tile row that reads LAST2."""
    W, H = 256, 128
    _check(W, H, ltr_frames(W, H), want_cfl=(20,), qp=24, stripe_height=STRIPE, use_paint_over=False, ltr_slots=2,
           intra_inter=True)


def test_gpu_with_chroma_palette():
    W, H = 256, 128
    _check(W, H, [K.combined_picture(W, H, 0), K.combined_picture(W, H, 1)], want_cfl=(0, 1), qp=QP, intra_inter=True,
           chroma_palette=True)


def test_gpu_1080p():
    """Frames 1..3 of the hue-texture window sequence at 1080p with intra_inter (frame 0 of the run is
    the key frame): tiles hold more units on an anti-diagonal than the workgroups of the wavefront
    kernels have waves."""
    W, H = 1920, 1080
    _check(W, H, K.window_frames(W, H)[1:4], want_cfl=(1,), qp=QP, intra_inter=True)
