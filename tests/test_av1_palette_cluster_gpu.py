"""AV1 clustered luma palettes on the HIP back end (the clustering of intra_mode_wave, the luma
recoding of intra_rec_block, the nearest-colour map of k_av1_tokens) against the CPU reference encoder
with the option on: identical cells, luma palette cells, reconstruction and temporal units byte for
byte (so the levels, through the bitstream), and dav1d decodes the GPU stream to the GPU's
reconstruction (all planes)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, hip_device_count
from tests import av1_chroma_palette_util as C
from tests import av1_intra_inter_util as U
from tests import av1_palette_cluster_util as P
from tests.ltr_util import STRIPE, ref_planes
from tests.test_av1_palette_cluster import CBR_KBPS, QP, cbr_frames, ltr_frames

pytestmark = pytest.mark.gpu


def _pair(W, H, **kw):
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    kw = dict(dict(palette_cluster=True), **kw)
    return Av1Encoder(W, H, backend="hip", **kw), Av1Encoder(W, H, backend="cpu", **kw)


def _check(W, H, seq, want=(0,), **kw):
    """HIP == CPU on every frame of seq (BGRx arrays or (Y, U, V) tuples); want: frames that must hold
    clustered blocks. Returns the rate-control statistics of both encoders."""
    gpu, cpu = _pair(W, H, **kw)
    ck = C.Checked(gpu, W, H)      # dav1d on the GPU stream
    for t, f in enumerate(seq):
        og = ck.step(f)
        pc = cpu.encode_yuv("i420", *f, frame_id=t) if isinstance(f, tuple) else cpu.encode(f, t)
        bg, bc = og["cells"].reshape(-1, 12), cpu.debug_buffer("blk").reshape(-1, 12)
        bad = np.argwhere((bg != bc).any(axis=1))
        assert len(bad) == 0, f"frame {t}: {len(bad)} cells differ, first {bad[:3].ravel().tolist()} " \
                              f"gpu {bg[bad[0][0]].tolist()} cpu {bc[bad[0][0]].tolist()}"
        ny = P.pal_n(bg)
        pg, pcu = P.pal_y(gpu, W, H).reshape(-1, 8)[ny > 0], cpu.debug_buffer("pal").reshape(-1, 8)[ny > 0]
        assert np.array_equal(pg, pcu), f"frame {t}: luma palette cells differ at {np.argwhere(pg != pcu)[:3].tolist()}"
        for a, b, n in zip(og["rec"], ref_planes(cpu, W, H), "YUV"):
            assert np.array_equal(a, b), f"frame {t}: {n} reconstruction differs at {np.argwhere(a != b)[:3].tolist()}"
        assert og["data"] == bytes(pc[0].data), f"frame {t}: bitstream differs"
        if t in want:
            assert P.clustered(og["src"][0], og["cells"]).any(), f"frame {t}: no clustered block"
    return gpu.rc_stats(), cpu.rc_stats()


def test_gpu_designed_picture():
    _check(P.DESIGN_W, P.DESIGN_H, [P.designed_picture()], qp=QP)


def test_gpu_aa_field_72():
    """72x72: 8x8 blocks in the last column and row (one histogram of 64 samples per wave)."""
    _check(72, 72, [P.aa_field(72, 72, 0), P.aa_field(72, 72, 3)], want=(0, 1), qp=QP, intra_inter=True)


@pytest.mark.parametrize("W,H,kw", [(200, 120, {}), (512, 320, dict(tile_cols_log2=2, tile_rows_log2=1))])
def test_gpu_tiles(W, H, kw):
    _check(W, H, [P.aa_field(W, H, 0), P.soft_field(W, H, 3)], want=(0, 1), qp=QP, intra_inter=True, **kw)


def test_gpu_inter_frames():
    _check(256, 128, P.window_frames(256, 128), want=(U.WINDOW_FRAME,), qp=QP, intra_inter=True)


def test_gpu_recode_under_cbr():
    """256x128 CBR over the plain wallpaper: the gated re-code passes cluster again at their own
    qindex; the same passes as the CPU encoder's."""
    W, H = 256, 128
    sg, sc = _check(W, H, cbr_frames(W, H), want=(), intra_inter=True, rate_control="cbr", bitrate_kbps=CBR_KBPS,
                    fps=60.0)
    assert sg == sc and sg["redos"] > 0, (sg, sc)


def test_gpu_with_ltr_slots():
    """256x128, ltr_slots = 2: A -> B -> A with an anti-aliased opening in the tile row that reads LAST2."""
    W, H = 256, 128
    _check(W, H, ltr_frames(W, H), want=(20,), qp=QP, stripe_height=STRIPE, use_paint_over=False, ltr_slots=2,
           intra_inter=True)


def test_gpu_with_chroma_tools():
    W, H = 256, 128
    _check(W, H, P.shifted_frames(P.aa_field, W, H), want=(0, 1, 2), qp=QP, intra_inter=True, chroma_palette=True,
           cfl=True)


def test_gpu_1080p():
    """Frames 1..3 of the anti-aliased window sequence at 1080p with intra_inter (frame 0 of the run is
    the key frame): tiles hold more units on an anti-diagonal than the workgroups of the wavefront
    kernels have waves."""
    W, H = 1920, 1080
    _check(W, H, P.window_frames(W, H)[1:4], want=(1,), qp=QP, intra_inter=True)
