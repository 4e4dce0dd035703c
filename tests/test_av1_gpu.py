"""HIP AV1 back end (kernels/av1_kernels.hip) against the CPU reference encoder
(codec/av1_cpu.cpp): identical temporal units byte for byte (headers, every tile),
identical block decisions, levels and reconstruction; dav1d decodes the GPU stream
to the GPU's own reconstruction."""
import numpy as np
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from selkies_gstreamer_amd.ops.native import Av1Encoder, hip_device_count
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
from tests.extremes_util import _planes

pytestmark = pytest.mark.gpu


def _pair(W, H, **kw):
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    return Av1Encoder(W, H, backend="hip", **kw), Av1Encoder(W, H, backend="cpu", **kw)


def _check(W, H, kind, frames, **kw):
    gpu, cpu = _pair(W, H, **kw)
    src = SyntheticDesktop(W, H, kind=kind)
    dec = dav1d.Decoder() if dav1d.available() else None
    sy = (W + 15) // 16 * 16
    for t in range(frames):
        f = src.frame(t)
        pg = gpu.encode(f, t)
        pc = cpu.encode(f, t)
        bg = gpu.debug_buffer("blk").reshape(-1, 12)
        bc = cpu.debug_buffer("blk").reshape(-1, 12)
        bad = np.argwhere((bg != bc).any(axis=1))
        assert len(bad) == 0, f"frame {t}: {len(bad)} cells differ, first {bad[:3].ravel().tolist()} " \
                              f"gpu {bg[bad[0][0]].tolist()} cpu {bc[bad[0][0]].tolist()}"
        ry_g = gpu.debug_buffer("ref_y").reshape(-1, sy)[:H, :W]
        ry_c = cpu.debug_buffer("ref_y").reshape(-1, sy)[:H, :W]
        assert (ry_g == ry_c).all(), f"frame {t}: reconstruction differs at {np.argwhere(ry_g != ry_c)[:3].tolist()}"
        assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: bitstream differs"
        if dec is not None:
            pic = dec.decode(pg[0].data[10:])
            assert pic is not None, f"frame {t}: dav1d produced no picture"
            for name, a, b in zip("YUV", pic, _planes(gpu, W, H)):
                assert a.shape == b.shape, f"frame {t} plane {name}: decoder {a.shape}, encoder {b.shape}"
                assert np.array_equal(a, b), f"frame {t} plane {name}: first difference at {np.argwhere(a != b)[:3].tolist()}"


@pytest.mark.parametrize("W,H", [(64, 64), (256, 128), (200, 120), (640, 360)])
def test_gpu_matches_cpu(W, H):
    _check(W, H, "motion", 4, qp=25)


def test_gpu_tiles_and_noise():
    _check(512, 320, "motion", 3, qp=30, tile_cols_log2=2, tile_rows_log2=1)
    _check(192, 128, "noise", 2, qp=30)


def test_gpu_1080p():
    _check(1920, 1080, "motion", 3, qp=25)


def test_gpu_4k_tile_layout():
    """3840x2160: the automatic 16 x 4 tile split (av1_core.h auto_tiles), key and inter
    frames, GPU == CPU."""
    _check(3840, 2160, "desktop", 2, qp=30)


def test_gpu_palette_key_frames():
    """Palette blocks (desktop content: text and flat UI on key frames): the GPU's
    decisions (k_av1_intra_rec), colour caches and lane-parallel index-map tokens equal
    the CPU reference's."""
    _check(640, 360, "desktop", 3, qp=22)
    _check(1920, 1080, "desktop", 2, qp=30)
