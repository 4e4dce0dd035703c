"""The AV1 encoder's tools in all 16 combinations on the HIP back end against the CPU reference
encoder: identical cells, palette cells (luma and chroma, where their counts are nonzero),
reconstruction (all planes) and temporal units byte for byte on the sequence of av1_tools_util.py,
whose CPU streams test_av1_tools.py pins to recorded digests; dav1d decodes the GPU stream to the
GPU's reconstruction. Masks 5 (chroma palette + cluster) and 6 (CfL + cluster) run nowhere else."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, hip_device_count
from tests import av1_chroma_palette_util as C
from tests import av1_palette_cluster_util as P
from tests import av1_tools_util as T
from tests.ltr_util import ref_planes

pytestmark = pytest.mark.gpu


def _check(w, h, seq, mask, ii, **kw):
    """HIP == CPU on every frame of seq; returns what the GPU frames' blocks took (av1_tools_util.took)."""
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    kw = dict(T.case_kwargs(mask, ii), qp=T.QP, **kw)
    gpu, cpu = Av1Encoder(w, h, backend="hip", **kw), Av1Encoder(w, h, backend="cpu", **kw)
    ck = C.Checked(gpu, w, h)      # dav1d on the GPU stream
    took = []
    for t, f in enumerate(seq):
        og = ck.step(f)
        pc = cpu.encode(f, t)
        bg, bc = og["cells"].reshape(-1, 12), cpu.debug_buffer("blk").reshape(-1, 12)
        bad = np.argwhere((bg != bc).any(axis=1))
        assert len(bad) == 0, f"frame {t}: {len(bad)} cells differ, first {bad[:3].ravel().tolist()} " \
                              f"gpu {bg[bad[0][0]].tolist()} cpu {bc[bad[0][0]].tolist()}"
        ny, nuv = P.pal_n(bg), bg[:, C.BLK_PAL_N] >> 4
        pg, pcu = P.pal_y(gpu, w, h).reshape(-1, 8)[ny > 0], cpu.debug_buffer("pal").reshape(-1, 8)[ny > 0]
        assert np.array_equal(pg, pcu), f"frame {t}: luma palette cells differ at {np.argwhere(pg != pcu)[:3].tolist()}"
        ug, ucu = og["pal_uv"].reshape(-1, 16)[nuv > 0], cpu.debug_buffer("pal_uv").reshape(-1, 16)[nuv > 0]
        assert np.array_equal(ug, ucu), f"frame {t}: chroma palette cells differ at {np.argwhere(ug != ucu)[:3].tolist()}"
        for a, b, n in zip(og["rec"], ref_planes(cpu, w, h), "YUV"):
            assert np.array_equal(a, b), f"frame {t}: {n} reconstruction differs at {np.argwhere(a != b)[:3].tolist()}"
        assert og["data"] == bytes(pc[0].data), f"frame {t}: bitstream differs"
        took.append(T.took(og["src"][0], og["cells"], og["key"]))
    gpu.close()
    cpu.close()
    return took


@pytest.mark.parametrize("mask,ii", T.CASES, ids=[T.case_id(m, ii) for m, ii in T.CASES])
def test_gpu_equals_cpu(mask, ii):
    took = _check(T.W, T.H, T.frames(), mask, ii)
    for name, on in T.case_kwargs(mask, ii).items():
        assert any(f[name] for f in took) == on, f"{name}: enabled {on}, taken {[f[name] for f in took]}"


def test_gpu_two_tile_columns():
    """200x120 in two tile columns, every tool on: the wavefront of the intra kernels ends at a tile
    edge inside the picture, in key and inter frames."""
    w, h = 200, 120
    took = _check(w, h, T.frames(w, h, cuts=(96, 144)), 7, True, tile_cols_log2=1)
    assert all(any(f[name] for f in took) for name in took[0]), took
