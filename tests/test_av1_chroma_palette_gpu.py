"""AV1 chroma palettes on the HIP back end (the chroma candidate of intra_mode_wave, the decision of
intra_rec_block, the chroma map of k_av1_tokens) against the CPU reference encoder with the option
on: identical cells, chroma palette cells, reconstruction and temporal units byte for byte, and
dav1d decodes the GPU stream to the GPU's reconstruction (all planes)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import Av1Encoder, hip_device_count
from tests import av1_chroma_palette_util as C
from tests import av1_intra_inter_util as U
from tests.av1_ltr_util import contents, sequence
from tests.ltr_util import STRIPE, ref_planes
from tests.test_av1_chroma_palette import cbr_frames

pytestmark = pytest.mark.gpu


def _pair(W, H, **kw):
    if hip_device_count() < 1:
        pytest.skip("no HIP device")
    kw = dict(dict(chroma_palette=True), **kw)
    return Av1Encoder(W, H, backend="hip", **kw), Av1Encoder(W, H, backend="cpu", **kw)


def _check(W, H, seq, want_uv=(0,), **kw):
    """HIP == CPU on every frame of seq (BGRx arrays or (Y, U, V) tuples); want_uv: frames that must
    hold chroma palettes. Returns the rate-control statistics of both encoders."""
    gpu, cpu = _pair(W, H, **kw)
    ck = C.Checked(gpu, W, H)      # dav1d on the GPU stream
    for t, f in enumerate(seq):
        og = ck.step(f)
        pc = cpu.encode_yuv("i420", *f, frame_id=t) if isinstance(f, tuple) else cpu.encode(f, t)
        bg, bc = og["cells"].reshape(-1, 12), cpu.debug_buffer("blk").reshape(-1, 12)
        bad = np.argwhere((bg != bc).any(axis=1))
        assert len(bad) == 0, f"frame {t}: {len(bad)} cells differ, first {bad[:3].ravel().tolist()} " \
                              f"gpu {bg[bad[0][0]].tolist()} cpu {bc[bad[0][0]].tolist()}"
        uv = bg[:, C.BLK_PAL_N] >> 4
        pg, pcu = og["pal_uv"].reshape(-1, 16)[uv > 0], cpu.debug_buffer("pal_uv").reshape(-1, 16)[uv > 0]
        assert np.array_equal(pg, pcu), f"frame {t}: chroma palette cells differ"
        for a, b, n in zip(og["rec"], ref_planes(cpu, W, H), "YUV"):
            assert np.array_equal(a, b), f"frame {t}: {n} reconstruction differs at {np.argwhere(a != b)[:3].tolist()}"
        assert og["data"] == bytes(pc[0].data), f"frame {t}: bitstream differs"
        if t in want_uv:
            assert (uv >= 2).any(), f"frame {t}: no chroma palette"
        if not og["key"]:
            assert (uv[(bg[:, C.BLK_FLAGS] & 1) == 1] == 0).all()
    return gpu.rc_stats(), cpu.rc_stats()


def test_gpu_pairs_picture():
    _check(C.PAIRS_W, C.PAIRS_H, [C.pairs_picture()], qp=25)


def test_gpu_glyph_field():
    """72x72: 8x8 blocks with 4x4 chroma maps in the last column and row (16 lanes of the wave)."""
    _check(72, 72, [C.glyph_field(72, 72), C.glyph_field(72, 72, 2)], want_uv=(0, 1), qp=25, intra_inter=True)


@pytest.mark.parametrize("W,H,kw", [(200, 120, {}), (512, 320, dict(tile_cols_log2=2, tile_rows_log2=1))])
def test_gpu_tiles(W, H, kw):
    _check(W, H, [C.glyph_field(W, H), C.glyph_field(W, H, 2)], want_uv=(0, 1), qp=25, intra_inter=True, **kw)


def test_gpu_inter_frames():
    _check(256, 128, U.frames(256, 128), want_uv=(0, U.WINDOW_FRAME), qp=25, intra_inter=True)


@pytest.mark.parametrize("content", ["window", "glyphs"])
def test_gpu_recode_under_cbr(content):
    """256x128 CBR over the plain wallpaper: the gated re-code passes redo the candidates and the
    decisions; the same passes as the CPU encoder's."""
    W, H = 256, 128
    seq, kbps = cbr_frames(W, H, content)
    sg, sc = _check(W, H, seq, want_uv=(U.WINDOW_FRAME,) if content == "glyphs" else (), intra_inter=True,
                    rate_control="cbr", bitrate_kbps=kbps, fps=60.0)
    assert sg == sc and sg["redos"] > 0, (sg, sc)


def test_gpu_with_ltr_slots():
    """256x128, ltr_slots = 2: A -> B -> A with a glyph field in the tile row that reads LAST2."""
    W, H = 256, 128
    seq = [f for _, _, f in sequence("A10 B10", W, H)]
    back = contents(W, H)["A"].copy()
    back[8:48, 48:144] = C.glyph_field(96, 40)
    seq += [back, back]
    _check(W, H, seq, want_uv=(0, 20), qp=24, stripe_height=STRIPE, use_paint_over=False, ltr_slots=2, intra_inter=True)


def test_gpu_1080p():
    """Frames 1..3 of the window sequence at 1080p (frame 0 of the run is the key frame): tiles hold
    more units on an anti-diagonal than the workgroups of the wavefront kernels have waves."""
    W, H = 1920, 1080
    _check(W, H, U.frames(W, H)[1:4], want_uv=(0, 1), qp=25, intra_inter=True)
