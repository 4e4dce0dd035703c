"""Fused motion estimation (k_me: exhaustive search and candidate / diamond search in one
dispatch, SADs read from the exhaustive search's LDS window) and the two-dispatch
emulation prevention with the rate accounting inside it: bit-exact against the CPU
reference, frame by frame, at the smallest shapes that reach every path of the search."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import H264Encoder, ME_DTYPE, TASK_DTYPE
from tests.h264_util import synthetic_frames

pytestmark = pytest.mark.gpu

ACT_P = 1


def _run(W, H, frames, **kw):
    """Encodes `frames` on both back ends and compares packets, the search results of every
    P-planned slice and the exhaustive-search winners of its dirty macroblocks. Returns
    per-frame (tasks, me, mb_dirty) of the CPU reference for the callers' own conditions."""
    cpu, gpu = H264Encoder(W, H, backend="cpu", **kw), H264Encoder(W, H, backend="hip", **kw)
    mb_w = (W + 15) // 16
    seen = []
    for t, f in enumerate(frames):
        pc, pg = cpu.encode(f, t), gpu.encode(f, t)
        assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: bitstreams differ"
        ta, tb = cpu.debug_buffer("tasks", TASK_DTYPE), gpu.debug_buffer("tasks", TASK_DTYPE)
        assert np.array_equal(ta, tb), f"frame {t}: slice tasks differ"
        ma, mg = cpu.debug_buffer("me", ME_DTYPE), gpu.debug_buffer("me", ME_DTYPE)
        da, dg = cpu.debug_buffer("mb_dirty"), gpu.debug_buffer("mb_dirty")
        fa, fg = (e.debug_buffer("fs_mv", np.int16).reshape(-1, 2) for e in (cpu, gpu))
        for task in ta:
            if task["action"] != ACT_P:
                continue
            sl = slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)
            assert np.array_equal(da[sl], dg[sl]), f"frame {t}: damage differs"
            if task["final_action"] == ACT_P:   # a scene cut re-codes the slice as I and drops the vectors
                for name in ("mvx", "mvy", "ref"):
                    assert np.array_equal(ma[name][sl], mg[name][sl]), f"frame {t}: ME {name} differs"
            for name in ("sad", "intra_est"):
                assert np.array_equal(ma[name][sl], mg[name][sl]), f"frame {t}: ME {name} differs"
            if kw.get("me_full", True):
                dirty = da[sl] != 0
                assert np.array_equal(fa[sl][dirty], fg[sl][dirty]), f"frame {t}: fs_mv differs"
        seen.append((ta.copy(), ma.copy(), da.copy()))
    return seen


def _coded_p(seen, mb_w):
    """(me, dirty) rows of every macroblock of a coded P slice, all frames together."""
    me, dirty = [], []
    for ta, ma, da in seen:
        for task in ta:
            if task["action"] == ACT_P and task["final_action"] == ACT_P:
                sl = slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)
                me.append(ma[sl])
                dirty.append(da[sl])
    assert me, "no coded P slice"
    return np.concatenate(me), np.concatenate(dirty)


def _base(W, H):
    return next(iter(synthetic_frames(W, H, 1, seed=3)))


def _shifted(W, H, n, dx=40, dy=20):
    base = _base(W, H)
    return [np.roll(base, (dy * t, dx * t), axis=(0, 1)) for t in range(n)]


def _half_moving(W, H, n):
    base = _base(W, H)
    out = []
    for t in range(n):
        f = base.copy()
        f[:, W // 2:] = np.roll(base[:, W // 2:], (3 * t, 5 * t), axis=(0, 1))
        out.append(f)
    return out


def test_odd_geometry_partial_workgroup():
    """130x70: mb_w 9, 45 macroblocks (the last workgroup has one wave of work), right and
    bottom edges clamped inside the exhaustive search's window."""
    W, H = 130, 70
    seen = _run(W, H, list(synthetic_frames(W, H, 5, seed=9)), stripe_height=48, qp=26)
    _coded_p(seen, 9)


def test_vectors_beyond_the_window_and_stripe_clamps():
    """40 px / 20 px per frame: predictors leave the +-16 window (global-memory SADs) and the
    vertical motion runs into the stripes' row clamps."""
    W, H = 192, 128
    seen = _run(W, H, _shifted(W, H, 6), stripe_height=32, qp=26)
    me, _ = _coded_p(seen, 12)
    reach = np.maximum(np.abs(me["mvx"].astype(int)), np.abs(me["mvy"].astype(int)))
    assert (reach > 16).any() and (reach <= 16).any()


def test_clean_macroblocks_of_p_slices():
    """Static left half, moving right half: P slices with dirty macroblocks (exhaustive search,
    big window) and clean ones (no phase 1, small window)."""
    W, H = 192, 128
    seen = _run(W, H, _half_moving(W, H, 5), stripe_height=32, qp=26)
    _, dirty = _coded_p(seen, 12)
    assert (dirty != 0).any() and (dirty == 0).any()


@pytest.mark.parametrize("kw", [dict(me_range=8), dict(num_refs=2), dict(fullframe=True), dict(me_full=False)],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_search_options(kw):
    """me_range 8 clips inside the window; two references; one picture of slices (vertical
    clamps at the picture, not the stripe); me_full off runs the kept k_motion_search."""
    W, H = 192, 128
    frames = _shifted(W, H, 3, dx=6, dy=3) + _half_moving(W, H, 4)[1:]
    seen = _run(W, H, frames, stripe_height=32, qp=26, **kw)
    _coded_p(seen, 12)


def test_emulation_prevention_carries_across_tiles():
    """One 320x64 stripe of noise at QP 4: the slice's RBSP spans more than two 4 KiB
    emulation-prevention tiles, so tiles 1 and 2 take their carry by looking backwards."""
    W, H = 320, 64
    kw = dict(stripe_height=64, qp=4, paint_qp=4)
    cpu, gpu = H264Encoder(W, H, backend="cpu", **kw), H264Encoder(W, H, backend="hip", **kw)
    rng = np.random.default_rng(1)
    for t in range(2):
        f = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        pc, pg = cpu.encode(f, t), gpu.encode(f, t)
        assert len(pc) == 1 and len(pc[0].data) > 2 * 4096
        assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: bitstreams differ"
