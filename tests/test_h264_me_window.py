"""k_me with one reference window and one |r|^2 table per workgroup (four neighbouring
macroblocks of one MB row): bit-exact against the CPU reference, frame by frame, at the
smallest shapes at which sharing can go wrong. Every sequence is encoded once on the CPU
back end (cached); a test without the gpu mark checks that it really reaches its case there,
the gpu test compares packets, the exhaustive-search winners and the motion results."""
import functools

import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import H264Encoder, HevcEncoder, ME_DTYPE, TASK_DTYPE
from tests.h264_util import synthetic_frames
from tests.ltr_util import sequence

ACT_P = 1
GROUP = 4   # macroblocks of a k_me workgroup


def _base(W, H, seed=3):
    return next(iter(synthetic_frames(W, H, 1, seed=seed)))


def _shifted(W, H, n, dx, dy, seed=3):
    base = _base(W, H, seed)
    return [np.roll(base, (dy * t, dx * t), axis=(0, 1)) for t in range(n)]


def _rectangle(W, H, n):
    """Static picture; only the rectangle x 72..135, y 24..87 moves (3 px right, 2 px down per frame)."""
    base = _base(W, H)
    out = []
    for t in range(n):
        f = base.copy()
        f[24:88, 72:136] = np.roll(base[24:88, 72:136], (2 * t, 3 * t), axis=(0, 1))
        out.append(f)
    return out


def _flat_blocks(W, H, n, step=16):
    """Flat 32 x 32 colour tiles moving `step` pixels to the right per frame over a textured lower
    half that moves with them: tile interiors match exactly at their previous vector, the texture
    and the tile edges do not."""
    rng = np.random.default_rng(5)
    tiles = rng.integers(0, 4, (H // 32, W // 32 + 1)) * 60 + 20
    pic = np.kron(tiles, np.ones((32, 32), np.int64))[:H, :W]
    base = np.zeros((H, W, 4), np.uint8)
    base[..., :3] = pic[..., None]
    tex = _base(W, H)
    base[H // 2:] = tex[H // 2:]
    return [np.roll(base, step * t, axis=1) for t in range(n)]


# name -> (codec, width, height, frames, encoder options)
CASES = {
    "last_group_of_one": ("h264", 208, 128, lambda: _shifted(208, 128, 4, 5, 3), dict(stripe_height=32)),
    "row_shorter_than_a_group": ("h264", 48, 64, lambda: _shifted(48, 64, 4, 3, 2), dict(stripe_height=32)),
    "window_leaves_the_picture": ("h264", 64, 64, lambda: _shifted(64, 64, 4, 7, 5), dict(stripe_height=64)),
    "slice_row_clamps": ("h264", 256, 128, lambda: _shifted(256, 128, 4, 5, 9), dict(stripe_height=64)),
    "picture_row_clamps": ("h264", 256, 128, lambda: _shifted(256, 128, 4, 5, 9), dict(stripe_height=64, fullframe=True)),
    "clean_and_dirty_in_a_group": ("h264", 208, 128, lambda: _rectangle(208, 128, 4), dict(stripe_height=32)),
    "exact_match_shortcut": ("h264", 256, 128, lambda: _flat_blocks(256, 128, 5), dict(stripe_height=64, qp=10)),
    "jump_beyond_the_window": ("h264", 208, 128, lambda: _shifted(208, 128, 4, 24, 0), dict(stripe_height=32)),
    "two_references": ("h264", 208, 128, lambda: _shifted(208, 128, 4, 5, 3), dict(stripe_height=32, num_refs=2)),
    "ltr_cache_hit": ("h264", 208, 112, lambda: [f for _, _, f in sequence("A10 B10 A2")],
                      dict(stripe_height=32, qp=24, use_paint_over=False, ltr_slots=2)),
    "hevc": ("hevc", 128, 128, lambda: _shifted(128, 128, 4, 5, 3), dict(qp=26, use_paint_over=False)),
}


def _encoder(codec, W, H, backend, kw):
    kw = dict(dict(qp=26), **kw)
    return (HevcEncoder if codec == "hevc" else H264Encoder)(W, H, backend=backend, **kw)


def _snapshot(enc, packets, codec):
    """The HEVC CPU back end keeps no damage map or fs_mv of its own to read back: there the packets,
    the tasks and the motion results are compared, and every macroblock counts as dirty."""
    me = enc.debug_buffer("me", ME_DTYPE).copy()
    if codec == "hevc":
        dirty, fs = np.ones(len(me), np.uint8), np.stack([me["mvx"], me["mvy"]], axis=1)
    else:
        dirty, fs = enc.debug_buffer("mb_dirty").copy(), enc.debug_buffer("fs_mv", np.int16).reshape(-1, 2).copy()
    return dict(packets=[p.data for p in packets], tasks=enc.debug_buffer("tasks", TASK_DTYPE).copy(), me=me,
                dirty=dirty, fs=fs)


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(frames, per-frame snapshots of the CPU back end), computed once per case."""
    codec, W, H, frames, kw = CASES[name]
    frames = frames()
    cpu = _encoder(codec, W, H, "cpu", kw)
    return frames, [_snapshot(cpu, cpu.encode(f, t), codec) for t, f in enumerate(frames)]


def _p_slices(snap, mb_w):
    for task in snap["tasks"]:
        if task["action"] == ACT_P:
            yield task, slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)


def _facts(name):
    """What the CPU reference did over the sequence, per dirty macroblock of a planned P slice:
    searched (no exact match at the previous vector: its final SAD is not 0), shortcut (final
    vector = previous vector = fs_mv with SAD 0), and the groups (MB row, mbx / 4) they lie in."""
    _, W, H, _, _ = CASES[name]
    mb_w = (W + 15) // 16
    frames, snaps = _reference(name)
    nmb = len(snaps[0]["me"])
    prev = np.zeros((nmb, 2), np.int64)   # the CPU model's mvfield: vectors of the last coded picture
    out = dict(searched=0, shortcut=0, nonzero_fs=0, far=0, clean=0, ref1=0, groups=[], last_col=0)
    for snap in snaps:
        me = snap["me"]
        mv = np.stack([me["mvx"], me["mvy"]], axis=1).astype(np.int64)
        for task, sl in _p_slices(snap, mb_w):
            idx = np.arange(sl.start, sl.stop)
            dirty = snap["dirty"][sl] != 0
            searched = dirty & (me["sad"][sl] != 0)
            shortcut = dirty & (me["sad"][sl] == 0) & (mv[sl] == prev[sl]).all(1) & (snap["fs"][sl] == prev[sl]).all(1)
            out["searched"] += int(searched.sum())
            out["shortcut"] += int(shortcut.sum())
            out["clean"] += int((~dirty).sum())
            out["nonzero_fs"] += int((searched & (snap["fs"][sl] != 0).any(1)).sum())
            out["far"] += int((searched & (np.abs(mv[sl]).max(1) > 16)).sum())
            out["ref1"] += int((me["ref"][sl] == 1).sum())
            out["last_col"] += int((searched & (idx % mb_w == mb_w - 1)).sum())
            grp = (idx // mb_w) * 64 + (idx % mb_w) // GROUP
            for g in np.unique(grp):
                m = grp == g
                out["groups"].append((bool(searched[m].any()), bool(shortcut[m].any()), bool((~dirty[m]).any())))
        for task in snap["tasks"]:
            sl = slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)
            if task["final_action"] in (ACT_P, 2):   # coded (2 = I): the vectors of the search
                prev[sl] = mv[sl]
            elif task["final_action"] == 3:          # skip-all picture: zero vectors
                prev[sl] = 0
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_sequence_reaches_its_case_on_cpu(name):
    f = _facts(name)
    assert f["searched"] > 0 and f["nonzero_fs"] > 0, f
    if name == "last_group_of_one":
        assert f["last_col"] > 0, f
    if name == "clean_and_dirty_in_a_group":
        assert any(s and c for s, _, c in f["groups"]), f
    if name == "exact_match_shortcut":
        assert any(s and k for s, k, _ in f["groups"]), f
    if name == "jump_beyond_the_window":
        assert f["far"] > 0, f
    if name == "ltr_cache_hit":
        assert f["ref1"] > 0, f


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_matches_cpu(name):
    codec, W, H, _, kw = CASES[name]
    mb_w = (W + 15) // 16
    frames, snaps = _reference(name)
    gpu = _encoder(codec, W, H, "hip", kw)
    for t, (f, ref) in enumerate(zip(frames, snaps)):
        got = _snapshot(gpu, gpu.encode(f, t), codec)
        assert got["packets"] == ref["packets"], f"frame {t}: bitstreams differ"
        assert np.array_equal(got["tasks"], ref["tasks"]), f"frame {t}: slice tasks differ"
        for task, sl in _p_slices(ref, mb_w):
            assert np.array_equal(got["dirty"][sl], ref["dirty"][sl]), f"frame {t}: damage differs"
            dirty = ref["dirty"][sl] != 0
            assert np.array_equal(got["fs"][sl][dirty], ref["fs"][sl][dirty]), f"frame {t}: fs_mv differs"
            names = ("sad", "intra_est") + (("mvx", "mvy", "ref") if task["final_action"] == ACT_P else ())
            for n in names:   # a scene cut re-codes the slice as I and drops the vectors
                assert np.array_equal(got["me"][n][sl], ref["me"][n][sl]), f"frame {t}: ME {n} differs"
