"""The zero-level fast paths of k_code_inter (luma levels all zero, chroma levels all zero, cbp 0
after the analysis), its CAVLC tables loaded only by workgroups with a coded macroblock, and the
intra pre-pass in the same launch (P and I waves in one workgroup): bit-exact against the CPU
reference, frame by frame, at the smallest shapes at which they can go wrong.
Every sequence is encoded once on the CPU back end (cached); a test without the gpu mark checks
that it really reaches its case there, the gpu test compares packets, macroblock decisions, the
motion field and the reference pictures, and feeds every stream to the decoder."""
import functools

import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import H264Encoder, MB_INFO_DTYPE, ME_DTYPE, TASK_DTYPE
from tests.h264_util import StripeDecoder, synthetic_frames

ACT_P, ACT_I, ACT_SKIPALL = 1, 2, 3
MB_P_SKIP = 0
GROUP = 4   # macroblocks of a k_code_inter workgroup: idx // 4
MB_FIELDS = ("type", "mvx", "mvy", "mvdx", "mvdy", "ref", "i16_mode", "chroma_mode", "qp", "cbp", "nnz")


def _base(W, H, seed=3):
    return next(iter(synthetic_frames(W, H, 1, seed=seed)))


def _texture(W, H, seed=7, colour=False):
    """Smooth random texture (box-filtered noise), grey or with independent colour planes."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 256, (H + 8, W + 8, 3 if colour else 1)).astype(np.int64)
    s = sum(n[dy:dy + H, dx:dx + W] for dy in range(4) for dx in range(4)) // 16
    f = np.zeros((H, W, 4), np.uint8)
    f[..., :3] = s
    return f


def _rectangle(W, H, n):
    """Static textured picture; a 64 x 48 rectangle of other texture moves 3 px right and 2 px
    down per frame, and a second, flat one jumps by 16 px (its interior matches exactly)."""
    base = _base(W, H)
    patch = _texture(64, 48, seed=11, colour=True)
    out = []
    for t in range(n):
        f = base.copy()
        f[8 + 2 * t:56 + 2 * t, 40 + 3 * t:104 + 3 * t] = patch
        f[72:104, 16 + 16 * t:80 + 16 * t, :3] = (40, 170, 90)
        out.append(f)
    return out


def _colour_scroll(W, H, n):
    """Saturated colour texture shifted vertically by 3 px per frame."""
    tex = _texture(W, H + 3 * n, seed=5, colour=True)
    tex[..., 0] = tex[..., 0] // 4
    tex[..., 1] = 255 - tex[..., 1] // 4
    return [tex[3 * t:3 * t + H].copy() for t in range(n)]


def _grey_under_colour_change(W, H, n):
    """Grey texture moving by whole pixels; the right half gets a flat tint that changes from frame
    to frame: the luma moves everywhere, the chroma planes stay as they were in the left half
    (nothing to code) and flat inside a macroblock in the right half (DC only)."""
    tex = _texture(W + 2 * n, H, seed=9)
    out = []
    for t in range(n):
        f = tex[:, 2 * t:2 * t + W].astype(np.int64) // 2 + 40
        f[:, W // 2:, 2] += 9 * t
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def _dithered_shift(W, H, n):
    """A picture shifted by whole pixels with +-1 dither on a few pixels of every frame."""
    tex = _texture(W + 4 * n, H, seed=13, colour=True)
    rng = np.random.default_rng(2)
    out = []
    for t in range(n):
        f = tex[:, 4 * t:4 * t + W].astype(np.int64)
        ys, xs = rng.integers(0, H, 120), rng.integers(0, W, 120)
        f[ys, xs, :3] += rng.choice([-1, 1], 120)[:, None]
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return out


def _toggle(W, H, n):
    """A caret blinks and a button toggles: frame t equals frame t - 2 (tests/test_h264_cpu.py)."""
    base = next(synthetic_frames(W, H, 1, seed=4))
    on = base.copy()
    on[20:36, 40:42, :3] = 10
    on[60:76, 90:130, :3] = (230, 160, 40)
    return [base if t % 2 == 0 else on for t in range(n)]


def _half_pel_gradient(W, H, n):
    """A smooth gradient moved by half a pixel per frame: rendered at 2x, shifted by one fine
    pixel, down-sampled by averaging 2 x 2."""
    yy, xx = np.mgrid[0:2 * H, 0:2 * W + 2 * n].astype(np.float64)
    fine = 128 + 60 * np.sin(xx / 23.0) + 50 * np.cos(yy / 31.0 + xx / 57.0)
    out = []
    for t in range(n):
        g = fine[:, t:t + 2 * W].reshape(H, 2, W, 2).mean(axis=(1, 3))
        f = np.zeros((H, W, 4), np.uint8)
        f[..., :3] = np.clip(np.rint(g), 0, 255).astype(np.uint8)[..., None]
        out.append(f)
    return out


def _stripe_cut(W, H, n, at, stripe):
    """A moving rectangle; from frame `at` on every second stripe shows an unrelated picture."""
    frames = _rectangle(W, H, n)
    other = np.random.default_rng(5).integers(0, 256, (H, W, 4), dtype=np.uint8)
    for t in range(at, n):
        for y in range(stripe, H - stripe, 2 * stripe):   # the last stripe stays as it was
            frames[t][y:y + stripe] = np.roll(other[y:y + stripe], 2 * (t - at), axis=1)
    return frames


def _hard_cut(W, H, n, at):
    """tests/test_h264_chain_fused.py: a moving desktop, then another, noise-textured image."""
    other = np.random.default_rng(5).integers(0, 256, (H, W, 4), dtype=np.uint8)
    a = list(synthetic_frames(W, H, n, seed=4))
    return [a[t] if t < at else np.roll(other, 2 * (t - at), axis=1) for t in range(n)]


# name -> (width, height, frames, encoder options). 208 wide: 13 MBs per row, so the
# workgroups of 4 straddle row and slice boundaries. An unchanged slice is ACT_NONE in stripe
# mode and SKIPALL only in a full frame, so the P / I / SKIPALL frame also runs as "_ff".
CASES = {
    "all_zero_skip_and_coded": (208, 112, lambda: _rectangle(208, 112, 5), dict(stripe_height=32)),
    "luma_zero_chroma_coded": (208, 112, lambda: _colour_scroll(208, 112, 5), dict(stripe_height=32, qp=10)),
    "chroma_zero_luma_coded": (208, 112, lambda: _grey_under_colour_change(208, 112, 5), dict(stripe_height=32, qp=10)),
    "decimated_to_zero": (208, 112, lambda: _dithered_shift(208, 112, 5), dict(stripe_height=32)),
    "qp_0": (208, 112, lambda: _rectangle(208, 112, 5), dict(stripe_height=32, qp=0)),
    "qp_51": (208, 112, lambda: _rectangle(208, 112, 5), dict(stripe_height=32, qp=51)),
    "aq_start_qp": (208, 112, lambda: _rectangle(208, 112, 5), dict(stripe_height=32, aq_strength=1.0)),
    "second_reference": (208, 112, lambda: _toggle(208, 112, 6), dict(stripe_height=32, qp=24, use_paint_over=False, num_refs=2)),
    "fractional_vector": (208, 112, lambda: _half_pel_gradient(208, 112, 5), dict(stripe_height=32)),
    "p_and_i_in_one_workgroup": (208, 128, lambda: _stripe_cut(208, 128, 6, 3, 16), dict(stripe_height=16)),
    "p_and_i_in_one_workgroup_i4": (208, 128, lambda: _stripe_cut(208, 128, 6, 3, 16), dict(stripe_height=16, intra4x4=True)),
    "p_and_i_in_one_workgroup_ff": (208, 128, lambda: _stripe_cut(208, 128, 6, 3, 16), dict(stripe_height=16, fullframe=True)),
    "cbr_gated_second_pass": (192, 128, lambda: _hard_cut(192, 128, 6, 3),
                              dict(stripe_height=32, rate_control="cbr", bitrate_kbps=200, fps=60.0)),
    "fullframe": (208, 112, lambda: _rectangle(208, 112, 5), dict(stripe_height=32, fullframe=True)),
}


def _encoder(W, H, backend, kw):
    return H264Encoder(W, H, backend=backend, **dict(dict(qp=26), **kw))


def _snapshot(enc, packets):
    s = dict(packets=[p.data for p in packets], tasks=enc.debug_buffer("tasks", TASK_DTYPE).copy(),
             mbs=enc.debug_buffer("mbs", MB_INFO_DTYPE).copy(), me=enc.debug_buffer("me", ME_DTYPE).copy())
    for n in ("src_y", "ref_y", "ref_u", "ref_v"):
        s[n] = enc.debug_buffer(n).copy()
    return s


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(frames, per-frame snapshots of the CPU back end, its rate control's counters), once per case."""
    W, H, frames, kw = CASES[name]
    frames = frames()
    cpu = _encoder(W, H, "cpu", kw)
    snaps = [_snapshot(cpu, cpu.encode(f, t)) for t, f in enumerate(frames)]
    return frames, snaps, cpu.rc_stats()


def _rows(task, mb_w):
    return slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)


def _residual_nonzero(snap, prev, task, idx, mb_w):
    """Luma source of MB idx differs from its motion-compensated prediction (whole-pixel vector
    into the previous picture, prediction block inside the slice's picture rows)."""
    mb = snap["mbs"][idx]
    if mb["ref"] != 0 or (mb["mvx"] | mb["mvy"]) & 3:
        return False
    stride = snap["src_y"].size // (len(snap["mbs"]) // mb_w * 16)
    src, ref = snap["src_y"].reshape(-1, stride), prev["ref_y"].reshape(-1, stride)
    x, y = idx % mb_w * 16, idx // mb_w * 16
    px, py = x + mb["mvx"] // 4, y + mb["mvy"] // 4
    if px < 0 or px + 16 > mb_w * 16 or py < task["pic_row0"] * 16 or py + 16 > (task["pic_row0"] + task["pic_rows"]) * 16:
        return False
    return bool((src[y:y + 16, x:x + 16] != ref[py:py + 16, px:px + 16]).any())


def _facts(name):
    """What the CPU reference did, per frame: counts over the macroblocks of its final P slices."""
    W, H, _, _ = CASES[name]
    mb_w = (W + 15) // 16
    _, snaps, _ = _reference(name)
    out = []
    for t, snap in enumerate(snaps):
        mbs, tasks = snap["mbs"], snap["tasks"]
        f = dict(p=0, skip=0, zero_not_skip=0, coded=0, luma_zero_chroma_coded=0, chroma_zero_luma_coded=0,
                 zero_with_residual=0, fast_other_qp=0, zero_ref1=0, zero_ref1_skip=0, zero_fractional=0,
                 groups=set(), pi_in_group=0, skipall_next_to_coded=0,
                 actions=[int(a) for a in tasks["final_action"]])
        is_p = np.zeros(len(mbs), bool)
        for task in tasks:
            if task["final_action"] != ACT_P:
                continue
            sl = _rows(task, mb_w)
            is_p[sl] = True
            m = mbs[sl]
            zero = m["cbp"] == 0
            f["p"] += len(m)
            f["skip"] += int((zero & (m["type"] == MB_P_SKIP)).sum())
            f["zero_not_skip"] += int((zero & (m["type"] != MB_P_SKIP)).sum())
            f["coded"] += int((~zero).sum())
            f["luma_zero_chroma_coded"] += int((((m["cbp"] & 15) == 0) & ((m["cbp"] >> 4) != 0)).sum())
            f["chroma_zero_luma_coded"] += int((((m["cbp"] & 15) != 0) & ((m["cbp"] >> 4) == 0)).sum())
            f["fast_other_qp"] += int((zero & (m["qp"] != task["qp"])).sum())
            f["zero_ref1"] += int((zero & (m["ref"] == 1)).sum())
            f["zero_ref1_skip"] += int((zero & (m["ref"] == 1) & (m["type"] == MB_P_SKIP)).sum())
            f["zero_fractional"] += int((zero & (((m["mvx"] | m["mvy"]) & 3) != 0)).sum())
            if t > 0:
                f["zero_with_residual"] += sum(_residual_nonzero(snap, snaps[t - 1], task, i, mb_w)
                                               for i in range(sl.start, sl.stop) if mbs["cbp"][i] == 0)
        is_i = np.zeros(len(mbs), bool)
        for task in tasks:
            if task["final_action"] == ACT_I:
                is_i[_rows(task, mb_w)] = True
        for g in range(0, len(mbs), GROUP):
            sl = slice(g, min(g + GROUP, len(mbs)))
            if is_p[sl].all():
                z = mbs["cbp"][sl] == 0
                f["groups"].add("all fast" if z.all() else ("none fast" if not z.any() else "mixed"))
            f["pi_in_group"] += int(is_p[sl].any() and is_i[sl].any())
        acts = f["actions"]
        f["skipall_next_to_coded"] = sum(1 for a, b in zip(acts, acts[1:])
                                         if ACT_SKIPALL in (a, b) and (a in (ACT_P, ACT_I) or b in (ACT_P, ACT_I)))
        out.append(f)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_sequence_reaches_its_case_on_cpu(name):
    facts = _facts(name)
    any_frame = lambda key: any(f[key] > 0 for f in facts)
    assert any_frame("p"), facts
    if name in ("all_zero_skip_and_coded", "fullframe", "aq_start_qp"):
        assert any(f["skip"] and f["zero_not_skip"] and f["coded"] and
                   f["groups"] >= {"all fast", "mixed", "none fast"} for f in facts), facts
    if name == "luma_zero_chroma_coded":
        assert any_frame("luma_zero_chroma_coded"), facts
    if name == "chroma_zero_luma_coded":
        assert any_frame("chroma_zero_luma_coded"), facts
    if name == "decimated_to_zero":
        assert any_frame("zero_with_residual"), facts
    if name == "qp_0":
        assert any_frame("skip") and any_frame("coded"), facts
    if name == "qp_51":
        assert any(f["skip"] + f["zero_not_skip"] > 3 * f["coded"] for f in facts if f["p"]), facts
    if name == "aq_start_qp":
        assert any_frame("fast_other_qp"), facts
    if name == "second_reference":
        assert any_frame("zero_ref1") and not any_frame("zero_ref1_skip"), facts
    if name == "fractional_vector":
        assert any_frame("zero_fractional"), facts
    if name.startswith("p_and_i_in_one_workgroup"):
        f = facts[3]   # the frame of the cut
        assert ACT_P in f["actions"] and ACT_I in f["actions"] and f["pi_in_group"] > 0, facts
        if name.endswith("_ff"):   # stripes code an unchanged slice as ACT_NONE; only a full frame has SKIPALL
            assert f["skipall_next_to_coded"] > 0, facts
    if name == "cbr_gated_second_pass":
        assert _reference(name)[2]["redos"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_matches_cpu(name):
    W, H, _, kw = CASES[name]
    mb_w = (W + 15) // 16
    frames, snaps, rc = _reference(name)
    gpu = _encoder(W, H, "hip", kw)
    sd = StripeDecoder(W, H)
    for t, (f, ref) in enumerate(zip(frames, snaps)):
        got = _snapshot(gpu, gpu.encode(f, t))
        assert got["packets"] == ref["packets"], f"frame {t}: bitstreams differ"
        assert np.array_equal(got["tasks"]["final_action"], ref["tasks"]["final_action"]), f"frame {t}: slice decisions differ"
        for task in ref["tasks"]:
            if task["final_action"] not in (ACT_P, ACT_I):
                continue
            sl = _rows(task, mb_w)
            for n in MB_FIELDS:
                assert np.array_equal(got["mbs"][n][sl], ref["mbs"][n][sl]), f"frame {t}: MB {n} differs from row {task['first_row']}"
            if task["final_action"] == ACT_P:
                for n in ("mvx", "mvy", "ref"):
                    assert np.array_equal(got["me"][n][sl], ref["me"][n][sl]), f"frame {t}: ME {n} differs"
        for n in ("ref_y", "ref_u", "ref_v"):
            assert np.array_equal(got[n], ref[n]), f"frame {t}: {n} differs"
        for p in got["packets"]:
            sd.feed(p)
    assert gpu.rc_stats() == rc
