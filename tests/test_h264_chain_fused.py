"""The bookkeeping of a frame's dispatch chain (stripe controller, scene-cut decisions, frame
QP, intra launches, slice scan, the CBR guard's gated second pass) and the overlay placement,
which is copied ahead of the graph only when it changed: bit-exact against the CPU reference,
frame by frame (packets, slice tasks, the search's sad / intra_est), at the smallest shapes
at which each of them can go wrong (slices straddled by workgroups, slices that are not
coded, scene cuts, host requests between frames, sub-sliced I slices, two frames in flight)."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import (Av1Encoder, H264Encoder, HevcEncoder, MB_INFO_DTYPE, ME_DTYPE,
                                              TASK_DTYPE, convert_bgrx)
from tests.h264_util import synthetic_frames

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_P, ACT_I = 0, 1, 2
MB_P_SKIP = 0
GPU = "hip"   # the back end under test
CBR_KBPS = 200   # 192x128 at 60 fps: the CPU reference re-codes a frame after the hard cut


def _compare(cpu, gpu, t, pc, pg, mb_w):
    """Packets, final tasks and the search's sums of frame t; returns the CPU's (tasks, mbs)."""
    assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: bitstreams differ"
    assert [(p.y, p.key) for p in pg] == [(p.y, p.key) for p in pc], f"frame {t}: packet heads differ"
    ta, tb = cpu.debug_buffer("tasks", TASK_DTYPE), gpu.debug_buffer("tasks", TASK_DTYPE)
    assert np.array_equal(ta, tb), f"frame {t}: slice tasks differ"
    ma, mg = cpu.debug_buffer("me", ME_DTYPE), gpu.debug_buffer("me", ME_DTYPE)
    for task in ta:
        if task["action"] not in (ACT_P, ACT_I):
            continue   # the search leaves these slices' results alone
        sl = slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)
        for name in ("sad", "intra_est"):
            assert np.array_equal(ma[name][sl], mg[name][sl]), f"frame {t}: ME {name} differs"
    return ta.copy(), cpu.debug_buffer("mbs", MB_INFO_DTYPE).copy()


def _run(W, H, frames, before=None, cls=H264Encoder, **kw):
    """Encodes `frames` serially on both back ends; before(t, enc) runs on each ahead of
    frame t. Returns the CPU reference's per-frame (tasks, mbs) and both encoders."""
    cpu, gpu = cls(W, H, backend="cpu", **kw), cls(W, H, backend=GPU, **kw)
    seen = []
    for t, f in enumerate(frames):
        if before:
            before(t, cpu)
            before(t, gpu)
        seen.append(_compare(cpu, gpu, t, cpu.encode(f, t), gpu.encode(f, t), (W + 15) // 16))
    return seen, cpu, gpu


def _run_two_in_flight(W, H, frames, before=None, **kw):
    """The GPU encoder with upload / launch of frame n + 1 before finish of frame n against
    the CPU encoder run serially (packets only: the debug buffers follow the last launch)."""
    cpu, gpu = H264Encoder(W, H, backend="cpu", **kw), H264Encoder(W, H, backend=GPU, **kw)
    want = []
    for t, f in enumerate(frames):
        if before:
            before(t, cpu)
        want.append([p.data for p in cpu.encode(f, t)])
    if GPU == "cpu":
        return
    got = []
    for t, f in enumerate(frames):
        if before:
            before(t, gpu)
        gpu.upload(f, t)
        gpu.launch()
        if t > 0:
            got.append([p.data for p in gpu.finish()])
    got.append([p.data for p in gpu.finish()])
    for t, (a, b) in enumerate(zip(want, got)):
        assert a == b, f"frame {t}: bitstreams differ with two frames in flight"
    assert len(got) == len(want)


def _base(W, H, seed=3):
    return next(iter(synthetic_frames(W, H, 1, seed=seed)))


def _half_moving(W, H, n):
    base = _base(W, H)
    out = []
    for t in range(n):
        f = base.copy()
        f[:, W // 2:] = np.roll(base[:, W // 2:], (3 * t, 5 * t), axis=(0, 1))
        out.append(f)
    return out


def _hard_cut(W, H, n, at):
    """A moving desktop, then from frame `at` a different image (noise-textured) that moves on."""
    rng = np.random.default_rng(5)
    other = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    a = list(synthetic_frames(W, H, n, seed=4))
    return [a[t] if t < at else np.roll(other, 2 * (t - at), axis=1) for t in range(n)]


def _cut_happened(seen):
    return any(((ta["action"] == ACT_P) & (ta["final_action"] == ACT_I)).any() for ta, _ in seen)


def test_slices_straddled_by_workgroups():
    """130x70, stripes of 48: mb_w 9, slices of 27 macroblocks, so k_me's workgroups (four
    macroblocks) straddle two slices and the last one is partial."""
    W, H = 130, 70
    seen, _, _ = _run(W, H, list(synthetic_frames(W, H, 5, seed=9)), stripe_height=48, qp=26)
    assert any((ta["final_action"] == ACT_P).any() for ta, _ in seen)


def test_skipped_untouched_and_paint_over_slices():
    """Upper two stripes: right half moving, left half static (P slices with skipped
    macroblocks). Lower two stripes: still, nearly flat blocks, so they are not coded until
    the paint-over, whose P slices at the paint QP find the coarse reference worse than intra
    and are re-coded as I by the scene-cut decision."""
    W, H, mb_w, paint_qp = 192, 128, 12, 18
    lv = np.random.default_rng(1).integers(60, 65, (H // 16, W // 8))
    flat = np.kron(lv, np.ones((8, 8), int)).astype(np.uint8)
    frames = _half_moving(W, H, 7)
    for f in frames:
        f[H // 2:] = flat[..., None]
    seen, _, _ = _run(W, H, frames, stripe_height=32, qp=34, paint_qp=paint_qp, paint_over_trigger=2,
                      paint_over_burst=2)
    skipped = untouched = paint_i = False
    for ta, mbs in seen:
        for task in ta:
            sl = slice(task["first_row"] * mb_w, (task["first_row"] + task["num_rows"]) * mb_w)
            if task["final_action"] == ACT_P and (mbs["type"][sl] == MB_P_SKIP).any():
                skipped = True
            if task["action"] == ACT_NONE:
                untouched = True
            if task["action"] == ACT_P and task["qp"] == paint_qp and task["final_action"] == ACT_I:
                paint_i = True
    assert skipped and untouched and paint_i


def test_hard_cut_turns_p_slices_into_i():
    """A hard cut in mid-sequence: planned P slices are re-coded as I."""
    W, H = 192, 128
    seen, _, _ = _run(W, H, _hard_cut(W, H, 6, 3), stripe_height=32, qp=26)
    assert _cut_happened(seen)


def test_keyframe_and_qp_requests_between_frames():
    """request_keyframe() and set_qp() between frames: the controller's host snapshot."""
    W, H = 192, 128

    def before(t, e):
        if t == 2:
            e.request_keyframe()
        if t == 4:
            e.set_qp(33, 20)

    seen, _, _ = _run(W, H, _half_moving(W, H, 6), before, stripe_height=32, qp=26)
    assert (seen[2][0]["action"] == ACT_I).all()
    assert (seen[4][0]["qp"][seen[4][0]["final_action"] == ACT_P] == 33).all()


@pytest.mark.parametrize("W,H", [(672, 64), (192, 128)], ids=["sub-sliced", "wavefront"])
def test_intra_slices_first_frame_and_cut(W, H):
    """First frame plus a hard cut. 672x64: mb_w 42, I slices are sub-sliced (3 NALs per
    slice); 192x128: the wavefront intra kernel."""
    seen, _, _ = _run(W, H, _hard_cut(W, H, 4, 2), stripe_height=32, qp=26)
    assert (seen[0][0]["final_action"] == ACT_I).all()
    assert _cut_happened(seen)


def test_cbr_gated_second_pass():
    """CBR at a rate the content overflows: the guard's gated second coding pass, and before it
    the frames of the hard cut, which overflow at the top QP, where the guard has no coarser
    step to apply and must leave the first pass's slices as they are."""
    W, H = 192, 128
    frames = _hard_cut(W, H, 12, 3)
    seen, cpu, gpu = _run(W, H, frames, stripe_height=32, rate_control="cbr", bitrate_kbps=CBR_KBPS, fps=60.0)
    assert cpu.rc_stats()["redos"] > 0
    assert cpu.rc_stats() == gpu.rc_stats()


@pytest.mark.parametrize("kw", [dict(me_full=False), dict(fullframe=True), dict(num_refs=2), dict(intra4x4=True),
                                dict(aq_strength=1.0)],
                         ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_option_variants(kw):
    W, H = 192, 128
    _run(W, H, _hard_cut(W, H, 5, 3), stripe_height=32, qp=26, **kw)


def test_two_frames_in_flight():
    W, H = 192, 128
    _run_two_in_flight(W, H, _hard_cut(W, H, 6, 3), stripe_height=32, qp=26)


def _overlay_script(rng):
    img = rng.integers(0, 256, (24, 40, 4), dtype=np.uint8)
    img[..., :3] = (img[..., :3].astype(np.int32) * img[..., 3:] // 255).astype(np.uint8)   # premultiplied

    def before(t, e):
        if t == 0:
            e.set_overlay(0, img)
            e.set_overlay_pos(0, 20, 10)
        if t == 2:
            e.set_overlay_pos(0, 90, 60)
        if t == 4:
            e.set_overlay_pos(0, 90, 60, enabled=False)

    return before


@pytest.mark.parametrize("inflight", [1, 2])
def test_overlay_set_moved_disabled(inflight):
    """Overlay set at frame 0, moved at frame 2, disabled at frame 4, unchanged in between:
    the placement copy ahead of the graph, sent only on a change, serially and with two
    frames in flight (the copy is ordered behind the previous frame's graph)."""
    W, H = 192, 128
    frames = _half_moving(W, H, 6)
    before = _overlay_script(np.random.default_rng(2))
    if inflight == 1:
        _run(W, H, frames, before, stripe_height=32, qp=26)
    else:
        _run_two_in_flight(W, H, frames, before, stripe_height=32, qp=26)


def test_planar_input():
    """encode_yuv: the stripe flags come from k_yuv_damage."""
    W, H = 192, 128
    cpu, gpu = (H264Encoder(W, H, backend=b, stripe_height=32, qp=26) for b in ("cpu", GPU))
    for t, f in enumerate(_half_moving(W, H, 3)):
        planes = convert_bgrx(f, "i420")
        pc, pg = cpu.encode_yuv("i420", *planes, frame_id=t), gpu.encode_yuv("i420", *planes, frame_id=t)
        _compare(cpu, gpu, t, pc, pg, (W + 15) // 16)


@pytest.mark.parametrize("cls,W,H", [(HevcEncoder, 64, 64), (Av1Encoder, 64, 64)], ids=["hevc", "av1"])
def test_other_codecs_share_the_front_end(cls, W, H):
    """HEVC and AV1 run launch_convert_damage and launch_frontend too (their own suites are
    the real check)."""
    cpu, gpu = cls(W, H, backend="cpu"), cls(W, H, backend=GPU)
    for t, f in enumerate(synthetic_frames(W, H, 3, seed=6)):
        pc, pg = cpu.encode(f, t), gpu.encode(f, t)
        assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: packets differ"
        assert np.array_equal(cpu.debug_buffer("tasks", TASK_DTYPE), gpu.debug_buffer("tasks", TASK_DTYPE))
