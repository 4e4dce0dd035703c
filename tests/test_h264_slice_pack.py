"""k_slice_pack (one workgroup per slice: header, scan of the MB bit counts, MB words shifted
into an LDS chunk, emulation prevention, 16-byte stores to the host slot), the rate
accounting moved to k_commit, the CBR guard's size-only pass, and the launches that are
left out of a frame's graphs (the intra kernel that cannot have work, the deblocking
kernels of a frame in which no slice can be filtered): the HIP back end against the CPU
reference, frame by frame - packet bytes, packet heads and the rate controller's state.

Noise never produces an emulation-prevention byte, so most tests here use "sparse" frames:
every pixel 128, 2 % of the pixels (drawn fresh per frame) 0 or 255 in all four channels,
coded at QP 0. Every test asserts the property it relies on from the CPU's packets;
insertions are counted as 00 00 03 inside the slice NALs."""
import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import H264Encoder, MB_INFO_DTYPE, TASK_DTYPE
from tests.h264_util import synthetic_frames

pytestmark = pytest.mark.gpu

ACT_NONE, ACT_P, ACT_I = 0, 1, 2
MB_P_SKIP = 0
GPU = "hip"            # the back end under test
CHUNK = 8192           # k_slice_pack's kPackChunk: RBSP bytes per pass
AUTO_DEBLOCK_QP = 34   # kAutoDeblockQp


def sparse_frames(W, H, n, dense_from=None):
    """dense_from: from that frame on 15 % of the pixels instead of 2 %."""
    rng = np.random.default_rng(1)
    out = []
    for t in range(n):
        f = np.full((H, W, 4), 128, np.uint8)
        hit = rng.random((H, W)) < (0.02 if dense_from is None or t < dense_from else 0.15)
        val = (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8)
        f[hit] = val[hit][:, None]
        out.append(f)
    return out


def slice_nals(packet, striped=True):
    """The slice NALs (types 1 and 5) of a packet, without their start codes. Inside a NAL no
    00 00 00 / 00 00 01 survives emulation prevention, so the start codes split exactly."""
    data = bytes(packet.data)[10 if striped else 0:]
    return [n for n in data.split(b"\x00\x00\x00\x01") if n and (n[0] & 0x1F) in (1, 5)]


def insertions(nal):
    return nal.count(b"\x00\x00\x03")


def _same(t, cpu, gpu, pc, pg, rc=True):
    assert [p.data for p in pg] == [p.data for p in pc], f"frame {t}: packet bytes differ"
    assert [(p.y, p.key) for p in pg] == [(p.y, p.key) for p in pc], f"frame {t}: packet heads differ"
    if rc:
        assert gpu.rc_stats() == cpu.rc_stats(), f"frame {t}: rate controller state differs"


def _run(W, H, frames, before=None, **kw):
    """Both back ends serially; before(t, enc) runs on each ahead of frame t. Returns the CPU's
    packets and slice tasks per frame, and both encoders."""
    cpu, gpu = H264Encoder(W, H, backend="cpu", **kw), H264Encoder(W, H, backend=GPU, **kw)
    packets, tasks = [], []
    for t, f in enumerate(frames):
        if before:
            before(t, cpu)
            before(t, gpu)
        pc, pg = cpu.encode(f, t), gpu.encode(f, t)
        _same(t, cpu, gpu, pc, pg)
        packets.append(pc)
        tasks.append(cpu.debug_buffer("tasks", TASK_DTYPE).copy())
    return packets, tasks, cpu, gpu


def _coded_qps(ta):
    return ta["qp"][(ta["final_action"] == ACT_P) | (ta["final_action"] == ACT_I)]


def test_one_chunk_nals_straddled_slices():
    """130x70, stripes of 48: slices of 27 macroblocks, straddled by the four-MB workgroups of
    the kernels before the packing, a partial last slice; every NAL fits one chunk and every
    P NAL holds insertions."""
    W, H = 130, 70
    packets, tasks, _, _ = _run(W, H, sparse_frames(W, H, 4), stripe_height=48, qp=0, paint_qp=0)
    for t in range(1, 4):
        assert (tasks[t]["final_action"] == ACT_P).all()
        for p in packets[t]:
            (nal,) = slice_nals(p)
            assert len(nal) < CHUNK and insertions(nal) > 0


@pytest.fixture(scope="module")
def wide():
    W, H = 672, 128
    return W, H, sparse_frames(W, H, 3)


def _check_wide(packets, striped):
    """672 wide (mb_w 42): the first frame's I slices are sub-sliced, several NALs chained in
    one slot; the P NALs after it are longer than two chunks (stripes of 128) or than one
    (stripes of 64), all with insertions."""
    first = [n for p in packets[0] for n in slice_nals(p, striped)]
    assert len(first) > len(packets[0]) and sum(insertions(n) for n in first) > 0
    return [[n for p in packets[t] for n in slice_nals(p, striped)] for t in (1, 2)]


def test_sub_nals_and_a_nal_of_several_chunks(wide):
    W, H, frames = wide
    packets, _, _, _ = _run(W, H, frames, stripe_height=128, qp=0, paint_qp=0)
    for nals in _check_wide(packets, True):
        (nal,) = nals
        assert len(nal) > 2 * CHUNK and insertions(nal) > 0


def test_two_slices_in_one_picture(wide):
    W, H, frames = wide
    packets, _, _, _ = _run(W, H, frames, stripe_height=64, fullframe=True, qp=0, paint_qp=0)
    for nals in _check_wide(packets, False):
        assert len(nals) == 2
        for nal in nals:
            assert len(nal) > CHUNK and insertions(nal) > 0


def test_two_frames_in_flight(wide):
    """upload / launch of frame n + 1 before finish of frame n: the host slots of both parities."""
    W, H, frames = wide
    kw = dict(stripe_height=128, qp=0, paint_qp=0)
    cpu, gpu = H264Encoder(W, H, backend="cpu", **kw), H264Encoder(W, H, backend=GPU, **kw)
    want = [cpu.encode(f, t) for t, f in enumerate(frames)]
    assert all(insertions(n) > 0 for t in (1, 2) for p in want[t] for n in slice_nals(p))
    got = []
    for t, f in enumerate(frames):
        gpu.upload(f, t)
        gpu.launch()
        if t > 0:
            got.append(gpu.finish())
    got.append(gpu.finish())
    assert len(got) == len(want)
    for t, (pc, pg) in enumerate(zip(want, got)):
        _same(t, cpu, gpu, pc, pg, rc=False)
    assert gpu.rc_stats() == cpu.rc_stats()


def test_cbr_second_pass_with_insertions():
    """CBR at 9 Mbit/s, which the sparse frames fit at QP 10-12 (with insertions) until frame
    3 is seven times as dense and overflows the buffer: the size-only pass ahead of the guard,
    the gated second coding pass, one full packing behind it, the accounting in k_commit.
    (The re-coded frame itself runs at QP 23, where these frames hold no insertion; the frames
    before it and frame 5 behind it do.)"""
    W, H = 672, 64
    packets, _, cpu, _ = _run(W, H, sparse_frames(W, H, 7, dense_from=3), stripe_height=64, rate_control="cbr",
                              bitrate_kbps=9000, fps=60.0)
    assert cpu.rc_stats()["redos"] > 0
    count = [sum(insertions(n) for p in pk for n in slice_nals(p)) for pk in packets]
    assert sum(count[:3]) > 0 and sum(count[4:]) > 0


def test_identical_frames_code_nothing():
    W, H = 130, 70
    f = sparse_frames(W, H, 1)[0]
    packets, tasks, _, _ = _run(W, H, [f] * 4, stripe_height=48, qp=0, paint_qp=0, use_paint_over=False)
    for t in range(1, 4):
        assert (tasks[t]["final_action"] == ACT_NONE).all() and packets[t] == []


def test_skip_runs_at_the_end_of_a_slice():
    """The right half static: P slices whose last macroblocks are skipped (the trailing
    mb_skip_run behind the last coded macroblock)."""
    W, H = 192, 64
    frames = sparse_frames(W, H, 4)
    for f in frames[1:]:
        f[:, W // 2:] = frames[0][:, W // 2:]
    _, tasks, cpu, _ = _run(W, H, frames, stripe_height=32, qp=0, paint_qp=0)
    for t in range(1, 4):
        assert (tasks[t]["final_action"] == ACT_P).all()
    mbs, mb_w = cpu.debug_buffer("mbs", MB_INFO_DTYPE), W // 16
    for ta in tasks[3]:   # the last macroblock of every slice of the last frame is skipped
        assert mbs["type"][(ta["first_row"] + ta["num_rows"]) * mb_w - 1] == MB_P_SKIP


BATCH = 512   # k_slice_pack's kPackThreads: macroblocks per batch of its scan


@pytest.mark.parametrize("static", ["none", "right", "bottom"])
def test_slice_of_several_batches(static):
    """1920x128, one stripe of 128: a slice of 960 macroblocks, two batches of the kernel's scan,
    a P NAL of a dozen chunks. Only batch 0 keeps its offsets in registers: batch 1 is loaded
    and scanned again for every chunk, and the RBSP word at the batch boundary has bits of both.
    "right": the right half static, so the last coded macroblock and the trailing skip run
    lie in batch 1. "bottom": the lower four MB rows static, so batch 1 is runs of macroblocks
    without a bit between a few coded ones (QP 0 is not lossless: some static MBs still code)."""
    W, H, mb_w = 1920, 128, 120
    frames = sparse_frames(W, H, 3)
    for f in frames[1:]:
        if static == "right":
            f[:, W // 2:] = frames[0][:, W // 2:]
        if static == "bottom":
            f[H // 2:] = frames[0][H // 2:]
    packets, tasks, cpu, _ = _run(W, H, frames, stripe_height=128, qp=0, paint_qp=0)
    assert len(tasks[2]) == 1 and tasks[2]["num_rows"][0] * mb_w > BATCH
    for t in (1, 2):
        assert (tasks[t]["final_action"] == ACT_P).all()
        (nal,) = [n for p in packets[t] for n in slice_nals(p)]
        assert len(nal) > 2 * CHUNK and insertions(nal) > 0
    coded = np.flatnonzero(cpu.debug_buffer("mbs", MB_INFO_DTYPE)["type"][:8 * mb_w] != MB_P_SKIP)
    if static == "none":
        assert coded[-1] == 8 * mb_w - 1
    if static == "right":   # rows end in skipped macroblocks; the last coded one is in batch 1
        assert BATCH < coded[-1] < 8 * mb_w - mb_w // 4
    if static == "bottom":
        assert 0 < (coded >= BATCH).sum() < (8 * mb_w - BATCH) // 4


def test_p_and_i_slices_side_by_side():
    """130x70, stripes of 48: from frame 2 on the top stripe shows another image (its planned
    P slice is re-coded as I) while the bottom keeps moving: I and P slices of one frame go
    through one launch of the packing kernel (and workgroups of four macroblocks of the coding
    kernels hold waves of both)."""
    W, H = 130, 70
    frames = list(synthetic_frames(W, H, 5, seed=9))
    other = np.random.default_rng(5).integers(0, 256, (H, W, 4), dtype=np.uint8)
    for t in range(2, 5):
        frames[t][:48] = np.roll(other[:48], 2 * (t - 2), axis=1)
    _, tasks, _, _ = _run(W, H, frames, stripe_height=48, qp=26)
    assert any((ta["final_action"] == ACT_I).any() and (ta["final_action"] == ACT_P).any() for ta in tasks)


@pytest.mark.parametrize("W,H", [(192, 128), (672, 64)], ids=["wavefront", "sub-sliced"])
def test_first_frame_and_hard_cut(W, H):
    """The one intra kernel a geometry launches: the wavefront kernel (192 wide) or the
    sub-slice kernel (672 wide: mb_w 42)."""
    other = np.random.default_rng(5).integers(0, 256, (H, W, 4), dtype=np.uint8)
    a = list(synthetic_frames(W, H, 4, seed=4))
    frames = [a[t] if t < 2 else np.roll(other, 2 * (t - 2), axis=1) for t in range(4)]
    _, tasks, _, _ = _run(W, H, frames, stripe_height=32, qp=26)
    assert (tasks[0]["final_action"] == ACT_I).all()
    assert any(((ta["action"] == ACT_P) & (ta["final_action"] == ACT_I)).any() for ta in tasks)


# Which commit graph a frame took cannot be seen from outside: the output is the same by
# design. What these cases can show is a graph taken wrongly: the short graph for a frame with
# a filtered slice leaves its reference unfiltered and the following frames differ from the CPU's.


def test_auto_deblock_crf_stays_unfiltered():
    """CRF 25: no slice reaches QP 34, the commit graph without the deblocking kernels."""
    W, H = 192, 128
    _, tasks, _, _ = _run(W, H, list(synthetic_frames(W, H, 6, seed=4)), stripe_height=32, qp=25,
                          rate_control="crf", deblock="auto")
    assert all((_coded_qps(ta) < AUTO_DEBLOCK_QP).all() for ta in tasks)
    assert any(len(_coded_qps(ta)) for ta in tasks[1:])


def test_auto_deblock_follows_set_qp():
    """set_qp(36) before frame 3, set_qp(26) before frame 5: frames 3 and 4 are filtered, the
    others are not; equal packets afterwards show that the references stayed in step."""
    W, H = 192, 128

    def before(t, e):
        if t == 3:
            e.set_qp(36, 20)
        if t == 5:
            e.set_qp(26, 20)

    _, tasks, _, _ = _run(W, H, list(synthetic_frames(W, H, 8, seed=4)), before, stripe_height=32, qp=26,
                          deblock="auto")
    for t, ta in enumerate(tasks):
        q = _coded_qps(ta)
        assert len(q) > 0
        assert (q >= AUTO_DEBLOCK_QP).all() if t in (3, 4) else (q < AUTO_DEBLOCK_QP).all()


def test_auto_deblock_cbr_reaches_filtered_qps():
    W, H = 192, 128
    _, tasks, _, _ = _run(W, H, list(synthetic_frames(W, H, 8, seed=4)), stripe_height=32, rate_control="cbr",
                          bitrate_kbps=200, fps=60.0, deblock="auto")
    assert any((_coded_qps(ta) >= AUTO_DEBLOCK_QP).any() for ta in tasks[:-1])


def test_deblock_on_at_qp_26():
    W, H = 192, 128
    _, tasks, _, _ = _run(W, H, list(synthetic_frames(W, H, 5, seed=4)), stripe_height=32, qp=26, deblock=True)
    assert all((_coded_qps(ta) == 26).all() for ta in tasks)
