"""The four switches of the HIP back end that change which code runs: SK_HEVC_PC_SEG, SK_HEVC_REG_STEPS,
SK_NO_GRAPHS and SK_UPLOAD_MODE. Each is read when an encoder is made (member initialisers of
hip_session.h, HevcTail::alloc), so the tests set it in their own process before they make one.
Every case expects exactly the CPU reference, which does not know the switches.

SK_HEVC_PC_SEG (k_pc_model, hevc_kernels.hip): a chain is the context-coded bins of one context in
one CTB row (in a split key-frame row: in one row segment), `tot` of them. It is modelled in up to
64 speculative segments of `seglen = tot > 64 * pc_seg ? ceil(tot / 64) : pc_seg` bins; a segment
whose guessed start state was wrong is run again. At the default 32 the first branch needs 2048
bins of one context in a row and the re-run loop next to never iterates. The reach test shows on the
CPU reference, per content, for pc_seg 1, 2 and 7 a chain in either branch and a guessed start that
is wrong (the loop iterates), and for 4096 that every chain is in the second branch.
  How a chain's length is known: `bin_n` counts a unit's entries, and an entry is a context bin, a
  bypass run of up to 8 bins or a terminating bin, so it bounds the context bins from above only, and
  the share of the largest of 142 contexts only by pigeonhole (a row of noise: some 20 bins). So the
  CPU back end answers the debug name `bins`, the binariser's entries with their context indices
  (hevc_core.h BinBuf), and the test counts exactly: tot(row, segment, context) = the entries of that
  context in the units of the row's segment, in coding order (CTBs left to right, units in z order;
  SliceMap::seg for the segment of a CTB).
  How a wrong guess is known: for the first row of a key frame the chain starts from the context's
  initial state (9.3.2.2, the tables parsed from hevc_core.h); the test runs the kernel's first pass
  on it (every segment from the initial state) and compares each segment's end with the true state
  there.

SK_HEVC_REG_STEPS=0: the 4x4 TUs of intra units in LDS batches (tu_batch / merge_ts) instead of
registers (intra4x4_step / intra_c4_pair). `reg_steps` reaches intra_cu through intra_unit alone, which
three kernels call: k_hevc_intra<4> (stripes of up to four CTB rows), k_hevc_intra<15> (taller stripes)
and k_hevc_intra_seg (split rows, SK_HEVC_SEG_CTBS); one case each, all frames key frames. No other
test codes stripes of more than four CTB rows, so k_hevc_intra<15> runs here with the switch unset
as well (test_tall_stripes).

SK_NO_GRAPHS=1: direct launches through enqueue(part). SK_UPLOAD_MODE 0 / 1: the upload of a frame
that meets one in flight runs on the session stream / the session's own upload stream instead of
the device's shared copy stream. Both run cases of tests/test_session_dynamics.py."""
import functools
import re

import numpy as np
import pytest

from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
from tests import dynamics_util as du
from tests import extremes_util as xu
from tests.matrix_util import hevc_slice_nals
from tests.test_session_dynamics import CASES

W, H, QP = 208, 112, 22
PC_SEGS = (1, 2, 7, 4096)
CTX_COUNT = 142   # hevc_core.h (an enumerator; _tables checks it)
CONTENTS = {"noise": ("noise", None), "desktop": ("desktop", None), "noise-seg3": ("noise", "3")}
DYN_A = [n for n in CASES if n.startswith("a-")]
DYN_D = [n for n in CASES if n.startswith("d-")]


def _hevc_run(content, w=W, h=H, frames=4, **kw):
    return xu.run("hevc", w, h, content, frames=frames, **dict(dict(qp=QP, use_paint_over=False), **kw))


def _frames(r):
    _, w, h, content, n, _ = r
    if content == "noise":
        return xu.noise(w, h, n)
    src = SyntheticDesktop(w, h, kind=content)
    return [src.frame(t) for t in range(n)]


def _env(monkeypatch, **env):
    for n in ("SK_HEVC_SEG_CTBS", "SK_HEVC_PC_SEG", "SK_HEVC_REG_STEPS", "SK_NO_GRAPHS", "SK_UPLOAD_MODE"):
        monkeypatch.delenv(n, raising=False)
    for n, v in env.items():
        if v is not None:
            monkeypatch.setenv(n, str(v))


_CPU = {}


def _cpu(monkeypatch, r, seg, all_key=False):
    """Per-frame snapshots of the CPU back end under SK_HEVC_SEG_CTBS=seg (with the binariser's
    entries), once per (run, seg)."""
    _env(monkeypatch, SK_HEVC_SEG_CTBS=seg)
    key = (r, seg, all_key)
    if key not in _CPU:
        cpu = xu.encoder(r, "cpu")
        snaps = []
        for t, f in enumerate(_frames(r)):
            if all_key:
                cpu.request_keyframe()
            s = xu.snapshot(cpu, r, cpu.encode(f, t))
            s["bins"] = cpu.debug_buffer("bins", np.uint16).copy()
            snaps.append(s)
        cpu.close()
        du._freeze(snaps)
        _CPU[key] = snaps
    return _CPU[key]


def _hip_equals(monkeypatch, r, seg, all_key=False, **switch):
    ref = _cpu(monkeypatch, r, seg, all_key)
    _env(monkeypatch, SK_HEVC_SEG_CTBS=seg, **switch)
    gpu = xu.encoder(r, "hip")
    for t, f in enumerate(_frames(r)):
        if all_key:
            gpu.request_keyframe()
        xu.assert_same(r, t, xu.snapshot(gpu, r, gpu.encode(f, t)), ref[t])
    gpu.close()


# ---- SK_HEVC_PC_SEG ------------------------------------------------------------------------------
def _units_in_coding_order(w, h, cy):
    """Unit indices of CTB row cy with their CTB column: CTBs left to right, units in z order."""
    w16, h16 = (w + 15) // 16, (h + 15) // 16
    for c in range((w16 + 1) // 2):
        for z in range(4):
            ux, uy = 2 * c + (z & 1), 2 * cy + (z >> 1)
            if ux < w16 and uy < h16:
                yield uy * w16 + ux, c


def chains(snap, w, h, seg):
    """{(CTB row, segment, context): [bin, ...]}: the context bins of a coded frame in coding order."""
    cap = xu.K_CU_BIN_CAP
    ctb_w, ctb_h = (w + 31) // 32, (h + 31) // 32
    K = -(-ctb_w // int(seg)) if seg and ctb_w > int(seg) else 1
    bins, out = snap["bins"].reshape(-1, cap), {}
    for cy in range(ctb_h):
        task = next(t for t in snap["tasks"] if t["first_row"] <= 2 * cy < t["first_row"] + t["num_rows"])
        if task["final_action"] == 0:
            continue
        split = K > 1 and task["final_action"] == 2   # SliceMap::split
        for idx, c in _units_in_coding_order(w, h, cy):
            k = ((c + 1) * K - 1) // ctb_w if split else 0   # SliceMap::seg
            for e in bins[idx, :snap["bin_n"][idx]].tolist():
                if not e & 0x8000 and (e & 0xff) < CTX_COUNT:
                    out.setdefault((cy, k, e & 0xff), []).append((e >> 8) & 1)
    return out


@functools.lru_cache(maxsize=None)
def _tables():
    """(HEVC_CTX_INIT of I slices, CABAC_NEXT_LPS) from csrc/codec/hevc_core.h."""
    text = re.sub(r"//[^\n]*", "", (xu.CSRC / "codec/hevc_core.h").read_text())
    assert int(re.search(r"CTX_COUNT = (\d+)", text).group(1)) == CTX_COUNT
    init = [int(v) for v in re.findall(r"\d+", re.search(r"HEVC_CTX_INIT\[2\]\[CTX_COUNT\] = \{(.*?)\};", text, re.S).group(1))]
    nxt = [int(v) for v in re.findall(r"\d+", re.search(r"CABAC_NEXT_LPS\[64\] = \{(.*?)\};", text, re.S).group(1))]
    assert len(init) == 2 * CTX_COUNT and len(nxt) == 64
    return init[:CTX_COUNT], nxt


def _init_state(init_value, qp):
    """9.3.2.2: (pStateIdx << 1) | valMps."""
    m, n = (init_value >> 4) * 5 - 45, ((init_value & 15) << 3) - 16
    pre = min(max(((m * min(max(qp, 0), 51)) >> 4) + n, 1), 126)
    return ((pre - 64) << 1) | 1 if pre > 63 else (63 - pre) << 1


def _step(s, b, nxt):
    st, mps = s >> 1, s & 1
    if b == mps:
        return (min(st + 1, 62) << 1) | mps
    return (nxt[st] << 1) | (mps ^ (st == 0))


def wrong_guesses(chain, s0, pc_seg, nxt):
    """k_pc_model's first pass on one chain: the number of segments whose guessed start state (the end
    of the segment before it, run from s0) is not the true state there."""
    tot = len(chain)
    seglen = -(-tot // 64) if tot > 64 * pc_seg else pc_seg
    true, s = [], s0
    for b in chain:
        true.append(s)
        s = _step(s, b, nxt)
    bad = 0
    for j in range(2, -(-tot // seglen)):   # segment 1's guess is segment 0's end from s0: the truth
        g = s0
        for b in chain[(j - 1) * seglen:j * seglen]:
            g = _step(g, b, nxt)
        bad += g != true[j * seglen]
    return bad


@pytest.mark.parametrize("content", list(CONTENTS))
def test_pc_seg_reach(content, monkeypatch):
    kind, seg = CONTENTS[content]
    r = _hevc_run(kind)
    snaps = _cpu(monkeypatch, r, seg)
    assert [bool(s["packets"][0][2]) for s in snaps] == [True, False, False, False]
    per_frame = [chains(s, W, H, seg) for s in snaps]
    lengths = np.array([len(c) for f in per_frame for c in f.values()])
    print(f"\n{content}: {len(lengths)} chains, longest {lengths.max()}, over 64: {(lengths > 64).sum()}, "
          f"over 128: {(lengths > 128).sum()}, over 448: {(lengths > 448).sum()}")
    if seg:
        assert any(k > 0 for (_, k, _) in per_frame[0]), "no split row in the key frame"
    # pc_seg 7 (448 bins) may have chains of either branch or of the second alone
    assert (lengths > 128).any(), "pc_seg 1 and 2: no chain of the first branch (more than 64 * pc_seg bins)"
    assert (lengths <= 64).any(), "pc_seg 1 and 2: no chain of the second branch"
    assert lengths.max() <= 64 * 4096, "pc_seg 4096: a chain of the first branch"
    # the re-run loop: the chains of the key frame's first row (and first segment) start from the initial states
    init, nxt = _tables()
    first = {c: ch for (cy, k, c), ch in per_frame[0].items() if cy == 0 and k == 0}
    for pc_seg in PC_SEGS[:3]:
        bad = sum(wrong_guesses(ch, _init_state(init[c], QP), pc_seg, nxt) for c, ch in first.items())
        print(f"{content}: pc_seg {pc_seg}: {bad} wrong guesses in the {len(first)} chains of the key frame's first row")
        assert bad > 0, f"pc_seg {pc_seg}: every guess is right, the loop does not iterate"


@pytest.mark.gpu
@pytest.mark.parametrize("content", list(CONTENTS))
@pytest.mark.parametrize("pc_seg", PC_SEGS)
def test_pc_seg(pc_seg, content, monkeypatch):
    xu.need_gpu()
    kind, seg = CONTENTS[content]
    _hip_equals(monkeypatch, _hevc_run(kind), seg, SK_HEVC_PC_SEG=pc_seg)


# ---- SK_HEVC_REG_STEPS ---------------------------------------------------------------------------
# name: (stripe_height, SK_HEVC_SEG_CTBS): the kernel that codes the intra units
REG_CASES = {"rows-intra4": (64, None), "rows-intra15": (160, None), "seg3": (64, "3")}


def _reg_run(stripe):
    # the content of test_hevc.py test_hevc_coding_quadtree at 200 x 100
    return _hevc_run("desktop", 200, 100, frames=3, qp=32, paint_qp=32, rate_control="cqp", stripe_height=stripe)


@pytest.mark.parametrize("name", list(REG_CASES))
def test_reg_steps_reach(name, monkeypatch):
    """Key frames with CU8s, PART_NxN and 4x4 TUs in the CPU reference, in the slice layout that sends
    the HIP back end to the kernel the case is named after (launch_code, hevc_kernels.hip)."""
    stripe, seg = REG_CASES[name]
    r = _reg_run(stripe)
    snaps = _cpu(monkeypatch, r, seg, all_key=True)
    # launch_code: k_hevc_intra<4> up to four CTB rows per stripe, else k_hevc_intra<15>; the picture's
    # four CTB rows are then one slice, one wave each
    assert (stripe // 32 > 4) == (name == "rows-intra15") and (len(snaps[0]["tasks"]) == 1) == (stripe // 32 > 4)
    for t, s in enumerate(snaps):
        assert s["packets"][0][2] and (s["tasks"]["final_action"] == 2).all(), f"frame {t} is not a key frame"
        cus = s["cus"]
        cu8 = cus[:, 21]
        assert (cu8 & 16).any(), f"frame {t}: no CU8"
        assert (((cu8 & 16) != 0) & ((cu8 & 15) != 0)).any(), f"frame {t}: no PART_NxN"
        assert (((cus[:, 6] & 16) != 0) & ((cus[:, 6] & 15) != 0)).any(), f"frame {t}: no 4x4 TU"
        assert (hevc_slice_nals(s["packets"][0][3]) > (r[2] + 31) // 32) == (seg is not None)
    xu.assert_decodes(r, snaps, f"{name}: CPU")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(REG_CASES))
def test_reg_steps_off(name, monkeypatch):
    xu.need_gpu()
    stripe, seg = REG_CASES[name]
    _hip_equals(monkeypatch, _reg_run(stripe), seg, all_key=True, SK_HEVC_REG_STEPS=0)


@pytest.mark.gpu
def test_tall_stripes(monkeypatch):
    """k_hevc_intra<15> on its default path (4x4 TUs in registers)."""
    xu.need_gpu()
    stripe, seg = REG_CASES["rows-intra15"]
    _hip_equals(monkeypatch, _reg_run(stripe), seg, all_key=True)


# ---- SK_NO_GRAPHS, SK_UPLOAD_MODE ----------------------------------------------------------------
def _dynamics(monkeypatch, name, pacing, **switch):
    xu.need_gpu()
    r = CASES[name]
    ref = du.reference(r)
    _env(monkeypatch, **switch)
    got = du.drive(r, "hip", pacing)
    who = f"{name} {pacing} {switch}"
    if pacing == "serial":
        from tests.test_session_dynamics import _assert_serial_same
        _assert_serial_same(r, got, ref, who)
    du.assert_packets_equal(got["packets"], ref["packets"], who)
    du.assert_end_state_equal(got, ref, who)


@pytest.mark.gpu
@pytest.mark.parametrize("pacing", ["serial", "two"])
@pytest.mark.parametrize("name", DYN_A)
def test_no_graphs(name, pacing, monkeypatch):
    """The control script without graphs: the key / QP / rate snapshot of launch(), the CBR guard's
    gated second pass and parts 1 / 2 (commit with and without deblocking) as plain launches."""
    _dynamics(monkeypatch, name, pacing, SK_NO_GRAPHS=1)


@pytest.mark.gpu
@pytest.mark.parametrize("pacing", ["overlapped", "two"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", DYN_D + DYN_A)
def test_upload_mode(name, mode, pacing, monkeypatch):
    """Damage rows and replaced uploads (d), and the control script (a), with the upload that meets a
    frame in flight on the session stream (0: behind that frame) or on the session's own upload
    stream (1: beside it, ordered by the slot's events)."""
    _dynamics(monkeypatch, name, pacing, SK_UPLOAD_MODE=mode)
