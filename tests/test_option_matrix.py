"""Encoder options in combination, every codec: a pairwise matrix of the options through the scripted
session of tests/test_session_dynamics.py, the HIP back end against the CPU reference.

Every option has a GPU test of its own that turns on that option alone, and the HIP back end chooses
code by option (AV1 template instantiations by tools word, fused and unfused H.264 chains, HEVC row
segments, graphs with and without the CBR guard); the CPU reference shares none of that selection.
tests/matrix_util.py builds, per codec, rows in which every allowed pair of option values occurs
(H.264 12 rows, HEVC 8, AV1 12 with its seed; test_pairs_are_covered prints the counts). One session
per row: the frames "A10 B3 A3 C2 B2" and the control script of test_session_dynamics.py (key request,
set_qp(36), a CBR stretch, back to CRF, set_qp(20)), so every row also crosses its options with the
long-term cache's switch back, the graphs re-captured for the CBR guard and a second coding pass.

CPU tier: the independent decoder returns the reference's reconstruction of every frame of every
row, and every option value other than the default acts in at least one row that carries it
(test_every_option_acts, which prints the table row x option x reached).
GPU tier, per row: the production pacing with two frames in flight (packets with their frame ids,
the final reference picture, the rate controller's state), and the serial pacing, in which the
debug buffers belong to the frame just finished: slice decisions and QPs, block / CU / MB records,
levels and all three reconstruction planes of every frame. With a second frame in flight the
buffers follow the later launch, and reading them waits for the stream, which would take the
overlap away; so the records are compared in the serial run. The HIP packets equal the CPU's, whose
decoding the CPU tier checks."""
import pytest

from selkies_gstreamer_amd.models.av1 import dav1d
from tests import dynamics_util as du
from tests import extremes_util as xu
from tests import matrix_util as mu
from tests.test_session_dynamics import _assert_serial_same, control

CASES = {mu.row_id(codec, k, row): (codec, row) for codec in mu.ROWS for k, row in enumerate(mu.ROWS[codec])}

# The option values that have to act in a row that carries them, by the names matrix_util.reached gives.
MUST_ACT = {
    "h264": ("intra4x4", "num_refs=2", "ltr_slots=2", "aq_strength", "deblock=True", "paint", "redos"),
    "hevc": ("ltr_slots=1", "ltr_slots=2", "SEG_CTBS", "paint", "redos"),
    "av1": ("intra_inter", "chroma_palette", "cfl", "palette_cluster", "ltr_slots=2", "ltr_slots=7",
            "tiles=(1, 1)", "tiles=(2, 0)", "PALETTE=0", "redos"),
}


def _case(name):
    codec, row = CASES[name]
    return mu.case(codec, row, control(codec))


# ---- CPU tier ------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", list(mu.AXES))
def test_pairs_are_covered(codec):
    """Every allowed (value of one axis, value of another axis) occurs in a row, every row is allowed
    and complete, and the generator gives the same rows again."""
    axes, rows = mu.AXES[codec], mu.ROWS[codec]
    want = mu.allowed_pairs(axes, lambda row: mu.allowed(codec, row))
    got = set()
    for row in rows:
        assert list(row) == list(axes) and all(row[n] in axes[n] for n in axes), row
        assert mu.allowed(codec, row), row
        got |= mu._pairs_of(row, list(axes))
    assert not want - got, sorted(want - got, key=repr)[:5]
    # the constraint took pairs away, and only those
    every = mu.allowed_pairs(axes, lambda row: True)
    assert all(not mu.allowed(codec, dict(p)) for p in every - want)
    assert (len(every) > len(want)) == (codec == "h264")
    again = mu.pairwise(axes, lambda row: mu.allowed(codec, row))
    assert again == rows[:len(again)] and rows[len(again):] == mu.EXTRA[codec]
    print(f"{codec}: {len(rows)} rows ({len(mu.EXTRA[codec])} by hand) hold {len(want)} pairs")


def test_generator_on_a_small_table():
    """Three axes of 3, 2 and 2 values with one pair forbidden: all other pairs, no forbidden one."""
    axes = dict(a=(0, 1, 2), b=("x", "y"), c=(False, True))
    ok = lambda row: not (row.get("a") == 2 and row.get("b") == "y")   # noqa: E731
    rows = mu.pairwise(axes, ok, seed=5)
    assert all(ok(r) for r in rows) and 6 <= len(rows) <= 8
    got = set().union(*(mu._pairs_of(r, list(axes)) for r in rows))
    assert got == mu.allowed_pairs(axes, ok) and len(got) == 6 + 6 + 4 - 1


@pytest.mark.parametrize("name", list(CASES))
def test_reference_decodes(name, monkeypatch):
    if CASES[name][0] == "av1" and not dav1d.available():
        pytest.skip("dav1d (Pillow libavif) not available")
    c = _case(name)
    xu.assert_decodes(c[0], mu.reference(monkeypatch, c)["snaps"], f"{name}: CPU")


@pytest.mark.parametrize("codec", list(mu.AXES))
def test_every_option_acts(codec, monkeypatch):
    """Asserted on the CPU reference (matrix_util.reached says how each is read): a row that merely
    carries an option whose code never runs would compare nothing."""
    table = {}
    for name, (cd, row) in CASES.items():
        if cd != codec:
            continue
        plain = None
        if codec == "h264" and row["deblock"] is True:
            plain = mu.reference(monkeypatch, mu.case(codec, dict(row, deblock="auto"), control(codec)))
        table[name] = mu.reached(codec, row, mu.reference(monkeypatch, _case(name)), plain)
    feats = MUST_ACT[codec]
    print(f"\n{'row':<100} " + " ".join(feats))
    for name, got in table.items():
        print(f"{name:<100} " + " ".join(f"{('yes' if got[f] else 'NO') if f in got else '-':<{len(f)}}" for f in feats))
    assert {f for got in table.values() for f in got} == set(feats), "an option value without a reader, or the reverse"
    for f in feats:
        assert any(got.get(f) for got in table.values()), f"{codec}: {f} acts in no row"
    if codec == "av1":   # the palette switch takes something away: a row without it has luma palettes
        assert any((s["blk"][:, 10] & 15).any() for name, (cd, row) in CASES.items() if cd == codec and
                   row["SK_AV1_PALETTE"] is None for s in mu.reference(monkeypatch, _case(name))["snaps"])


# ---- GPU tier ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_two_in_flight(name, monkeypatch):
    xu.need_gpu()
    c = _case(name)
    ref = mu.reference(monkeypatch, c)
    got = du.drive(c[0], "hip", "two")
    du.assert_packets_equal(got["packets"], ref["packets"], name)
    du.assert_end_state_equal(got, ref, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_serial_records(name, monkeypatch):
    xu.need_gpu()
    c = _case(name)
    r = c[0]
    ref = mu.reference(monkeypatch, c)
    got = du.drive(r, "hip", "serial")
    if r[0] == "h264":
        from tests.test_h264_gpu import _compare_state
        for t, (g, s) in enumerate(zip(got["snaps"], ref["snaps"])):
            _compare_state(xu.Recorded(s), xu.Recorded(g), r[1], t)
    _assert_serial_same(r, got, ref, name)
    du.assert_packets_equal(got["packets"], ref["packets"], name)
    du.assert_end_state_equal(got, ref, name)
