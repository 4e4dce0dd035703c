"""The AV1 encoder's tools in all 16 combinations (chroma_palette, cfl, palette_cluster; intra_inter off /
on) on the CPU back end against recorded digests: every temporal unit and every reconstruction plane
of the sequence of av1_tools_util.py equals what the library of the commit named in
tests/golden/av1_tools_streams.json produced (tools/av1_tools_fixture.py writes that file). The
content exercises what the digests pin: every enabled tool is taken by at least one block of the
sequence, and a session with intra_inter holds an intra cell in an inter frame."""
import json
from pathlib import Path

import pytest

from tests import av1_tools_util as T

FIXTURE = json.loads((Path(__file__).parent / "golden" / "av1_tools_streams.json").read_text())


def test_fixture_names_its_library():
    assert FIXTURE["library_commit"] == "f290c0e"
    assert set(FIXTURE["cases"]) == {T.case_id(m, ii) for m, ii in T.CASES}


@pytest.mark.parametrize("mask,ii", T.CASES, ids=[T.case_id(m, ii) for m, ii in T.CASES])
def test_streams_equal_the_recorded_ones(mask, ii):
    res = T.run_cpu(mask, ii)
    want = FIXTURE["cases"][T.case_id(mask, ii)]
    assert len(res) == len(want) == 3
    for t, (got, ref) in enumerate(zip(res, want)):
        assert got["tu"] == ref["tu"], f"frame {t}: the temporal unit differs from the recorded one"
        for g, r, n in zip(got["rec"], ref["rec"], "YUV"):
            assert g == r, f"frame {t}: the {n} reconstruction differs from the recorded one"
    for name, on in T.case_kwargs(mask, ii).items():
        taken = any(f["took"][name] for f in res)
        assert taken == on, f"{name}: enabled {on}, a block took it: {taken}"
