"""The long-term reference cache's decisions pinned to a recorded trace (tools/ltr_trace.py,
tests/golden/ltr_traces.npz): LtrState of every stream and LtrTask of every slice after every frame
of a window-switch sequence, H.264 striped and full frame, HEVC with the default and a small expiry
age, AV1, one and two slots. CPU and GPU run the same ltr.h code, so a comparison between them
cannot see a change to it; the fixture can. On the HIP back end the state read after a frame is the
host's commit of it (committed_ltr_state); the device's own commit (k_plan) shows in the next
frame's state, the trailing frame's for the last one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ltr_trace  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(ltr_trace.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _check(case, backend, golden):
    state, task = ltr_trace.run(case, backend)
    ltr_trace.check_conditions(case, state, task)
    for name, got in (("state", ltr_trace.as_words(state)), ("task", ltr_trace.as_words(task))):
        want = golden[f"{case}_{name}"]
        assert want.dtype == np.int32 and got.shape == want.shape
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{case}: ltr_{name} differs first at [frame, item, word] {bad[0].tolist()}"


def test_fixture_holds_every_case(golden):
    assert sorted(golden) == sorted(f"{c}_{n}" for c in ltr_trace.CASES for n in ("state", "task"))


@pytest.mark.parametrize("case", list(ltr_trace.CASES))
def test_ltr_trace_cpu(case, golden):
    _check(case, "cpu", golden)


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(ltr_trace.CASES))
def test_ltr_trace_gpu(case, golden):
    _check(case, "hip", golden)
