"""Per-frame trace of the long-term reference cache (csrc/codec/ltr.h): the `ltr_state` and `ltr_task`
debug buffers after every frame of a window-switch sequence, for H.264 (striped and full frame),
HEVC (default expiry age and a small one) and AV1, each with one and two slots.

    python tools/ltr_trace.py            # record tests/golden/ltr_traces.npz on the CPU back end

tests/test_ltr_traces.py replays the same cases on both back ends and requires equality with the
fixture, so a change to the cache's shared code shows even where CPU and GPU still agree. Recording
asserts that every case stores and matches, that a one-slot case evicts, and that the small-age
HEVC case expires a slot; re-record only when a policy change is intended.
"""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from selkies_gstreamer_amd.ops.native import (Av1Encoder, H264Encoder, HevcEncoder,  # noqa: E402
                                              LTR_STATE_DTYPE, LTR_TASK_DTYPE)
from tests.ltr_util import contents, make_enc, sequence  # noqa: E402

FIXTURE = ROOT / "tests" / "golden" / "ltr_traces.npz"
SPEC = "A10 B10 A3 C10 B2 A2 C2"
SMALL_AGE = 12   # pictures: the picture stored at frame 20 (POC 19) expires at frame 31, while C is shown
AGE_ENV = "SK_HEVC_LTR_MAX_AGE"

# name -> (encoder class, extra configuration, expiry age or None, caret)
# AV1: without the caret; at 13 x 7 MBs the caret's tile row is never quiet (tests/av1_ltr_util.py frames)
CASES = {}
for _slots in (1, 2):
    CASES[f"h264_striped_s{_slots}"] = (H264Encoder, dict(fullframe=False), None, True)
    CASES[f"h264_full_s{_slots}"] = (H264Encoder, dict(fullframe=True), None, True)
    CASES[f"hevc_s{_slots}"] = (HevcEncoder, {}, None, True)
    CASES[f"hevc_age_s{_slots}"] = (HevcEncoder, {}, SMALL_AGE, True)
    CASES[f"av1_s{_slots}"] = (Av1Encoder, {}, None, False)


def slots_of(case: str) -> int:
    return int(case[-1])


def frames(caret: bool) -> list:
    """The sequence's frames and one more of the last content: on the HIP back end a frame's state is
    committed on the device by the next frame's plan, which that frame's trace then shows."""
    if caret:
        out = [f for _, _, f in sequence(SPEC)]
    else:
        c = contents()
        out = [c[item[0]] for item in SPEC.split() for _ in range(int(item[1:]))]
    return out + [out[-1]]


def run(case: str, backend: str = "cpu"):
    """-> (state [frames][streams] LTR_STATE_DTYPE, task [frames][slices] LTR_TASK_DTYPE)"""
    cls, kw, age, caret = CASES[case]
    old = os.environ.get(AGE_ENV)
    os.environ.pop(AGE_ENV, None)
    if age is not None:
        os.environ[AGE_ENV] = str(age)
    try:   # the age is read when the encoder is built
        enc = make_enc(cls, slots_of(case), backend=backend, **kw)
    finally:
        os.environ.pop(AGE_ENV, None)
        if old is not None:
            os.environ[AGE_ENV] = old
    state, task = [], []
    for t, f in enumerate(frames(caret)):
        enc.encode(f, t)
        state.append(enc.debug_buffer("ltr_state", LTR_STATE_DTYPE).copy())
        task.append(enc.debug_buffer("ltr_task", LTR_TASK_DTYPE).copy())
    return np.stack(state), np.stack(task)


def as_words(a: np.ndarray) -> np.ndarray:
    """A structured trace as the int32 words the fixture holds, [frames][items][words]."""
    return a.view(np.int32).reshape(a.shape[0], a.shape[1], -1)


def check_conditions(case: str, state: np.ndarray, task: np.ndarray) -> None:
    """What a recorded case must exercise, from the trace alone."""
    assert (task["store_slot"] >= 0).any(), f"{case}: no store"
    assert (task["slot"] >= 0).any(), f"{case}: no match"
    nstreams = state.shape[1]
    stream = (lambda s: s) if case.startswith("h264_striped") else (lambda s: nstreams - 1)
    if slots_of(case) == 1:   # a store into a slot that is valid before the frame
        evict = any(task["store_slot"][t, s] >= 0 and
                    (state["valid"][t - 1, stream(s)] >> task["store_slot"][t, s]) & 1
                    for t in range(1, task.shape[0]) for s in range(task.shape[1]))
        assert evict, f"{case}: no eviction"
    if case.startswith("hevc_age"):   # a valid bit that falls without a key picture's reset (which zeroes the clock)
        v, clock = state["valid"][:, -1], state["clock"][:, -1]
        assert any(v[t - 1] & ~v[t] and clock[t] >= clock[t - 1] for t in range(1, len(v))), f"{case}: no expiry"


def main():
    out = {}
    for case in CASES:
        state, task = run(case)
        check_conditions(case, state, task)
        out[case + "_state"], out[case + "_task"] = as_words(state), as_words(task)
        print(f"{case}: {state.shape[0]} frames, {state.shape[1]} streams, "
              f"{int((task['store_slot'][:, 0] >= 0).sum())} stores, {int((task['slot'] >= 0).any(axis=1).sum())} matched frames")
    FIXTURE.parent.mkdir(exist_ok=True)
    np.savez_compressed(FIXTURE, **out)
    print(f"wrote {FIXTURE} ({FIXTURE.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
