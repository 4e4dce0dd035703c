"""bench.py --dump-outputs and the plain / --full split, rehearsed on the CPU encoder:
a plain run runs no end-to-end check and no extra session, and two runs with the same
arguments dump the same packets, on the capture path and through the encoder API."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, STRIPE, SESSIONS = 128, 96, 64, 2


def bench(out_dir, path):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--backend", "cpu",
           "--width", str(W), "--height", str(H), "--sessions", str(SESSIONS), "--path", path,
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return res, np.load(out_dir / "packets.npy"), np.load(out_dir / "packet_index.npy")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_outputs")
    return {"capture": bench(d / "capture", "capture"), "capture2": bench(d / "capture2", "capture"),
            "encoder": bench(d / "encoder", "encoder")}


def test_plain_run_is_the_timed_window_only(runs):
    res = runs["capture"][0]
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert abs(res["value"] - SESSIONS * 1e3 / res["ms_per_step"]) <= 0.01 * res["value"]
    assert res["e2e"] is None and res["e2e_av1_4k"] is None and res["concurrent_60fps_sessions"] is None
    assert not [k for k in res if k.startswith(("hevc_", "av1_", "cpu_480p"))]


def test_dump_is_every_packet_of_the_last_step(runs):
    _, packets, index = runs["capture"]
    assert packets.dtype == np.float32 and index.dtype == np.float64
    stripes = -(-H // STRIPE)
    assert index.shape == (SESSIONS * stripes, 5)
    assert index[:, 0].tolist() == [s for s in range(SESSIONS) for _ in range(stripes)]
    assert index[:, 1].tolist() == [y * STRIPE for _ in range(SESSIONS) for y in range(stripes)]
    assert packets.size == int(index[:, 4].sum()) and (index[:, 4] > 0).all()
    assert packets.min() >= 0 and packets.max() <= 255 and (packets == np.round(packets)).all()


def test_dump_repeats_and_paths_agree(runs):
    _, packets, index = runs["capture"]
    assert np.array_equal(packets, runs["capture2"][1]) and np.array_equal(index, runs["capture2"][2])
    # the encoder API hands back the same bytes (its index carries the key flag where the
    # capture path's carries the stripe result's type)
    assert np.array_equal(packets, runs["encoder"][1])
    assert np.array_equal(index[:, [0, 1, 2, 4]], runs["encoder"][2][:, [0, 1, 2, 4]])
