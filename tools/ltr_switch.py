"""Window switches with and without the long-term reference cache (EncoderConfig::ltr_slots), H.264
(the default), HEVC or AV1 (--codec hevc / av1: one full-frame session per setting).

One 1080p session per mode (striped, full frame) and per setting (ltr_slots 0 and 4) on the
same build, fed the same sequence: two full-screen desktops A and B that alternate, each
shown long enough to settle (a caret blinks meanwhile), then short visits. Prints, per mode
and setting: bytes and host-side encode time of the switch-back frames (the first frame of a
content the session has shown before) and the steady-state frame time (the quiet frames between
switches), with the two settings alternating frame by frame so both see the same machine state.

    python tools/ltr_switch.py [--backend hip|cpu] [--cycles N] [--slots K] [--codec h264|hevc|av1]

Run under `rocprofv3 --kernel-trace --stats -- python tools/ltr_switch.py --only-ltr` for the
k_ltr_match / k_ltr_decide / k_commit times (tools/rocprof_summary.py reads the result).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from selkies_gstreamer_amd.ops.native import Av1Encoder, H264Encoder, HevcEncoder  # noqa: E402
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backend", default="hip", choices=["hip", "cpu"])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--settle", type=int, default=12, help="frames each content is shown before a switch")
    ap.add_argument("--cycles", type=int, default=6, help="A/B switch pairs after both contents were cached")
    ap.add_argument("--codec", default="h264", choices=["h264", "hevc", "av1"])
    ap.add_argument("--only-ltr", action="store_true", help="run only the sessions with the cache (kernel traces)")
    a = ap.parse_args()
    W, H = a.width, a.height
    base = {"A": SyntheticDesktop(W, H, "desktop", seed=5).frame(0),
            "B": np.roll(SyntheticDesktop(W, H, "desktop", seed=9).frame(0), W // 3, axis=1)}
    seq = []   # (content, index in its run)
    for c in range(2 + a.cycles):
        for name in "AB":
            seq += [(name, k) for k in range(a.settle)]
    first_back = 2 * a.settle   # the first frame whose content was shown (and settled) before

    def frame(name, t):
        f = base[name].copy()
        if t & 1:
            f[8:24, 200:202, :3] = 255   # caret
        return f

    def make(mode, s):
        if a.codec == "av1":
            return Av1Encoder(W, H, stripe_height=64, backend=a.backend, use_paint_over=False, ltr_slots=s)
        if a.codec == "hevc":
            return HevcEncoder(W, H, stripe_height=64, backend=a.backend, use_paint_over=False, ltr_slots=s)
        return H264Encoder(W, H, stripe_height=64, fullframe=mode == "fullframe", backend=a.backend,
                           use_paint_over=False, ltr_slots=s)

    for mode in ((a.codec,) if a.codec != "h264" else ("striped", "fullframe")):
        settings = [a.slots] if a.only_ltr else [0, a.slots]
        encs = {s: make(mode, s) for s in settings}
        stats = {s: {"sw_bytes": [], "sw_ms": [], "steady_ms": [], "key": 0} for s in settings}
        for t, (name, k) in enumerate(seq):
            f = frame(name, t)
            order = settings if t % 2 == 0 else settings[::-1]   # alternate which setting goes first
            for s in order:
                t0 = time.perf_counter()
                pk = encs[s].encode(f, t)
                dt = (time.perf_counter() - t0) * 1e3
                if t >= first_back and k == 0:
                    stats[s]["sw_bytes"].append(sum(len(p.data) for p in pk))
                    stats[s]["sw_ms"].append(dt)
                    stats[s]["key"] += any(p.key for p in pk)
                elif t >= first_back and k >= 2:
                    stats[s]["steady_ms"].append(dt)
        for s in settings:
            st = stats[s]
            print(f"{mode:9s} ltr_slots={s}: switch-back frames n={len(st['sw_bytes'])} "
                  f"median {np.median(st['sw_bytes']) / 1024:.1f} KiB, encode median {np.median(st['sw_ms']):.3f} ms "
                  f"(min {min(st['sw_ms']):.3f} max {max(st['sw_ms']):.3f}), key packets {st['key']}; "
                  f"steady frames n={len(st['steady_ms'])} median {np.median(st['steady_ms']):.3f} ms "
                  f"(p10 {np.percentile(st['steady_ms'], 10):.3f} p90 {np.percentile(st['steady_ms'], 90):.3f})")
        if len(settings) == 2:
            r = np.median(stats[a.slots]["sw_bytes"]) / np.median(stats[0]["sw_bytes"])
            print(f"{mode:9s} switch-back bytes with the cache / without: {r:.3f}")


if __name__ == "__main__":
    main()
