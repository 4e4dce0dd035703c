"""AV1 intra blocks in inter frames (Av1Encoder(intra_inter=True)) against the same session
without the option, from the bare encoder.

    python tools/av1_intra_inter.py --width 1920 --height 1080            # HIP: encode time and bytes
    python tools/av1_intra_inter.py --rd                                  # CPU: bytes and Y-PSNR (the bias runs)

Timing mode: one encoder per setting in the same process, fed the same frames. A window
(tests/av1_intra_inter_util.py's content) opens over a still synthetic desktop and closes again,
`--reps` times after a warm-up; between the two every frame repeats the one before (steady state:
no block keeps a residual, so the option has no candidate). Prints the median and the spread of
the window frames' and of the steady frames' encode time, and the window frames' bytes.
--once: key frame, desktop, one window frame, for a kernel trace of an option-on window frame
(rocprofv3 --kernel-trace --stats -- python tools/av1_intra_inter.py --once ...).

RD mode (--rd): the test sequence and SyntheticDesktop "motion" at three QPs on the CPU encoder,
option on against off: total bytes and mean luma PSNR of the inter frames."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from selkies_gstreamer_amd.ops.native import Av1Encoder  # noqa: E402
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop  # noqa: E402
from tests import av1_intra_inter_util as U  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--qp", type=int, default=25)
ap.add_argument("--backend", default="hip")
ap.add_argument("--once", action="store_true")
ap.add_argument("--rd", action="store_true")
a = ap.parse_args()


def psnr(x, y):
    mse = np.mean((x.astype(np.float64) - y.astype(np.float64)) ** 2)
    return 99.0 if mse == 0 else 10 * np.log10(255 * 255 / mse)


def rd():
    for name, w, h, seq in (("window", 640, 360, U.frames(640, 360)),
                            ("motion", 640, 360, [SyntheticDesktop(640, 360, kind="motion").frame(t) for t in range(8)])):
        for qp in (20, 28, 36):
            row = []
            for on in (False, True):
                enc = Av1Encoder(w, h, backend="cpu", qp=qp, intra_inter=on)
                nb, ps, ni = 0, [], 0
                for t, f in enumerate(seq):
                    pk = enc.encode(f, t)
                    if t == 0:
                        continue
                    nb += len(pk[0].data)
                    ps.append(psnr(U.src_luma(enc, w, h), enc.debug_buffer("ref_y").reshape(-1, (w + 15) // 16 * 16)[:h, :w]))
                    ni += int(U.intra_cells(enc, w, h).sum())
                row.append((nb, float(np.mean(ps)), ni))
            (b0, p0, _), (b1, p1, n1) = row
            print(f"{name:7s} qp {qp}: off {b0:7d} B {p0:6.2f} dB | on {b1:7d} B {p1:6.2f} dB | "
                  f"{100.0 * (b1 - b0) / b0:+6.1f} % bytes {p1 - p0:+5.2f} dB, {n1} intra cells", flush=True)


def timing():
    w, h = a.width, a.height
    desk = SyntheticDesktop(w, h, kind="desktop").frame(0)
    win = U.draw_window(desk.copy())
    encs = {on: Av1Encoder(w, h, backend=a.backend, qp=a.qp, intra_inter=on, use_paint_over=False) for on in (False, True)}
    if a.once:
        for t, f in enumerate((desk, desk, win)):
            pk = encs[True].encode(f, t)
        print(f"window frame: {len(pk[0].data)} bytes, {int(U.intra_cells(encs[True], w, h).sum())} intra cells")
        return
    res = {on: {"win_ms": [], "win_b": [], "steady_ms": []} for on in encs}
    t = 0
    for rep in range(-3, a.reps):    # three warm-up rounds
        for k, f in enumerate((desk, desk, desk, win, win, win)):
            for on, enc in encs.items():
                t0 = time.perf_counter()
                pk = enc.encode(f, t)
                dt = (time.perf_counter() - t0) * 1e3
                if rep >= 0 and k == 3:
                    res[on]["win_ms"].append(dt)
                    res[on]["win_b"].append(len(pk[0].data))
                elif rep >= 0 and k in (2, 5):
                    res[on]["steady_ms"].append(dt)
            t += 1
    for on in (False, True):
        r = res[on]
        wm, sm = np.array(r["win_ms"]), np.array(r["steady_ms"])
        print(f"{w}x{h} intra_inter={int(on)}: window frame n={len(wm)} median {np.median(wm):.3f} ms "
              f"(min {wm.min():.3f}, p90 {np.percentile(wm, 90):.3f}), {int(np.median(r['win_b']))} bytes | "
              f"steady n={len(sm)} median {np.median(sm):.3f} ms (min {sm.min():.3f}, p90 {np.percentile(sm, 90):.3f})",
              flush=True)
    for enc in encs.values():
        enc.close()


rd() if a.rd else timing()
