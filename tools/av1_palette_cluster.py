"""AV1 clustered luma palettes (Av1Encoder(palette_cluster=True)) against the same session without the
option, from the bare encoder.

    python tools/av1_palette_cluster.py --rd                           # CPU: bytes, luma PSNR, BD-rate
    python tools/av1_palette_cluster.py --width 1920 --height 1080     # HIP: encode time and bytes

RD mode (--rd): the CPU encoder at QP 16, 20, 25, 30 and 38, option on against off, intra_inter,
chroma_palette and cfl on in both, at 256x128: a key frame and two shifted frames of the two
anti-aliased contents of tests/av1_palette_cluster_util.py (`aa`: coloured text, 4x box anti-aliasing,
9 luma values per unit; `soft`: grey text, soft 8x anti-aliasing, 14 values), the two-colour window
sequence of tests/av1_intra_inter_util.py and eight frames of SyntheticDesktop "motion". Prints total
bytes and mean luma PSNR per QP, the cells of clustered blocks, and the BD-rate of on against off (the
mean difference of log rate over the PSNR range both curves cover, cubic fit; negative: fewer bytes at
equal PSNR).

Timing mode: one encoder per setting in the same process (intra_inter on in both), fed the same
frames: a key frame of the synthetic desktop (forced every round), the desktop held still, then a
window of aa_field that opens and stays, `--reps` times after a warm-up. `--content aa` makes the
whole picture aa_field (the key frame where every block is a candidate). Prints the median and the
spread of the key frames', the window frames' and the steady frames' encode time, and the key and
window frames' bytes. `--off-only` never names the option, so it also runs on a library built without
it: the figure to compare with another build of the project."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from selkies_gstreamer_amd.ops.native import Av1Encoder  # noqa: E402
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop  # noqa: E402
from tests import av1_chroma_palette_util as C  # noqa: E402
from tests import av1_intra_inter_util as U  # noqa: E402
from tests import av1_palette_cluster_util as P  # noqa: E402
from tests.ltr_util import ref_planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--reps", type=int, default=16)
ap.add_argument("--qp", type=int, default=20)
ap.add_argument("--backend", default="hip")
ap.add_argument("--content", default="desktop", choices=("desktop", "aa"), help="timing: the picture under the window")
ap.add_argument("--rd", action="store_true")
ap.add_argument("--off-only", action="store_true", help="timing: the option-off encoder alone (also runs on a "
                "build without the option)")
a = ap.parse_args()
QPS = (16, 20, 25, 30, 38)


def bd_rate(off, on) -> float:
    """Bjontegaard delta rate in percent of the (bytes, dB) points `on` against `off`."""
    (r0, p0), (r1, p1) = (np.array(sorted(x, key=lambda t: t[1])).T for x in (off, on))
    f0, f1 = np.polyfit(p0, np.log(r0), 3), np.polyfit(p1, np.log(r1), 3)
    lo, hi = max(p0.min(), p1.min()), min(p0.max(), p1.max())
    i0, i1 = np.polyint(f0), np.polyint(f1)
    d = ((np.polyval(i1, hi) - np.polyval(i1, lo)) - (np.polyval(i0, hi) - np.polyval(i0, lo))) / (hi - lo)
    return float((np.exp(d) - 1) * 100)


def rd():
    w, h = 256, 128
    contents = (("aa", P.shifted_frames(P.aa_field, w, h)), ("soft", P.shifted_frames(P.soft_field, w, h)),
                ("window", U.frames(w, h)), ("motion", [SyntheticDesktop(w, h, kind="motion").frame(t) for t in range(8)]))
    for name, seq in contents:
        pts = {False: [], True: []}
        for qp in QPS:
            row = []
            for on in (False, True):
                enc = Av1Encoder(w, h, backend="cpu", qp=qp, intra_inter=True, chroma_palette=True, cfl=True,
                                 **({"palette_cluster": True} if on else {}))
                nb, ps, ncl = 0, [], 0
                for t, f in enumerate(seq):
                    pk = enc.encode(f, t)
                    nb += len(pk[0].data)
                    src = C.src_planes(enc, w, h)
                    ps.append(P.luma_psnr(src, ref_planes(enc, w, h)))
                    ncl += int(P.clustered(src[0], C.cells(enc, w, h)).sum())
                row.append((nb, float(np.mean(ps)), ncl))
                pts[on].append((nb, row[-1][1]))
            (b0, p0, _), (b1, p1, n1) = row
            print(f"{name:7s} qp {qp}: off {b0:6d} B {p0:6.2f} dB | on {b1:6d} B {p1:6.2f} dB | "
                  f"{100.0 * (b1 - b0) / b0:+6.2f} % bytes {p1 - p0:+5.2f} dB luma, {n1} cells clustered", flush=True)
        same = pts[True] == pts[False]
        print(f"{name:7s} BD-rate {'0.00 (identical points)' if same else '%+.2f' % bd_rate(pts[False], pts[True])} %", flush=True)


def window(f: np.ndarray, content: np.ndarray) -> np.ndarray:
    """`content` in the window's rectangle of BGRx frame f."""
    h, w = f.shape[:2]
    x0, y0, ww, wh = U.window_rect(w, h)
    f[y0:y0 + wh, x0:x0 + ww] = content[:wh, :ww]
    return f


def timing():
    w, h = a.width, a.height
    desk = P.aa_field(w, h, 6) if a.content == "aa" else SyntheticDesktop(w, h, kind="desktop").frame(0)
    win = window(desk.copy(), P.aa_field(w, h, 0))
    kw = dict(backend=a.backend, qp=a.qp, intra_inter=True, use_paint_over=False)
    encs = {False: Av1Encoder(w, h, **kw)}
    if not a.off_only:
        encs[True] = Av1Encoder(w, h, palette_cluster=True, **kw)
    res = {on: {"key_ms": [], "key_b": [], "win_ms": [], "win_b": [], "steady_ms": []} for on in encs}
    t = 0
    for rep in range(-3, a.reps):    # three warm-up rounds
        for k, f in enumerate((desk, desk, desk, win, win, win)):
            for on, enc in encs.items():
                if k == 0:
                    enc.request_keyframe()
                t0 = time.perf_counter()
                pk = enc.encode(f, t)
                dt = (time.perf_counter() - t0) * 1e3
                if rep < 0:
                    continue
                if k == 0:
                    assert pk[0].key
                    res[on]["key_ms"].append(dt)
                    res[on]["key_b"].append(len(pk[0].data))
                elif k == 3:
                    res[on]["win_ms"].append(dt)
                    res[on]["win_b"].append(len(pk[0].data))
                elif k in (2, 5):
                    res[on]["steady_ms"].append(dt)
            t += 1

    def stat(x):
        x = np.array(x)
        return f"n={len(x)} median {np.median(x):.3f} ms (min {x.min():.3f}, p90 {np.percentile(x, 90):.3f})"
    for on, r in res.items():
        print(f"{w}x{h} {a.content} qp {a.qp} palette_cluster={int(on)}: key frame {stat(r['key_ms'])}, "
              f"{int(np.median(r['key_b']))} bytes | window frame {stat(r['win_ms'])}, {int(np.median(r['win_b']))} bytes | "
              f"steady {stat(r['steady_ms'])}", flush=True)
    for enc in encs.values():
        enc.close()


rd() if a.rd else timing()
