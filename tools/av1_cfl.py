"""AV1 chroma from luma (Av1Encoder(cfl=True)) against the same session without the option, from the
bare encoder.

    python tools/av1_cfl.py --width 1920 --height 1080     # HIP: encode time and bytes
    python tools/av1_cfl.py --rd                           # CPU: bytes and chroma PSNR

Timing mode: one encoder per setting in the same process (intra_inter on in both), fed the same
frames: a key frame of the synthetic desktop (forced every round), the desktop held still, then a
window of the hue texture (tests/av1_cfl_util.py: saturated colours, brightness textured) that opens
and stays, `--reps` times after a warm-up. `--content hue` makes the whole picture hue texture (the
key frame where every block is a candidate), `--content grey` the desktop without colour (flat chroma:
no block passes the gate, so on minus off is what every block pays). `--with-palette` adds a third
encoder with chroma_palette=True and CfL off, which keeps the levels in LDS and computes the chroma J
like the CfL kernels but has no CfL pass. Prints the median and the spread of the key frames',
the window frames' and the steady frames' encode time, and the key and window frames' bytes. The
option-off row is also the figure to compare with another build of the project (same content, same
frames): `--off-only` never names the option, so it runs on a library built without it.

RD mode (--rd): the hue-texture window, the glyph-field window and SyntheticDesktop "motion" at QP
25 and 38 on the CPU encoder, option on against off: total bytes, chroma PSNR (both planes) and the
cells that take UV_CFL_PRED."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from selkies_gstreamer_amd.ops.native import Av1Encoder  # noqa: E402
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop  # noqa: E402
from tests import av1_cfl_util as K  # noqa: E402
from tests import av1_chroma_palette_util as C  # noqa: E402
from tests import av1_intra_inter_util as U  # noqa: E402
from tests.ltr_util import ref_planes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--reps", type=int, default=16)
ap.add_argument("--qp", type=int, default=25)
ap.add_argument("--backend", default="hip")
ap.add_argument("--content", default="desktop", choices=("desktop", "hue", "grey"), help="timing: the picture under the window")
ap.add_argument("--with-palette", action="store_true", help="timing: also an encoder with chroma_palette and without CfL")
ap.add_argument("--rd", action="store_true")
ap.add_argument("--off-only", action="store_true", help="timing: the option-off encoder alone (also runs on a "
                "build without the option)")
a = ap.parse_args()


def window(f: np.ndarray, content: np.ndarray) -> np.ndarray:
    """`content` in the window's rectangle of BGRx frame f."""
    h, w = f.shape[:2]
    x0, y0, ww, wh = U.window_rect(w, h)
    f[y0:y0 + wh, x0:x0 + ww] = content[:wh, :ww]
    return f


def psnr_c(src, rec):
    mse = np.mean([np.mean((src[p].astype(np.float64) - rec[p].astype(np.float64)) ** 2) for p in (1, 2)])
    return 99.0 if mse == 0 else 10 * np.log10(255 * 255 / mse)


def rd():
    w, h = 640, 360
    desk = SyntheticDesktop(w, h, kind="desktop").frame(0)
    contents = (("hue", [desk, desk] + [window(desk.copy(), K.hue_texture(w, h, s)) for s in (0, 1, 2)]),
                ("glyphs", [desk, desk] + [window(desk.copy(), C.glyph_field(w, h, s)) for s in (0, 3, 6)]),
                ("motion", [SyntheticDesktop(w, h, kind="motion").frame(t) for t in range(8)]))
    for name, seq in contents:
        for qp in (25, 38):
            row = []
            for on in (False, True):
                enc = Av1Encoder(w, h, backend="cpu", qp=qp, intra_inter=True, cfl=on)
                nb, ps, ncfl, nintra = 0, [], 0, 0
                for t, f in enumerate(seq):
                    pk = enc.encode(f, t)
                    nb += len(pk[0].data)
                    ps.append(psnr_c(C.src_planes(enc, w, h), ref_planes(enc, w, h)))
                    cells = C.cells(enc, w, h)
                    ncfl += int(K.is_cfl(cells).sum())
                    nintra += int(((cells[:, :, K.BLK_FLAGS] & 1) == 0).sum())
                row.append((nb, float(np.mean(ps)), ncfl, nintra))
            (b0, p0, _, _), (b1, p1, n1, i1) = row
            print(f"{name:7s} qp {qp}: off {b0:7d} B {p0:6.2f} dB | on {b1:7d} B {p1:6.2f} dB | "
                  f"{100.0 * (b1 - b0) / b0:+6.2f} % bytes {p1 - p0:+5.2f} dB chroma, {n1} of {i1} intra cells take CfL",
                  flush=True)


def timing():
    w, h = a.width, a.height
    desk = K.hue_texture(w, h, 3) if a.content == "hue" else SyntheticDesktop(w, h, kind="desktop").frame(0)
    if a.content == "grey":
        desk[:, :, :3] = (desk[:, :, :3].astype(np.uint16).sum(axis=2) // 3).astype(np.uint8)[:, :, None]
    win = window(desk.copy(), K.hue_texture(w, h, 0))
    kw = dict(backend=a.backend, qp=a.qp, intra_inter=True, use_paint_over=False)
    encs = {False: Av1Encoder(w, h, **kw)}
    if not a.off_only:
        encs[True] = Av1Encoder(w, h, cfl=True, **kw)
        if a.with_palette:
            encs["palette"] = Av1Encoder(w, h, chroma_palette=True, **kw)
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
        print(f"{w}x{h} {a.content} {'cfl=%d' % on if on != 'palette' else 'chroma_palette'}: key frame {stat(r['key_ms'])}, {int(np.median(r['key_b']))} bytes | "
              f"window frame {stat(r['win_ms'])}, {int(np.median(r['win_b']))} bytes | steady {stat(r['steady_ms'])}",
              flush=True)
    for enc in encs.values():
        enc.close()


rd() if a.rd else timing()
