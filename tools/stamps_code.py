"""Diagnostic: per-phase cycle shares of one k_code_inter wave (wave 0 of workgroup SK_STAMP_BLOCK),
by what became of its macroblock: all levels zero after the quantiser, decimated to cbp 0, coded.

Needs the stamps library, built for a workgroup in the middle of the picture:
SK_STAMPS_BUILD=1 SK_STAMP_BLOCK=1000 python -m selkies_gstreamer_amd.ops.build
(-> _lib/libselkies_native_stamps.so); this script selects it (or the library given as its
first argument) and sets SK_STAMPS=1. The stamps wait for LDS and scalar loads only: a global
load is charged to the phase that first uses its result (the fetch to the transform)."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["SK_STAMPS"] = "1"
os.environ["SK_NATIVE_LIB"] = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(
    ROOT, "selkies_gstreamer_amd", "_lib", "libselkies_native_stamps.so")
sys.path.insert(0, ROOT)
from selkies_gstreamer_amd.ops.native import H264Encoder
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
W, H = 1920, 1080
ROW = 62   # kCodeStampRow
# stamp points in the order a wave passes them; 11, 12 and 5 are not passed by a wave on the fast path
ORDER = [0, 1, 2, 3, 9, 10, 11, 12, 4, 5, 6, 7, 8]
NAMES = {1: "neighbour vectors", 2: "source + prediction fetch", 3: "transform", 9: "quantisation + LDS writes",
         10: "chroma DC", 11: "cbp analysis", 12: "bound", 4: "QP loop end", 5: "reconstruction",
         6: "level store", 7: "rec store", 8: "MbInfo store"}
KINDS = {1: "all levels zero", 2: "decimated to cbp 0", 3: "luma or chroma coded"}
src = SyntheticDesktop(W, H, "motion")
enc = H264Encoder(W, H, stripe_height=64, backend="hip")
rows = {k: [] for k in KINDS}
last0 = 0
for t in range(120):
    enc.encode(src.frame(t), t)
    r = enc.debug_buffer("stamps", np.uint64).astype(np.int64)[:1024].reshape(64, 16)[ROW]
    if r[0] <= last0 or r[8] < r[0] or int(r[13]) not in KINDS:
        continue   # the stamped wave coded no P macroblock in this frame
    last0 = r[0]
    pts = [p for p in ORDER if r[p] >= r[0]]   # a stamp older than this frame's start: not passed
    d = dict(zip(pts[1:], np.diff(r[pts])))
    if min(d.values()) >= 0:
        rows[int(r[13])].append(d)
if not any(rows.values()):
    sys.exit("no frame in which the stamped wave coded a P macroblock")
for k, name in KINDS.items():
    if not rows[k]:
        print(f"\n{name}: not seen")
        continue
    med = {p: float(np.median([d.get(p, 0) for d in rows[k]])) for p in ORDER[1:]}
    total = sum(med.values())
    print(f"\n{name}: s_memtime cycles, median of {len(rows[k])} frames, total {total:.0f}")
    for p in ORDER[1:]:
        print(f"{NAMES[p]:28s} {med[p]:7.0f} {100 * med[p] / total:5.1f} %")
