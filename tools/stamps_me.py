"""Diagnostic: per-phase cycle shares of k_me (wave 0 of workgroup SK_STAMP_BLOCK, last frame).

Needs the stamps library, built for a workgroup in the middle of the picture:
SK_STAMPS_BUILD=1 SK_STAMP_BLOCK=1000 python -m selkies_gstreamer_amd.ops.build
(-> _lib/libselkies_native_stamps.so); this script selects it and sets SK_STAMPS=1."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ["SK_STAMPS"] = "1"
os.environ["SK_NATIVE_LIB"] = os.path.join(ROOT, "selkies_gstreamer_amd", "_lib", "libselkies_native_stamps.so")
sys.path.insert(0, ROOT)
from selkies_gstreamer_amd.ops.native import H264Encoder
from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
W, H = 1920, 1080
src = SyntheticDesktop(W, H, "motion")
enc = H264Encoder(W, H, stripe_height=64, backend="hip")
# points of stamp row 63: 0 start, 1 exact-match test done, 2 window filled, 3 row sums, 4 column
# sums, 5 MFMA loop, 6 key reduction, 7 predictor SADs, 8 diamond, 9 activity / second reference / store
names = ["exact-match test", "window fill", "row sums", "column sums", "MFMA loop", "key reduction",
         "predictor SADs", "diamond", "activity + store"]
rows = []
for t in range(12):
    enc.encode(src.frame(t), t)
    r = enc.debug_buffer("stamps", np.uint64).astype(np.int64)[:1024].reshape(64, 16)[63, :10]
    if t >= 2 and (r > 0).all() and (np.diff(r) >= 0).all():
        rows.append(np.diff(r))
if not rows:
    sys.exit("no frame in which the stamped wave ran the full search")
med = np.median(np.array(rows), axis=0)
print(f"k_me phases, s_memtime cycles, median of {len(rows)} frames, total {med.sum():.0f}")
for n, v in zip(names, med):
    print(f"{n:18s} {v:7.0f} {100 * v / med.sum():5.1f} %")
