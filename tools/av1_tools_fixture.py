"""Writes tests/golden/av1_tools_streams.json: SHA-256 digests of every temporal unit and of the three
reconstruction planes of the CPU AV1 encoder over the sequence of tests/av1_tools_util.py, for all 16
combinations of the tools (chroma_palette, cfl, palette_cluster as mask bits 0..2, intra_inter off / on).

    python tools/av1_tools_fixture.py --commit f290c0e      # writes the fixture
    python tools/av1_tools_fixture.py --check               # compares this build with the fixture

Through the public Av1Encoder API only, so it runs on any build of the project that has the four
options. `--commit` names the commit whose library produced the digests; the file records it. Before
writing, the script checks that every enabled tool has at least one block that took it, and that the
sessions with intra_inter hold an intra cell in an inter frame: the fixture is only worth keeping on
content that exercises what it pins."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import av1_tools_util as T  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "av1_tools_streams.json")
ap = argparse.ArgumentParser()
ap.add_argument("--commit", default="", help="the commit whose library runs (recorded in the file)")
ap.add_argument("--check", action="store_true")
a = ap.parse_args()

cases = {}
for mask, ii in T.CASES:
    res = T.run_cpu(mask, ii)
    used = {k: any(f["took"][k] for f in res) for k in res[0]["took"]}
    print(T.case_id(mask, ii), used, flush=True)
    for name, on in T.case_kwargs(mask, ii).items():
        assert used[name] == on, f"{T.case_id(mask, ii)}: {name} enabled={on}, taken={used[name]}"
    cases[T.case_id(mask, ii)] = [{"tu": f["tu"], "rec": f["rec"]} for f in res]

if a.check:
    want = json.load(open(PATH))["cases"]
    bad = [k for k in cases if cases[k] != want[k]]
    print("identical to the fixture" if not bad else f"differs from the fixture: {bad}")
    sys.exit(1 if bad else 0)
doc = {"generated_by": "tools/av1_tools_fixture.py", "library_commit": a.commit,
       "note": "CPU encoder (backend=cpu), %dx%d, three frames, QP %d; digests are SHA-256" % (T.W, T.H, T.QP),
       "cases": cases}
with open(PATH, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print(f"wrote {PATH}")
