"""Layout of the session-state blob (codec/h264_state.h), section by section.

Geometry of tests/test_session_migration.py (160 x 128, 32-pixel stripes, its first four frames).
The section offsets are worked out here from the documented layout

    StateHeader (64) | StripeState[ns + 1] (44 each) | RcState | ref Y U V | ref1 Y U V |
    last source Y U V | MV field int16[2 * MBs] | version 4: LtrState[ns + 1] (96 each) | slot j Y U V ...

not from the C++ enumeration, and every plane section must equal the encoder's debug_buffer of that
plane. The SHA-256 of each CPU blob is the one the commit before the enumeration wrote
(tests/golden/state_blobs.json, recorded there twice with equal results; no byte range is left
out of the hash). Export -> import into a fresh encoder -> export gives the same bytes (the parent did too).
GPU variants: the HIP blob against the HIP debug_buffer planes, and a host export continued on the CPU.
"""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from selkies_gstreamer_amd.ops.native import RC_FIELDS, H264Encoder
from tests.test_session_migration import KW, H, W, _frames, _run

GOLDEN = json.loads((Path(__file__).parent / "golden" / "state_blobs.json").read_text())
CASES = {
    "h264_stripes": dict(KW),
    "h264_fullframe": dict(KW, fullframe=True),
    "h264_refs2": dict(KW, num_refs=2),
    "h264_ltr2": dict(KW, ltr_slots=2),
    "hevc": dict(codec="hevc", fullframe=True, qp=27),
    "av1": dict(codec="av1", fullframe=True, qp=27),
}
GPU_CASES = ["h264_stripes", "h264_ltr2", "hevc", "av1"]
MB_W, MB_H = (W + 15) // 16, (H + 15) // 16
NY, NC = MB_W * 16 * MB_H * 16, MB_W * 8 * MB_H * 8


def _sections(blob):
    """{debug_buffer name: (offset, bytes)} of the plane sections, and the blob's total size."""
    hdr = blob[:64].view(np.int32)
    version, ns, slots = int(hdr[1]), int(hdr[6]), int(hdr[11])
    off = 64 + 44 * (ns + 1) + 4 * len(RC_FIELDS)
    out = {}
    for name in ("ref", "ref1", "src"):
        for p, n in zip("yuv", (NY, NC, NC)):
            out[f"{name}_{p}"] = (off, n)
            off += n
    off += 2 * 2 * MB_W * MB_H
    assert (version, slots > 0) in ((3, False), (4, True))
    if slots:
        off += 96 * (ns + 1)
        for j in range(slots):
            out[f"ltr{j}_y"] = (off, NY)
            off += NY + 2 * NC
    return out, off


def _session(case, backend):
    enc = H264Encoder(W, H, backend=backend, **CASES[case])
    _run(enc, _frames()[:4], 0)
    return enc


def _check_planes(enc, blob, case):
    sec, total = _sections(blob)
    assert len(blob) == enc.state_bytes() == total
    names = ["ref_y", "ref_u", "ref_v", "src_y", "src_u", "src_v"]
    if case.startswith("h264"):
        names.append("ref1_y")
    if case == "h264_ltr2":
        names += ["ltr0_y", "ltr1_y"]
    for name in names:
        o, n = sec[name]
        assert np.array_equal(blob[o:o + n], enc.debug_buffer(name)), name


@pytest.mark.parametrize("case", list(CASES))
def test_cpu_blob_sections_hash_and_round_trip(case):
    a = _session(case, "cpu")
    blob = a.export_state()
    _check_planes(a, blob, case)
    digest = hashlib.sha256(blob.tobytes()).hexdigest()
    print(case, len(blob), digest)
    assert digest == GOLDEN[case]
    b = H264Encoder(W, H, backend="cpu", **CASES[case])
    b.import_state(blob)
    assert np.array_equal(b.export_state(), blob)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES)
def test_hip_blob_sections_and_continuation_on_cpu(case):
    a = _session(case, "hip")
    blob = a.export_state()
    _check_planes(a, blob, case)
    c = H264Encoder(W, H, backend="cpu", **CASES[case])
    c.import_state(blob)
    fr = _frames()
    ra, rc = _run(a, fr[4:], 4), _run(c, fr[4:], 4)
    assert ra == rc
    assert not any(key for frame in rc for _, key, _ in frame)
