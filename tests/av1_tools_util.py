"""Shared helpers of the AV1 tools tests (test_av1_tools.py, test_av1_tools_gpu.py) and of
tools/av1_tools_fixture.py: one small sequence on which every screen-content tool of the AV1 encoder
has candidates, the 16 combinations of the tools, and the digests of what a session produces.

Content: three regions side by side, cut at unit boundaries so that no 16x16 unit mixes two of them:
aa_field (av1_palette_cluster_util: anti-aliased glyphs, clustered luma palettes), glyph_field with the
iso-luma ink of av1_cfl_util (chroma palettes that CfL cannot replace) and the hue texture of
av1_cfl_util (CfL). Frames 1 and 2 move the glyph rows by the helpers' `shift` and take another
texture, so the inter frames of a session with intra_inter hold candidates of every tool too.

72x72: the last column and row of blocks are 8x8."""
from __future__ import annotations

import hashlib

import numpy as np

from selkies_gstreamer_amd.ops.native import Av1Encoder
from tests import av1_cfl_util as K
from tests import av1_chroma_palette_util as C
from tests import av1_palette_cluster_util as P
from tests.ltr_util import ref_planes

W = H = 72
QP = 20
CUTS = (32, 48)     # aa_field in [0, 32), glyph_field in [32, 48), hue texture in [48, w)
TOOLS = ("chroma_palette", "cfl", "palette_cluster")     # bit k of a case's mask (the kernels' tools word)
CASES = [(mask, ii) for ii in (False, True) for mask in range(8)]


def case_id(mask: int, ii: bool) -> str:
    return f"mask{mask}_ii{int(ii)}"


def case_kwargs(mask: int, ii: bool) -> dict:
    kw = {name: bool(mask >> k & 1) for k, name in enumerate(TOOLS)}
    kw["intra_inter"] = ii
    return kw


def picture(w: int, h: int, k: int, cuts=CUTS) -> np.ndarray:
    """Frame k of the sequence (BGRx)."""
    f = P.aa_field(w, h, 3 * k)
    f[:, cuts[0]:cuts[1]] = C.glyph_field(w, h, 3 * k, ink=K.ISO_INK)[:, cuts[0]:cuts[1]]
    f[:, cuts[1]:] = K.hue_texture(w, h, k)[:, cuts[1]:]
    return f


def frames(w: int = W, h: int = H, cuts=CUTS) -> list:
    return [picture(w, h, k, cuts) for k in range(3)]


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(enc, w: int, h: int, packets) -> dict:
    """Digests of the frame just coded: the temporal unit (the packet without its 10-byte stripe
    header) and the three reconstruction planes."""
    assert len(packets) == 1
    return {"tu": sha(np.frombuffer(bytes(packets[0].data[10:]), np.uint8)),
            "rec": [sha(p) for p in ref_planes(enc, w, h)]}


def took(src_y: np.ndarray, cells: np.ndarray, key: bool) -> dict:
    """Whether a block of the frame took each tool (read from the cells), and whether an inter frame
    holds an intra cell."""
    intra = ((cells[..., K.BLK_FLAGS] & 1) == 0) & (cells[..., 0] > 0)
    return {"chroma_palette": bool((intra & ((cells[..., C.BLK_PAL_N] >> 4) > 0)).any()),
            "cfl": bool(K.is_cfl(cells)[intra].any()),
            "palette_cluster": bool((intra & P.clustered(src_y, cells)).any()),
            "intra_inter": bool(not key and intra.any())}


def run_cpu(mask: int, ii: bool, w: int = W, h: int = H, seq=None, **kw) -> list:
    """The CPU encoder over the sequence: per frame the digests and what the frame's blocks took."""
    enc = Av1Encoder(w, h, backend="cpu", qp=QP, **case_kwargs(mask, ii), **kw)
    out = []
    for t, f in enumerate(seq if seq is not None else frames(w, h)):
        pk = enc.encode(f, t)
        d = digest(enc, w, h, pk)
        d["took"] = took(C.src_planes(enc, w, h)[0], C.cells(enc, w, h), bool(pk[0].key))
        out.append(d)
    enc.close()
    return out
