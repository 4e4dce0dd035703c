"""The pairwise option matrix of tests/test_option_matrix.py: a deterministic generator of rows in
which every allowed pair of option values occurs, the three codecs' tables of axes, the scripted
session a row stands for, and readers that tell from the CPU reference whether an option acted.

A row is a dict {axis: value}. An axis whose name is that of an environment switch (SK_...) carries
the switch's value, None for unset; `paint` and `size` and `tiles` stand for several constructor
arguments (`options`). Everything else is a constructor argument by its own name. A case is
(run, env): the hashable run of tests/dynamics_util.py plus the sorted environment items, so that a
reference computed under one environment is never handed out under another.

The generator runs at import; no table is stored."""
from __future__ import annotations

import itertools
import random

import numpy as np

from selkies_gstreamer_amd.models.hevc.decoder import split_annexb
from selkies_gstreamer_amd.ops.native import MB_INFO_DTYPE, ME_DTYPE
from tests import av1_tools_util as T
from tests import dynamics_util as du

SEED = 1
SPEC = "A10 B3 A3 C2 B2"          # test_session_dynamics.LONG
PAINT_QP, PAINT_TRIGGER = 20, 3
SIZES = ((208, 112), (200, 120))

# Every value list is complete; the first value is the default.
AXES = {
    "h264": {
        "fullframe": (False, True),
        "num_refs": (1, 2),
        "ltr_slots": (0, 2),
        "intra4x4": (False, True),
        "aq_strength": (0.0, 1.0),
        "deblock": ("auto", True, False),
        "subpel": (True, False),
        "me_full": (True, False),
        "stripe_height": (32, 64),
        "paint": (False, True),
        "qp": (25, 38),
        "size": SIZES,
    },
    "hevc": {
        "ltr_slots": (0, 1, 2),
        "subpel": (True, False),
        "SK_HEVC_SEG_CTBS": (None, "3"),
        "stripe_height": (32, 64),
        "paint": (False, True),
        "qp": (25, 37),
        "size": SIZES,
    },
    "av1": {
        "intra_inter": (False, True),
        "chroma_palette": (False, True),
        "cfl": (False, True),
        "palette_cluster": (False, True),
        "ltr_slots": (0, 2, 7),
        "tiles": ((-1, -1), (1, 1), (2, 0)),
        "SK_AV1_PALETTE": (None, "0"),
        "qp": (25, 38),
        "size": SIZES,
    },
}


def allowed(codec, row):
    """The constraint predicate; `row` may be partial (an axis it does not hold constrains nothing).
    H.264: the constructor refuses the long-term cache together with a second reference."""
    if codec == "h264":
        return not (row.get("ltr_slots", 0) > 0 and row.get("num_refs", 1) == 2)
    return True


# ---- generator -----------------------------------------------------------------------------------
def _pairs_of(row, names):
    return {((a, row[a]), (b, row[b])) for a, b in itertools.combinations(names, 2)}


def allowed_pairs(axes, ok):
    """Every ((axis, value), (axis, value)) of two different axes that the predicate lets stand."""
    names = list(axes)
    return {((a, va), (b, vb)) for a, b in itertools.combinations(names, 2)
            for va in axes[a] for vb in axes[b] if ok({a: va, b: vb})}


def pairwise(axes, ok=lambda row: True, seed=SEED, tries=40):
    """Rows over `axes` ({name: values}) that satisfy `ok` and together hold every allowed pair of
    values of two axes. Greedy (AETG): each new row is the best of `tries` candidates; a candidate
    starts from the first pair still missing and takes, axis by axis in a shuffled order, the value
    that adds the most missing pairs and keeps the row allowed. Deterministic for a seed."""
    rng = random.Random(seed)
    names = list(axes)
    missing = allowed_pairs(axes, ok)
    order = sorted(missing, key=repr)
    rows = []
    while missing:
        first = next(p for p in order if p in missing)
        best, best_gain = None, -1
        for _ in range(tries):
            row = dict(first)
            rest = [n for n in names if n not in row]
            rng.shuffle(rest)
            for n in rest:
                scored = []
                for v in axes[n]:
                    cand = dict(row, **{n: v})
                    if ok(cand):
                        scored.append((sum(((a, cand[a]), (n, v)) in missing or ((n, v), (a, cand[a])) in missing
                                           for a in row), v))
                assert scored, f"no allowed value of {n} for {row}"
                top = max(g for g, _ in scored)
                row[n] = rng.choice([v for g, v in scored if g == top])
            gain = len(_pairs_of(row, names) & missing)
            if gain > best_gain:
                best, best_gain = row, gain
        assert best_gain > 0
        rows.append({n: best[n] for n in names})
        missing -= _pairs_of(best, names)
    return rows


# Rows written by hand. With SEED = 1 every option value acts in a generated row (the reach test), so
# none is here for that. The one H.264 row is the four-way combination that selects the most code
# at once on the HIP back end (I_NxN macroblocks, per-MB QPs into k_code_inter and k_cavlc, the second
# reference, deblocking below QP 34); pairs alone put no more than three of the four into one row.
_DEFAULTS = {c: {n: v[0] for n, v in AXES[c].items()} for c in AXES}
EXTRA = {"h264": [dict(_DEFAULTS["h264"], intra4x4=True, aq_strength=1.0, num_refs=2, deblock=True)],
         "hevc": [], "av1": []}
ROWS = {c: pairwise(AXES[c], lambda row, c=c: allowed(c, row)) + EXTRA[c] for c in AXES}


def row_id(codec, k, row):
    short = []
    for n, v in row.items():
        if v == AXES[codec][n][0]:
            continue
        n = n.replace("SK_HEVC_", "").replace("SK_AV1_", "").lower()
        short.append(n if v is True else f"{n}{'x'.join(map(str, v)) if isinstance(v, tuple) else v}")
    return f"{codec}{k:02d}-" + ("-".join(short) or "defaults")


# ---- a row's session -----------------------------------------------------------------------------
def options(codec, row):
    """(W, H, constructor options, environment) of a row."""
    kw, env = dict(use_paint_over=False), {}
    if codec == "av1":
        kw["stripe_height"] = 32
    W, H = row["size"]
    for n, v in row.items():
        if n == "size":
            continue
        if n.startswith("SK_"):
            if v is not None:
                env[n] = v
        elif n == "paint":
            if v:
                kw.update(use_paint_over=True, paint_over_trigger=PAINT_TRIGGER, paint_qp=PAINT_QP)
        elif n == "tiles":
            kw.update(tile_cols_log2=v[0], tile_rows_log2=v[1])
        else:
            kw[n] = v
    return W, H, kw, env


def case(codec, row, script):
    W, H, kw, env = options(codec, row)
    return du.run(codec, W, H, SPEC, script, **kw), tuple(sorted(env.items()))


ENV_NAMES = tuple(n for axes in AXES.values() for n in axes if n.startswith("SK_"))
_REFERENCES = {}


def set_env(monkeypatch, env):
    """The case's environment, and none of the other switches, before an encoder is made."""
    for n in ENV_NAMES:
        monkeypatch.delenv(n, raising=False)
    for n, v in env:
        monkeypatch.setenv(n, v)


def reference(monkeypatch, c):
    """The CPU back end's serial run of case `c` under its environment, once per case (dynamics_util's
    own cache knows the run alone, so it is not used here)."""
    set_env(monkeypatch, c[1])
    if c not in _REFERENCES:
        res = du.drive(c[0], "cpu", "serial")
        du._freeze(res)
        _REFERENCES[c] = res
    return _REFERENCES[c]


# ---- reach: what the CPU reference shows of an option --------------------------------------------
def _coded(snap):
    return snap["tasks"][snap["tasks"]["final_action"] != 0]


def _slices(snap, W, actions):
    """(task, slice of macroblock indices) of the slices of a frame with a final action in `actions`."""
    mb_w = (W + 15) // 16
    return [(t, slice(t["first_row"] * mb_w, (t["first_row"] + t["num_rows"]) * mb_w))
            for t in snap["tasks"] if t["final_action"] in actions]


def av1_tile_log2(tu, W, H):
    """(tile_cols_log2, tile_rows_log2) read from the uncompressed header of a key frame's OBU_FRAME
    (AV1 5.9.2, 5.9.15 with uniform_tile_spacing_flag; 64x64 superblocks, the picture below the
    tile size limits, so both minima are 0): show_existing_frame, frame_type (2), show_frame,
    disable_cdf_update, allow_screen_content_tools, frame_size_override_flag,
    render_and_frame_size_different, allow_intrabc if screen content tools are on,
    disable_frame_end_update_cdf, uniform_tile_spacing_flag, then the increment bits."""
    sb_cols, sb_rows = (W + 63) // 64, (H + 63) // 64
    max_cols, max_rows = (sb_cols - 1).bit_length(), (sb_rows - 1).bit_length()
    i = 0
    while i < len(tu):
        typ = (tu[i] >> 3) & 15
        assert tu[i] & 2, "obu_has_size_field"
        n, i = 0, i + 1
        for s in range(0, 56, 7):
            n |= (tu[i] & 0x7f) << s
            i += 1
            if not tu[i - 1] & 0x80:
                break
        if typ == 6:
            bits = "".join(f"{b:08b}" for b in tu[i:i + 4])
            assert bits[:4] == "0001", "a shown key frame"
            pos = 4 + 1
            screen = bits[pos] == "1"
            pos += 3 + (1 if screen else 0)
            assert bits[pos:pos + 2] == "11", "disable_frame_end_update_cdf, uniform_tile_spacing_flag"
            pos += 2
            cols = rows = 0
            while cols < max_cols and bits[pos] == "1":
                cols, pos = cols + 1, pos + 1
            pos += cols < max_cols
            while rows < max_rows and bits[pos] == "1":
                rows, pos = rows + 1, pos + 1
            return cols, rows
        i += n
    raise AssertionError("no OBU_FRAME")


def hevc_slice_nals(data):
    """The number of slice segment NAL units (types 0..21) of a packet."""
    return sum(((n[0] >> 1) & 63) <= 21 for n in split_annexb(data[10:]))


SWITCH_BACK = 13   # the first frame of "A3"
CBR_AT = 8         # set_rate("cbr") of the control script
CBR_LAST = 11      # the last frame of the CBR stretch: set_rate() to another mode starts the statistics again


def reached(codec, row, ref, plain=None):
    """{feature: acted} of one row's CPU reference `ref`; `plain`: for an H.264 row with deblock=True,
    the reference of the same row with deblock "auto". A feature is listed only in the rows that
    carry its option value (`redos`: every row)."""
    snaps = ref["snaps"]
    W, H = row["size"]
    out = {"redos": snaps[CBR_LAST]["rc"]["redos"] >= 1}
    if row.get("ltr_slots"):
        out[f"ltr_slots={row['ltr_slots']}"] = max(snaps[SWITCH_BACK]["ltr_slot"]) >= 0
    if row.get("paint"):   # a slice at the paint QP before the CBR stretch, where the frame QP is the row's or 36
        out["paint"] = any((_coded(s)["qp"] == PAINT_QP).any() for s in snaps[:CBR_AT])
    if codec == "h264":
        mbs = [s["state"]["mbs"].view(MB_INFO_DTYPE) for s in snaps]
        if row["intra4x4"]:
            out["intra4x4"] = any((m["type"][sl] == 3).any() for s, m in zip(snaps, mbs) for _, sl in _slices(s, W, (1, 2)))
        if row["num_refs"] == 2:
            # The second reference is the picture before the last one (a sliding window of two), so
            # the switch back to A after three frames of B cannot hit it; the caret can, which
            # returns to its state of two pictures ago in every frame. A coded macroblock of a P
            # slice that the search gave reference 1 and the slice kept:
            out["num_refs=2"] = any(((s["state"]["me"].view(ME_DTYPE)["ref"][sl] == 1) & (m["ref"][sl] == 1)).any()
                                    for s, m in zip(snaps, mbs) for _, sl in _slices(s, W, (1,)))
        if row["aq_strength"]:
            out["aq_strength"] = any(len(np.unique(m["qp"][sl])) > 1 for s, m in zip(snaps, mbs)
                                     for _, sl in _slices(s, W, (1, 2)))
        if row["deblock"] is True:   # filtered where "auto" does not filter: another picture below QP 34
            out["deblock=True"] = any(len(_coded(s)) and _coded(s)["qp"].max() < 34 and
                                      any((a != b).any() for a, b in zip(s["planes"], p["planes"]))
                                      for s, p in zip(snaps, plain["snaps"]))
    if codec == "hevc" and row["SK_HEVC_SEG_CTBS"]:
        key = snaps[0]["packets"]
        out["SEG_CTBS"] = sum(hevc_slice_nals(p[3]) for p in key) > (H + 31) // 32
    if codec == "av1":
        cells = [s["blk"].reshape((H + 7) // 8, (W + 7) // 8, 12) for s in snaps]
        took = [T.took(s["src_y"], c, bool(s["packets"][0][2])) for s, c in zip(snaps, cells)]
        for name in ("intra_inter", "chroma_palette", "cfl", "palette_cluster"):
            # a session without luma palettes has neither of the tools that build on them (session_tools)
            if row[name] and not (row["SK_AV1_PALETTE"] == "0" and name in ("chroma_palette", "palette_cluster")):
                out[name] = any(f[name] for f in took)
        if row["tiles"] != (-1, -1):
            c, r = av1_tile_log2(snaps[0]["packets"][0][3][10:], W, H)
            out[f"tiles={row['tiles']}"] = (c, r) == row["tiles"] and c + r > 0
        if row["SK_AV1_PALETTE"] == "0":   # no palette anywhere (BlkInfo byte 10: luma size, chroma size << 4)
            out["PALETTE=0"] = not any(c[..., 10].any() for c in cells)
    return out
