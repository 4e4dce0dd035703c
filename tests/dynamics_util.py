"""One driver for tests/test_session_dynamics.py: a scripted session through any codec, either back
end and any pacing of upload / launch / finish.

A run is a hashable tuple (codec, W, H, frame spec, encoder options, script) in the style of
tests/extremes_util.run. The frames come from ltr_util.sequence(spec); the script is a tuple of
(t, event, args), each applied immediately before frame t is handed to the encoder:

  key ()                        request_keyframe()
  qp (qp,)                      set_qp(qp)
  rate (mode, kbps)             set_rate(mode, kbps)
  overlay_image (slot, seed, h, w)   set_overlay(slot, premultiplied random image); seed None clears it
  overlay_pos (slot, x, y, on)  set_overlay_pos
  input (kind,)                 the frames from t on arrive as 'bgrx', 'i420', 'nv12' or 'bgrx_padded'
                                (rows W * 4 + PAD bytes apart, the padding filled with noise)
  rows ()                       set_upload_rows with the real difference to the frame uploaded before
  replaced ()                   HIP only: another picture is uploaded under frame t's id and then
                                replaced by frame t before launch (the CPU back end codes on upload,
                                so its run is the run of the launched frames)
  handover ()                   frame t - 1 is left in flight, export_state(), finish(t - 1); fresh
                                encoders (`heirs`) import the blob and code the frames from t on

Pacings: 'serial' encode(); 'overlapped' upload(n + 1), finish(n), launch(n + 1); 'two' upload(n + 1),
launch(n + 1), finish(n). encode_yuv is synchronous, so the frame in flight is collected before a
planar frame. Frame ids start at FIRST_ID, so the 16-bit id wraps in mid-run, and every packet
collected for frame t must carry (FIRST_ID + t) & 0xFFFF in bytes 2..4: a finish() that returns the
other parity's packets fails right there."""
from __future__ import annotations

import collections
import functools

import numpy as np

from selkies_gstreamer_amd.ops.native import Av1Encoder, H264Encoder, HevcEncoder, convert_bgrx
from tests import extremes_util as xu
from tests import ltr_util

FIRST_ID = 65533
PAD = 96
PACINGS = ("serial", "overlapped", "two")
EVENTS = ("key", "qp", "rate", "overlay_image", "overlay_pos", "input", "rows", "replaced", "handover")


def run(codec, W, H, spec, script=(), **kw):
    """A hashable run: codec, picture size, ltr_util.sequence spec, encoder options, script."""
    script = tuple(sorted((t, ev, tuple(args)) for t, ev, args in script))
    assert all(ev in EVENTS for _, ev, _ in script), script
    return (codec, W, H, spec, tuple(sorted(kw.items())), script)


def without(r, event):
    """The run `r` with every `event` taken out of its script."""
    return r[:5] + (tuple(e for e in r[5] if e[1] != event),)


@functools.lru_cache(maxsize=None)
def frames_of(spec, W, H):
    out = [f for _, _, f in ltr_util.sequence(spec, W, H)]
    for f in out:   # shared between runs: nobody writes to it
        f.setflags(write=False)
    return out


def encoder(r, backend):
    cls = dict(h264=H264Encoder, hevc=HevcEncoder, av1=Av1Encoder)[r[0]]
    return cls(r[1], r[2], backend=backend, **dict(r[4]))


def overlay_image(seed, h, w):
    """Premultiplied BGRA noise with a fifth of the pixels fully transparent."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((h, w)) < 0.2, 0, img[..., 3])
    img[..., :3] = (img[..., :3].astype(np.uint32) * img[..., 3:4] // 255).astype(np.uint8)
    return img


def changed_rows(a, b):
    """Row ranges [(y, y + 1), ...] in which the BGRx frames differ (test_h264_gpu._changed_rows)."""
    rows = np.nonzero((a != b).any(axis=(1, 2)))[0]
    return [(int(y), int(y) + 1) for y in rows]


def padded(f, seed):
    """`f` as (H, W * 4 + PAD) rows; the padding is noise no encoder may read."""
    H, W = f.shape[:2]
    buf = np.random.default_rng(seed).integers(0, 256, (H, W * 4 + PAD), dtype=np.uint8)
    buf[:, :W * 4] = f.reshape(H, W * 4)
    return buf


def decoy(f):
    """The picture that is uploaded and then replaced: `f` with one band of rows changed."""
    d = f.copy()
    d[40:56, :, :3] ^= 0x3C
    return d


def check_frame_id(packets, t):
    """Every packet handed out for frame t carries that frame's id in bytes 2..4."""
    fid = (FIRST_ID + t) & 0xFFFF
    for p in packets:
        got = int.from_bytes(p.data[2:4], "big")
        assert got == fid, f"frame {t}: collected a packet (y={p.y}) of frame id {got}, expected {fid}"


def _pk(packets, t):
    """(y, h, key, data) of the packets collected for frame t, each carrying that frame's id."""
    check_frame_id(packets, t)
    return [(p.y, p.h, bool(p.key), p.data) for p in packets]


def apply_event(enc, st, ev, args):
    """One script event on one encoder; `st` is the driver's state of that session."""
    if ev == "key":
        enc.request_keyframe()
    elif ev == "qp":
        enc.set_qp(*args)
    elif ev == "rate":
        enc.set_rate(*args)
    elif ev == "overlay_image":
        slot, seed, h, w = args
        enc.set_overlay(slot, None if seed is None else overlay_image(seed, h, w))
    elif ev == "overlay_pos":
        slot, x, y, on = args
        enc.set_overlay_pos(slot, x, y, enabled=bool(on))
    elif ev == "input":
        st["kind"], = args
    elif ev in ("rows", "replaced"):
        st[ev] = True


class Session:
    """One encoder being driven through frames lo..hi of a run."""

    def __init__(self, r, backend, pacing, st=None, want_snaps=False):
        self.r, self.backend, self.pacing = r, backend, pacing
        self.enc = encoder(r, backend)
        self.st = dict(kind="bgrx", prev=None) if st is None else dict(st)
        self.pending = collections.deque()   # frames launched and not collected
        self.want_snaps = want_snaps
        self.packets, self.snaps, self.rows = {}, {}, {}

    def _done(self, t, packets):
        self.packets[t] = _pk(packets, t)
        if self.want_snaps:
            s = xu.snapshot(self.enc, self.r, packets)
            s["rc"] = self.enc.rc_stats()   # per frame: set_rate() to another mode starts the statistics again
            if dict(self.r[4]).get("ltr_slots"):
                s["ltr_slot"] = ltr_util.ltr_slots_of_tasks(self.enc)
            self.snaps[t] = s

    def collect(self):
        t = self.pending.popleft()
        self._done(t, self.enc.finish())

    def drain(self):
        while self.pending:
            self.collect()

    def _announce(self, t, f):
        """rows event: the damage of the coming upload against the picture uploaded before it."""
        if not self.st.get("rows"):
            return
        rows = None if self.st["prev"] is None else changed_rows(self.st["prev"], f)
        self.enc.set_upload_rows(rows)
        self.rows[t] = rows

    def hand_over(self, t, f, hold=False):
        """Frame t into the encoder in this session's pacing; hold: leave it in flight."""
        enc, st, fid = self.enc, self.st, FIRST_ID + t
        if st["kind"] in ("i420", "nv12"):
            assert not hold
            self.drain()
            st["prev"] = None   # the BGRx buffers no longer hold the last frames
            self._done(t, enc.encode_yuv(st["kind"], *convert_bgrx(f, st["kind"]), frame_id=fid))
            return
        if st.pop("replaced", False) and self.backend == "hip":
            d = decoy(f)
            self._announce(t, d)
            enc.upload(d, fid)
            st["prev"] = d
        self._announce(t, f)
        st.pop("rows", None)
        st["prev"] = f
        a = padded(f, t) if st["kind"] == "bgrx_padded" else f
        if self.pacing == "serial" and not hold:
            self._done(t, enc.encode(a, fid))
        elif self.pacing == "two":
            enc.upload(a, fid)
            enc.launch()
            self.pending.append(t)
            while len(self.pending) > 1:
                self.collect()
        else:   # overlapped (and a held frame of the serial pacing)
            enc.upload(a, fid)
            self.drain()
            enc.launch()
            self.pending.append(t)

    def close(self, res):
        self.drain()
        res["planes"] = xu._planes(self.enc, self.r[1], self.r[2])
        res["stats"] = self.enc.rc_stats()
        self.enc.close()


def _in_order(d, lo, hi):
    assert sorted(d) == list(range(lo, hi)), f"frames collected: {sorted(d)}, expected {lo}..{hi - 1}"
    return [d[t] for t in range(lo, hi)]


def drive(r, backend, pacing, heirs=None, want_snaps=None):
    """The run `r` on `backend` in `pacing`. Returns a dict: `packets` per frame [(y, h, key, data)],
    `planes` (the reference picture after the last finish) and `stats` (rc_stats), `rows` (what the
    rows events announced), under the serial pacing also `snaps` (extremes_util.snapshot per frame,
    plus `ltr_slot` with the cache on). With a handover in the script: `packets` are the donor's up to
    the frame in flight at the export, and `heirs[b]` is the same dict for the fresh encoder on back
    end b of `heirs` (default: the donor's), whose `packets` start at the handover frame."""
    assert pacing in PACINGS
    codec, W, H, spec, _, script = r
    frames = frames_of(spec, W, H)
    n = len(frames)
    events = collections.defaultdict(list)
    for t, ev, args in script:
        assert 0 <= t < n
        events[t].append((ev, args))
    cut = [t for t, ev, _ in script if ev == "handover"]
    assert len(cut) <= 1 and all(t > 0 for t in cut)
    cut = cut[0] if cut else n
    snaps = pacing == "serial" if want_snaps is None else want_snaps

    def segment(s, lo, hi, hold_last):
        for t in range(lo, hi):
            for ev, args in events[t]:
                apply_event(s.enc, s.st, ev, args)
            s.hand_over(t, frames[t], hold=hold_last and t == hi - 1)

    def result(s, lo, hi):
        res = {}
        s.close(res)
        res["packets"] = _in_order(s.packets, lo, hi)
        res["rows"] = s.rows
        if snaps:
            res["snaps"] = _in_order(s.snaps, lo, hi)
        return res

    donor = Session(r, backend, pacing, want_snaps=snaps)
    segment(donor, 0, cut, cut < n)
    if cut == n:
        return result(donor, 0, n)
    assert list(donor.pending) == [cut - 1], "the handover needs frame t - 1 in flight"
    blob = donor.enc.export_state()
    donor.collect()
    res = result(donor, 0, cut)
    res["heirs"] = {}
    for b in heirs or (backend,):
        heir = Session(r, b, pacing, st=donor.st, want_snaps=snaps)
        heir.enc.import_state(blob)
        segment(heir, cut, n, False)
        res["heirs"][b] = result(heir, cut, n)
    return res


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)


@functools.lru_cache(maxsize=None)
def reference(r):
    """The CPU back end's serial run of `r`, once per run; shared, so nobody writes to it."""
    res = drive(r, "cpu", "serial")
    _freeze(res)
    return res


def drive_many(runs, backend):
    """Several sessions from one thread: per frame upload + launch on each, then finish on each.
    Returns the packets per frame of every session."""
    ss = [Session(r, backend, "two") for r in runs]
    n = len(frames_of(runs[0][3], runs[0][1], runs[0][2]))
    for t in range(n):
        for s in ss:
            codec, W, H, spec, _, script = s.r
            for tt, ev, args in script:
                if tt == t:
                    apply_event(s.enc, s.st, ev, args)
            s.hand_over(t, frames_of(spec, W, H)[t], hold=True)
        for s in ss:
            s.drain()
    out = []
    for s in ss:
        s.enc.close()
        out.append(_in_order(s.packets, 0, n))
    return out


def assert_packets_equal(got, ref, who, t0=0):
    """Per frame: the same packets, (y, h, key) and every byte."""
    assert len(got) == len(ref), f"{who}: {len(got)} frames against {len(ref)}"
    for i, (g, c) in enumerate(zip(got, ref)):
        t = t0 + i
        assert [p[:3] for p in g] == [p[:3] for p in c], \
            f"{who} frame {t}: packet layout {[p[:3] for p in g]} against {[p[:3] for p in c]}"
        for (y, _, _, a), (_, _, _, b) in zip(g, c):
            if a != b:
                first = next((k for k, (x, z) in enumerate(zip(a, b)) if x != z), min(len(a), len(b)))
                raise AssertionError(f"{who} frame {t} packet y={y}: {len(a)} bytes against {len(b)}, "
                                     f"first difference at byte {first}")


def rc_state(stats):
    """rc_stats() without `seq`: that word is the HIP back end's count of set_rate() calls, by which
    k_rc_qp tells a new request apart (an imported state takes the importing encoder's); the CPU
    controller has no use for it and leaves it 0. Everything else is the controller's state."""
    return {k: v for k, v in stats.items() if k != "seq"}


def assert_end_state_equal(got, ref, who):
    """After the last finish(): the reference picture and the rate controller's state."""
    for name, a, b in zip("YUV", got["planes"], ref["planes"]):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"{who}: final reference plane {name} differs in {len(bad)} samples, first {bad[:3].tolist()}"
    assert rc_state(got["stats"]) == rc_state(ref["stats"]), f"{who}: rc_stats {got['stats']} against {ref['stats']}"
