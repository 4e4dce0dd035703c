"""Inputs, encoder runs and snapshots for tests/test_codec_extremes.py: content that drives the
quantisers to their rails (QP 0 / 51), the smallest pictures the front end accepts and CBR pinned
at either end of the QP range. A run is one short sequence through one encoder; the CPU back end's
result of every run is computed once (`reference`) and shared by the CPU and the GPU tests."""
from __future__ import annotations

import functools
import io
import re
from pathlib import Path

import numpy as np

from selkies_gstreamer_amd.ops.native import (Av1Encoder, H264Encoder, HevcEncoder, JpegEncoder, TASK_DTYPE,
                                              hip_device_count)

CSRC = Path(__file__).resolve().parents[1] / "csrc"
CUINFO = 40    # sizeof(hevc::CuInfo); byte 0 is the mode, CU_SKIP = 0
CU_SKIP = 0
BLK = 12       # sizeof(av1::BlkInfo); byte 10 is the luma palette size (0: none)
H264_STATE = ("src_y", "src_u", "src_v", "tasks", "mbs", "me", "ref_y", "ref_u", "ref_v")


def _constant(header, name):
    """`constexpr int <name> = <value>;` of a header under csrc/: the tests follow the code's caps."""
    m = re.search(rf"constexpr int {name} = (\d+);", (CSRC / header).read_text())
    assert m, f"{name} not found in {header}"
    return int(m.group(1))


K_CU_BIN_CAP = _constant("codec/hevc_core.h", "kCuBinCap")
K_SUBSTREAM_CTB_BYTES = _constant("codec/hevc_core.h", "kSubstreamCtbBytes")
K_TOK_CAP = _constant("kernels/av1_gpu.h", "kTokCap")


# ---- content -------------------------------------------------------------------------------------
def _grey(v):
    """(H, W) uint8 -> BGRx with B = G = R = x."""
    return np.ascontiguousarray(np.repeat(v[..., None], 4, axis=2))


def noise(W, H, n, seed=1):
    """Uniform random bytes in all four channels, new every frame."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(n)]


def binary(W, H, n, seed=2):
    """Every pixel 0 or 255 (B = G = R), new every frame: two levels at one-pixel granularity."""
    rng = np.random.default_rng(seed)
    return [_grey(rng.integers(0, 2, (H, W), dtype=np.uint8) * 255) for _ in range(n)]


def checker(W, H, n, seed=0):
    """One-pixel checkerboard rolled one pixel per frame: frame t + 2 is frame t, and every inter
    frame has an exact match one pixel away."""
    yy, xx = np.mgrid[0:H, 0:W]
    base = (((xx + yy) & 1) * 255).astype(np.uint8)
    return [_grey(np.roll(base, t, axis=1)) for t in range(n)]


def flat_steps(W, H, n, seed=0):
    """Whole-frame constants 0, 255, 128, ...: one DC level per block is the only residual."""
    return [np.full((H, W, 4), (0, 255, 128)[t % 3], np.uint8) for t in range(n)]


def primaries(W, H, n, seed=3):
    """8 x 8 tiles of saturated colours (each of B, G, R 0 or 255), new every frame: chroma at its
    clipping limits."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        t = rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8, 4), dtype=np.uint8) * 255
        out.append(np.ascontiguousarray(np.kron(t, np.ones((8, 8, 1), np.uint8))[:H, :W]))
    return out


CONTENT = dict(noise=noise, binary=binary, checker=checker, flat_steps=flat_steps, primaries=primaries)


# ---- runs ----------------------------------------------------------------------------------------
def run(codec, W, H, content, frames=3, **kw):
    """A hashable run: codec, picture size, content generator name, frame count, encoder options."""
    return (codec, W, H, content, frames, tuple(sorted(kw.items())))


def rail(codec, W, H, content, qp):
    """Constant QP on a rail: no paint-over, HEVC under rate_control 'cqp'."""
    kw = dict(qp=qp, paint_qp=qp, use_paint_over=False)
    if codec == "hevc":
        kw["rate_control"] = "cqp"
    return run(codec, W, H, content, **kw)


def cbr(codec, kbps):
    return run(codec, 128, 64, "noise", frames=16, rate_control="cbr", bitrate_kbps=kbps, use_paint_over=False)


def frames_of(r):
    _, W, H, content, n, _ = r
    return CONTENT[content](W, H, n)


def encoder(r, backend):
    codec, W, H, _, _, kw = r
    cls = dict(hevc=HevcEncoder, av1=Av1Encoder, h264=H264Encoder, jpeg=JpegEncoder)[codec]
    return cls(W, H, backend=backend, **dict(kw))


def need_gpu():
    import pytest
    if hip_device_count() < 1:
        pytest.skip("no HIP device")


def _planes(enc, W, H):
    """The reconstruction cropped to the picture: Y, U, V (chroma (W + 1) / 2 x (H + 1) / 2)."""
    sy = (W + 15) // 16 * 16
    cw, ch = (W + 1) // 2, (H + 1) // 2
    return (enc.debug_buffer("ref_y").reshape(-1, sy)[:H, :W].copy(),
            enc.debug_buffer("ref_u").reshape(-1, sy // 2)[:ch, :cw].copy(),
            enc.debug_buffer("ref_v").reshape(-1, sy // 2)[:ch, :cw].copy())


def snapshot(enc, r, packets):
    """What the tests compare of one coded frame (every value a copy)."""
    codec, W, H = r[:3]
    s = dict(packets=[(p.y, p.h, bool(p.key), p.data) for p in packets])
    if codec == "jpeg":
        return s
    s["planes"] = _planes(enc, W, H)
    s["tasks"] = enc.debug_buffer("tasks", TASK_DTYPE).copy()
    if codec == "hevc":
        s["cus"] = enc.debug_buffer("cus").reshape(-1, CUINFO).copy()
        s["coefs"] = enc.debug_buffer("coefs", np.int16).copy()
        s["bin_n"] = enc.debug_buffer("bin_n", np.int32).copy()
    elif codec == "av1":
        s["blk"] = enc.debug_buffer("blk").reshape(-1, BLK).copy()
        s["levels"] = enc.debug_buffer("levels", np.int16).copy()
        s["av1_qidx"] = int(enc.debug_buffer("av1_qidx", np.int32)[0])
        s["src_y"] = enc.debug_buffer("src_y").reshape(-1, (W + 15) // 16 * 16)[:H, :W].copy()
    else:   # H.264: the buffers tests/test_h264_gpu.py _compare_state reads
        s["state"] = {n: enc.debug_buffer(n).copy() for n in H264_STATE}
    return s


class Recorded:
    """A snapshot's H.264 buffers behind the encoder's debug_buffer interface, so that a finished
    CPU run can stand in for the live encoder in _compare_state."""

    def __init__(self, snap):
        self.state = snap["state"]

    def debug_buffer(self, name, dtype=np.uint8):
        return self.state[name].view(dtype)


@functools.lru_cache(maxsize=None)
def reference(r):
    """(frames, per-frame snapshots of the CPU back end, its rc_stats after the run), once per run."""
    frames = frames_of(r)
    cpu = encoder(r, "cpu")
    snaps = [snapshot(cpu, r, cpu.encode(f, t)) for t, f in enumerate(frames)]
    stats = cpu.rc_stats() if r[0] != "jpeg" else {}
    cpu.close()
    for s in snaps:   # shared between tests: nobody writes to it
        for v in s.values():
            for a in (v if isinstance(v, tuple) else v.values() if isinstance(v, dict) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
    return frames, snaps, stats


# ---- independent decoders ------------------------------------------------------------------------
class Decoder:
    """The independent decoder of a run's codec; `decode(packets)` returns the planes it produced
    for one coded frame ((Y, U, V); JPEG: nothing, the stripes are checked one by one)."""

    def __init__(self, r):
        self.codec, self.W, self.H = r[:3]
        if self.codec == "hevc":
            from selkies_gstreamer_amd.models.hevc.decoder import HevcDecoder
            self.dec = HevcDecoder()
        elif self.codec == "av1":
            from selkies_gstreamer_amd.models.av1 import dav1d
            self.dec = dav1d.Decoder()
        elif self.codec == "h264":
            from tests.h264_util import StripeDecoder
            self.dec = StripeDecoder(self.W, self.H)

    def decode(self, packets):
        if self.codec == "hevc":
            (_, _, _, data), = packets
            pics = self.dec.decode(data[10:])
            assert len(pics) == 1, "one picture per packet"
            return tuple(pics[0])
        if self.codec == "av1":
            (_, _, _, data), = packets
            pic = self.dec.decode(data[10:])
            assert pic is not None, "dav1d produced no picture"
            return tuple(pic)
        if self.codec == "h264":
            for _, _, _, data in packets:
                self.dec.feed(data)
            return self.dec.Y, self.dec.U, self.dec.V
        from PIL import Image
        for y, h, _, data in packets:   # libjpeg decodes every stripe to the end
            img = Image.open(io.BytesIO(data[4:]))
            img.load()
            assert img.size == (self.W, h), f"stripe y={y}: decoded {img.size}"
        return None


def assert_decodes(r, snaps, who):
    """The independent decoder, fed the packets of `snaps`, returns their reconstruction, all three
    planes (JPEG: every stripe decodes to the end at its size)."""
    dec = Decoder(r)
    for t, s in enumerate(snaps):
        got = dec.decode(s["packets"])
        if got is None:
            continue
        for name, a, b in zip("YUV", got, s["planes"]):
            assert a.shape == b.shape, f"{who} frame {t} plane {name}: decoder {a.shape}, encoder {b.shape}"
            bad = np.argwhere(a != b)
            assert len(bad) == 0, f"{who} frame {t} plane {name}: {len(bad)} samples differ, first {bad[:3].tolist()}"


def assert_same(r, t, got, ref):
    """The HIP back end's frame `t` against the CPU reference's: exact equality of everything."""
    codec = r[0]
    names = dict(hevc=("cus", "coefs", "bin_n"), av1=("blk", "levels", "av1_qidx"), h264=(), jpeg=())[codec]
    if codec != "jpeg":
        assert np.array_equal(got["tasks"]["final_action"], ref["tasks"]["final_action"]), f"frame {t}: slice decisions differ"
        assert np.array_equal(got["tasks"]["qp"], ref["tasks"]["qp"]), \
            f"frame {t}: slice QPs differ: {got['tasks']['qp'].tolist()} != {ref['tasks']['qp'].tolist()}"
    for n in names:
        a, b = np.asarray(got[n]), np.asarray(ref[n])
        assert a.shape == b.shape, f"frame {t}: {n} has shape {a.shape}, the reference {b.shape}"
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"frame {t}: {n} differs in {len(bad)} places, first {bad[:3].tolist()}"
    for name, a, b in zip("YUV", got.get("planes", ()), ref.get("planes", ())):
        bad = np.argwhere(a != b)
        assert len(bad) == 0, f"frame {t}: reconstruction {name} differs in {len(bad)} samples, first {bad[:3].tolist()}"
    assert [p[:3] for p in got["packets"]] == [p[:3] for p in ref["packets"]], f"frame {t}: packet layout differs"
    for (y, _, _, a), (_, _, _, b) in zip(got["packets"], ref["packets"]):
        if a != b:
            first = next((i for i, (x, z) in enumerate(zip(a, b)) if x != z), min(len(a), len(b)))
            raise AssertionError(f"frame {t} packet y={y}: {len(a)} bytes against {len(b)}, first difference at byte {first}")
