#!/usr/bin/env python3
"""Headline benchmark: encoded 1920x1080 H.264 frames per second on MI355X.

Metric (BASELINE.json): "encoded fps + glass-to-glass p50 ms at 1920x1080;
concurrent 60fps sessions/node". The reference's headline is ">= 60 fps at
1920x1080" for one session (README.md:7, docs/design.md:11).

One step = every session on every GPU encodes one captured 1920x1080 BGRx frame
through the full pipeline: pinned host frame -> H2D -> colour conversion +
damage -> motion search -> transform/quant/recon -> CAVLC -> slice assembly with
emulation prevention -> packets on the host (0x04 stripe framing), i.e. exactly
what the capture module hands to the WebSocket server. Sessions are independent
desktop streams (session-parallel "dp"), each with its own HIP stream/thread.
With --gpus N the driver starts one rank per GPU (torchrun); ranks synchronise
over RCCL (torch.distributed "nccl") and optionally gather every rank's packets
to rank 0 over xGMI (--gather, the single-server fan-out topology).

`value` is the whole-job aggregate encoded fps; the JSON also reports the p50/p99
capture-to-packet encode latency (the server-side share of glass-to-glass) and
how many concurrent 60 fps sessions that throughput sustains.

A plain run sets up, warms up, times --steps steps and prints the result line.
Everything else the benchmark measures (the end-to-end session checks with real
servers and clients, the 4K / 8K HEVC and AV1 sessions, the CPU 480p session)
runs only with --full. --dump-outputs DIR writes the packets of the last timed
step as .npy arrays, so that two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BASELINE_FPS = 60.0  # reference headline: >= 60 fps @ 1920x1080


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--sessions", type=int, default=8, help="concurrent sessions per GPU")
    p.add_argument("--width", type=int, default=1920)
    p.add_argument("--height", type=int, default=1080)
    p.add_argument("--content", default="motion", choices=["motion", "desktop", "noise"])
    p.add_argument("--mode", default="striped", choices=["striped", "fullframe"])
    p.add_argument("--stripe-height", type=int, default=64)
    p.add_argument("--qp", type=int, default=25, help="QP (cqp) or CRF value (crf)")
    p.add_argument("--rc", default="crf", choices=["cqp", "crf", "cbr"],
                   help="K10 rate control: crf = the reference's CRF semantics (h264_crf, settings.py:48)")
    p.add_argument("--kbps", type=int, default=8000, help="CBR bitrate (--rc cbr)")
    p.add_argument("--fps", type=float, default=60.0,
                   help="session frame rate the encoders are configured for (CBR frame budget, level)")
    p.add_argument("--av1-kbps", type=int, default=40000,
                   help="AV1 4K120 extra: CBR bitrate (the reference's AV1 encoders run bitrate-controlled in "
                        "the WebRTC mode; 40 Mbit/s = AV1 level 5.1 Main tier maximum); 0 = --rc/--qp")
    p.add_argument("--pool", type=int, default=16, help="pre-rendered frames per session pool")
    p.add_argument("--backend", default="hip", choices=["hip", "cpu"])
    p.add_argument("--encoder", default="h264", choices=["h264", "jpeg", "hevc", "av1"],
                   help="h264 (headline, x264enc-striped equivalent), jpeg stripes, hevc or av1 full frames")
    p.add_argument("--full", action="store_true",
                   help="also run what a plain run leaves out: the end-to-end session checks (--e2e-*) before the "
                        "timed window and the 4K / 8K / CPU 480p sessions (--extra-*) after it; without --full "
                        "those options have no effect and their keys in the result line are null or absent")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write the packets of the last timed step (what the path's caller "
                        "receives) to DIR/packets.npy (every packet's bytes, concatenated, as float32) and "
                        "DIR/packet_index.npy (one float64 row per packet: session, y, height, type, size); the "
                        "inputs are the same from run to run")
    p.add_argument("--extra-4k", type=int, default=1,
                   help="with --full, after the timed window: one 3840x2160 HEVC session (BASELINE config 3, 60 fps) and one "
                        "3840x2160 AV1 session (config 5, 120 fps), each timed over --extra-steps frames and "
                        "reported as extra keys (0 = skip)")
    p.add_argument("--extra-steps", type=int, default=60)
    p.add_argument("--extra-8k", type=int, default=1,
                   help="with --full, after the 4K extras: one 7680x4320 HEVC session at 60 fps (CRF 25 and CBR 40 Mbit/s) and "
                        "one 7680x4320 AV1 session at 60 fps (the reference's largest display, selkies.py:266) on ONE "
                        "GPU, --extra-steps / 2 frames each (0 = skip)")
    p.add_argument("--jpeg-quality", type=int, default=40)
    p.add_argument("--deblock", default="auto", choices=["0", "1", "auto"],
                   help="H.264 in-loop deblocking filter: 1 on, 0 off, auto (the default, as the server runs it): "
                        "the slices coded at QP >= 34 (off at CRF 25 like the reference's x264 ultrafast preset)")
    p.add_argument("--me-full", type=int, default=1, help="H.264 MFMA +-16 exhaustive search candidate (1 on, 0 off)")
    p.add_argument("--bands", type=int, default=1,
                   help="encode each session's frame as N bands of stripes on this GPU (parallel/banded.py): "
                        "byte-identical output, upload overlapped with encoding")
    p.add_argument("--num-refs", type=int, default=1, help="H.264 reference pictures (1 or 2, sliding window)")
    p.add_argument("--overlap", type=int, default=0,
                   help="1: upload frame n+1 while frame n encodes (upload/finish/launch); latency is "
                        "measured from the frame's upload to its packets")
    p.add_argument("--gather", action="store_true", help="sessions run in lockstep and every step's packets of "
                   "all ranks are gathered to rank 0 over RCCL in one collective (--path encoder only)")
    p.add_argument("--dist-bands", action="store_true",
                   help="ONE session of --width x --height split into one band of stripes per rank "
                        "(parallel/dist_banded.py): rank 0 scatters the bands over RCCL, every rank encodes its "
                        "band on its GPU, packets are gathered to rank 0 each step; strong scaling")
    p.add_argument("--e2e-sessions", default="auto",
                   help="with --full, before the timed window (single process, HIP, H.264 only): serve N 1080p60 sessions from "
                        "real server processes (session hosts) to headless websocket clients for --e2e-seconds and report the "
                        "measured capture->client latency; a comma list is tried in order and the first N at "
                        "which every session sustains 60 fps is reported (tools/bench_e2e.py); 'auto' descends "
                        "from the CPU quota's cap in steps of 8; 0 = skip")
    p.add_argument("--e2e-av1", default="3840x2160@120:40000",
                   help="WxH@fps:kbps of the AV1 end-to-end group (one session, encoder svtav1enc, the headless "
                        "client decodes every frame with dav1d: capture->decoded latency); 'none' = skip")
    p.add_argument("--e2e-no-cpu-cap", action="store_true",
                   help="try the session counts even above what the CPU quota can drive (cpu_budget)")
    p.add_argument("--e2e-seconds", type=float, default=4.0)
    p.add_argument("--e2e-warmup", type=float, default=6.0)
    p.add_argument("--e2e-force", action="store_true",
                   help="run the end-to-end check with --backend cpu too (servers use the CPU encoder): the "
                        "multi-rank rehearsal of the per-GPU check on gloo")
    p.add_argument("--e2e-sessions-per-proc", type=int, default=8,
                   help="sessions per server process in the end-to-end check (parallel/multi.py session hosts "
                        "sharing one HIP context; 1 = one process per session)")
    p.add_argument("--e2e-encoder", default="x264enc", choices=["x264enc", "x264enc-striped"],
                   help="encoder the e2e clients request (x264enc = full-frame pictures, the server default)")
    p.add_argument("--path", default="capture", choices=["capture", "encoder"],
                   help="capture: the production capture sessions (csrc/runtime/capture.cpp: native loop, "
                        "grab -> upload -> launch with two frames in flight -> packets -> per-frame callback), "
                        "driven in step mode from a pinned frame pool; encoder: Python threads calling the "
                        "encoder API directly")
    args = p.parse_args()
    if not args.full:   # a plain run: the timed window and nothing else
        args.e2e_sessions, args.e2e_av1, args.extra_4k, args.extra_8k = "0", "none", 0, 0
    return args


def run_capture_path(args, pool, local_rank, fast_cpu=False, last_packets=None, last_frame=0):
    """Times the production serving loop: S native capture sessions on this GPU.

    Each session is a pixelflux ScreenCapture whose frame source is the pinned
    pool (source 4) in step mode: sk_capture_run grants K frames, the native loop
    grabs, uploads, launches (two frames in flight) and collects packets exactly
    as when serving a display; Python only waits. With `last_packets` (a list with
    one slot per session, --dump-outputs) every session has a frame callback that
    counts its frames and copies the packets of frame number `last_frame`.
    """
    import pixelflux
    S = args.sessions
    H, W = pool.array.shape[1], pool.array.shape[2]
    caps = []
    null_cb = ctypes.cast(None, pixelflux.FrameCallback)   # packets stay native: bytes counted in stats()

    def recorder(i):
        seen = [0]

        def on_frame(res, n, user):
            seen[0] += 1
            if seen[0] == last_frame:
                last_packets[i] = [(res[k].stripe_y_start, res[k].stripe_height, res[k].type,
                                    ctypes.string_at(res[k].data, res[k].size)) for k in range(n)]
        return pixelflux.FrameCallback(on_frame)

    for i in range(S):
        if args.encoder == "jpeg":
            mode = pixelflux.OUTPUT_MODE_JPEG
        elif args.encoder == "hevc":
            mode = pixelflux.OUTPUT_MODE_HEVC
        elif args.encoder == "av1":
            mode = pixelflux.OUTPUT_MODE_AV1
        else:
            mode = pixelflux.OUTPUT_MODE_H264
        cs = pixelflux.default_settings(W, H, output_mode=mode, h264_crf=args.qp, use_paint_over_quality=0,
                                        jpeg_quality=args.jpeg_quality, stripe_height=args.stripe_height,
                                        h264_fullframe=int(args.mode == "fullframe"), device=local_rank,
                                        use_cpu=int(args.backend == "cpu"), source=pixelflux.SOURCE_POOL,
                                        step_mode=1, pool_frames=args.pool, pool_stride=W * 4,
                                        pool_phase=3 * i,
                                        target_fps=float(args.fps),
                                        h264_rc_mode={"cqp": 0, "crf": 1, "cbr": 2}[args.rc],
                                        h264_bitrate_kbps=args.kbps if args.rc == "cbr" else 0,
                                        # CPU plumbing (config 1): diamond search, integer vectors
                                        h264_me_full=-1 if fast_cpu else 0, h264_subpel=-1 if fast_cpu else 0)
        cs.pool = pool.array.ctypes.data
        c = pixelflux.ScreenCapture()
        c.start_frame_capture(cs, null_cb if last_packets is None else recorder(i))
        caps.append(c)

    def run_all(count):
        for c in caps:
            c.run(count)
        for c in caps:
            if c.wait(600_000) != 0:
                raise RuntimeError("capture session did not deliver its frames")

    return caps, run_all


def run_e2e(args, W, H, gpu=0, counts=None):
    """Short end-to-end check (tools/bench_e2e.py): N server processes on this GPU, N
    headless websocket clients, W x H at 60 fps. Latency is capture (frame grab) to
    client receipt of the frame's first stripe; the browser's decode/paint is not in it.
    Failures are reported, never raised: the encoder metric above stands on its own."""
    import asyncio
    import types
    try:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import bench_e2e
        ns = types.SimpleNamespace(width=W, height=H, fps=60, crf=args.qp, encoder=args.e2e_encoder,
                                   source="motion", gpu=gpu, use_cpu=args.backend == "cpu", sustain=0.97,
                                   seconds=args.e2e_seconds,
                                   warmup=args.e2e_warmup, hw_queues=None, client_procs=8,
                                   sessions_per_proc=args.e2e_sessions_per_proc,
                                   log_dir=os.path.join("gpurun_out", "bench_e2e_logs", f"gpu{gpu}"))
        os.makedirs(ns.log_dir, exist_ok=True)
        tried = []
        r = None
        for n in (counts or e2e_counts(args)):
            r = asyncio.run(asyncio.wait_for(bench_e2e.run_n(n, ns), 120))
            tried.append({"sessions": n, "sustained": bool(r.get("sustained")), "fps_min": r.get("fps_min")})
            if r.get("sustained"):
                break
        r["tried"] = tried
        r["method"] = (f"measured: session-host processes of {args.e2e_sessions_per_proc} servers each + headless "
                       f"websocket clients (reference protocol, encoder {args.e2e_encoder}), every session >= 97% "
                       "of 60 fps; latency = frame grab -> first packet received")
        return r
    except Exception as ex:   # noqa: BLE001 - reported in the JSON line
        return {"sessions": counts or e2e_counts(args), "error": f"{type(ex).__name__}: {ex}"}


def run_e2e_av1(args, gpu=0):
    """AV1 session group of the end-to-end check: one 4K120 CBR session whose headless
    client decodes every frame with dav1d (models/av1/dav1d.py, 4 threads) on a thread of
    its own. Reports capture -> first packet and capture -> decoded picture; the browser's
    paint is not measured."""
    import asyncio
    import types
    try:
        geo, _, rest = args.e2e_av1.partition("@")
        w, h = (int(x) for x in geo.split("x"))
        fps, _, kbps = rest.partition(":")
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
        import bench_e2e
        ns = types.SimpleNamespace(width=w, height=h, fps=int(fps), crf=args.qp, encoder="svtav1enc", kbps=int(kbps or 0),
                                   source="motion", gpu=gpu, use_cpu=False, sustain=0.97, seconds=args.e2e_seconds,
                                   warmup=args.e2e_warmup, hw_queues=None, client_procs=1, sessions_per_proc=1,
                                   decode=True, decode_threads=4,
                                   log_dir=os.path.join("gpurun_out", "bench_e2e_logs", f"av1_gpu{gpu}"))
        os.makedirs(ns.log_dir, exist_ok=True)
        r = asyncio.run(asyncio.wait_for(bench_e2e.run_n(1, ns), 150))
        r.update(resolution=f"{w}x{h}", target_fps=int(fps), rate_control=f"CBR {kbps} kbit/s" if kbps else "CRF",
                 browser_paint="UNMEASURED",
                 method="measured: one server + one headless websocket client (reference protocol, encoder "
                        "svtav1enc); latency_* = frame grab -> first packet received, decoded_latency_* = frame grab "
                        "-> dav1d returned the picture (4 decoder threads, fed on receipt). The clock starts before "
                        "the grab: the synthetic 4K source copies a 33 MB frame per grab (~7 ms on one core, about "
                        "what an X11 MIT-SHM grab of a 4K screen costs)")
        return r
    except Exception as ex:   # noqa: BLE001 - reported in the JSON line
        return {"error": f"{type(ex).__name__}: {ex}"}


# CPU cost of one end-to-end 1080p60 session, server and client side together:
# 8.9 + 1.1 CPUs for 48 sessions (profiles/r3_e2e_collapse.md); one more CPU per rank
# for the rank's own encoder loop and event handling.
E2E_CPU_PER_SESSION = 0.21
E2E_CPU_PER_RANK = 1.0


def cpu_budget() -> tuple[float, str]:
    """CPUs this command may use and where that number comes from: the cgroup v2 quota
    (/sys/fs/cgroup/cpu.max, what the GPU box enforces), else the affinity mask."""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
        if q != "max":
            return float(q) / float(per), "cgroup cpu.max"
    except (OSError, ValueError):
        pass
    try:
        return float(len(os.sched_getaffinity(0))), "sched_getaffinity"
    except (AttributeError, OSError):
        return float(os.cpu_count() or 1), "os.cpu_count"


def e2e_counts(args, world=1):
    """Session counts tried by the end-to-end check on each GPU. One GPU: the
    default sweep; a node of N GPUs: every rank serves its share of BASELINE config
    4 (64 sessions over 8 GPUs -> 8 per GPU) and one step above it. Counts above what
    this rank's share of the CPU quota can drive (E2E_CPU_PER_SESSION) are dropped:
    past it every session collapses together (profiles/r3_e2e_collapse.md)."""
    v = e2e_counts_uncapped(args, world)
    cap = e2e_cpu_cap(world)
    if v and not getattr(args, "e2e_no_cpu_cap", False):
        fit = [n for n in v if n <= cap]
        v = fit if fit else ([cap] if cap >= 1 else [])
    return v


def e2e_counts_uncapped(args, world=1):
    """'auto' (the default): one GPU descends in steps of 8 sessions from the most this
    rank's CPU share can drive (e2e_cpu_cap) and stops at the first count every session
    sustains, so the reported count is the measured knee and `tried` holds the failing
    count above it; a node of N GPUs serves BASELINE config 4's share per rank."""
    if str(args.e2e_sessions) == "auto":
        if world > 1:
            per = max(1, 64 // world)
            return [2 * per, per]
        top = max(8, e2e_cpu_cap(world) // 8 * 8)
        v = list(range(top, 47, -8))
        return v + [n for n in (32, 16) if n <= top and n not in v]
    v = [int(x) for x in str(args.e2e_sessions).split(",") if x.strip() and int(x) > 0]
    if world > 1 and args.e2e_sessions == "48,32,16":
        per = max(1, 64 // world)
        v = [2 * per, per]
    return v


def e2e_cpu_cap(world=1) -> int:
    cpus, _ = cpu_budget()
    return int(max(0.0, cpus / max(world, 1) - E2E_CPU_PER_RANK) // E2E_CPU_PER_SESSION)


def run_extra(args, W, H, encoder, fps, local_rank, steps, backend=None, cbr_kbps=0):
    """One W x H session of `encoder` through the production capture loop, timed over
    `steps` frames after a warm-up (key frame + steady state); runs after the headline
    window. Reports throughput, capture->packet latency and the frame-interval budget."""
    import types
    from selkies_gstreamer_amd.ops.native import PinnedBuffer
    from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
    try:
        src = SyntheticDesktop(W, H, kind=args.content, seed=7)
        pool = PinnedBuffer((8, H, W, 4))
        for i in range(8):
            src.frame(i, out=pool.array[i])
        a = types.SimpleNamespace(**vars(args))
        a.sessions, a.encoder, a.pool, a.mode, a.fps = 1, encoder, 8, "fullframe", float(fps)
        if backend is not None:
            a.backend = backend
        cpu_fast = a.backend == "cpu" and backend is not None   # x264 "ultrafast"-like tools
        if encoder == "av1" and args.av1_kbps > 0:
            a.rc, a.kbps = "cbr", args.av1_kbps
        if cbr_kbps > 0:
            a.rc, a.kbps = "cbr", cbr_kbps
        caps, run_caps = run_capture_path(a, pool, local_rank, fast_cpu=cpu_fast)
        run_caps(10)
        caps[0].latencies(reset=True)
        b0 = caps[0].stats()["bytes"]
        t0 = time.perf_counter()
        run_caps(steps)
        el = time.perf_counter() - t0
        lat = np.asarray(caps[0].latencies(), dtype=np.float64)
        st = caps[0].stats()
        # the same session fed like a real source: one frame granted every 1/fps s, so the
        # latency has no queueing behind earlier frames (the window above is saturated)
        caps[0].latencies(reset=True)
        tp = time.perf_counter()
        for k in range(steps):
            while True:
                d = tp + k / fps - time.perf_counter()
                if d <= 0:
                    break
                time.sleep(min(d, 0.0005))
            caps[0].run(1)
        if caps[0].wait(600_000) != 0:
            raise RuntimeError("paced window did not deliver its frames")
        paced_el = time.perf_counter() - tp
        plat = np.asarray(caps[0].latencies(), dtype=np.float64)
        # key frames on demand (a client connect / PLI): a few inter frames, then one
        # requested key frame alone in the pipeline, three times
        key_lat, key_kib = [], []
        for _ in range(3):
            caps[0].run(4)
            if caps[0].wait(600_000) != 0:
                raise RuntimeError("inter frames before the key-frame probe did not arrive")
            caps[0].latencies(reset=True)
            kb0 = caps[0].stats()["bytes"]
            caps[0].request_keyframe()
            caps[0].run(1)
            if caps[0].wait(600_000) != 0:
                raise RuntimeError("requested key frame did not arrive")
            kl = caps[0].latencies(reset=True)
            key_lat.append(float(kl[-1]) if kl else float("nan"))
            key_kib.append((caps[0].stats()["bytes"] - kb0) / 1024)
        for c in caps:
            c.close()
        budget = 1000.0 / fps
        p99 = float(np.percentile(lat, 99))
        pp99 = float(np.percentile(plat, 99))
        return {"resolution": f"{W}x{H}", "encoder": encoder, "target_fps": fps, "steps": steps,
                "fps": round(steps / el, 2), "p50_encode_latency_ms": round(float(np.percentile(lat, 50)), 3),
                "p99_encode_latency_ms": round(p99, 3), "max_encode_latency_ms": round(float(lat.max()), 3),
                "frame_interval_ms": round(budget, 3),
                "realtime": bool(steps / el >= fps and p99 < budget),
                "paced": {"fps": round(steps / paced_el, 2), "frames": int(plat.size),
                          "p50_encode_latency_ms": round(float(np.percentile(plat, 50)), 3),
                          "p99_encode_latency_ms": round(pp99, 3),
                          "max_encode_latency_ms": round(float(plat.max()), 3),
                          "method": f"one frame granted every {budget:.3f} ms (source at {fps} fps)"},
                "keyframe": {"latency_ms": [round(x, 3) for x in key_lat], "kib": [round(x, 1) for x in key_kib],
                             "method": "request_keyframe() after 4 inter frames, the key frame alone in the pipeline"},
                "realtime_at_source_rate": bool(steps / el >= fps and pp99 < budget),
                "kib_per_frame": round((st["bytes"] - b0) / steps / 1024, 1),
                "frames_in_flight": st.get("frames_in_flight"), "rate_control": rc_desc(a),
                "backend": a.backend + (" (diamond ME, integer-pel: x264 ultrafast-like)" if cpu_fast else "")}
    except Exception as ex:   # noqa: BLE001 - reported, never fatal for the headline
        return {"resolution": f"{W}x{H}", "encoder": encoder, "error": f"{type(ex).__name__}: {ex}"}


def deblock_arg(args):
    """--deblock as the encoder API takes it (True / False / "auto")."""
    return "auto" if args.deblock == "auto" else args.deblock == "1"


def rc_desc(args) -> str:
    """Rate control of a run, as quoted in the JSON config."""
    return f"CBR {args.kbps} kbit/s" if args.rc == "cbr" else f"{args.rc.upper()} {args.qp}"


DUMP_MAX_VALUES = 15 * 2 ** 20   # float32 values in packets.npy: 60 MiB, the index rides in the rest of 64 MB


def dump_outputs(dirname, sessions, rank=0):
    """--dump-outputs: the packets of the last timed step. `sessions` holds, per session,
    the list of (y, height, type, bytes) the path's caller received for that step (type:
    the stripe result's type on the capture path, the key flag on the encoder path).
    packets.npy: all bytes in session and packet order as float32; beyond DUMP_MAX_VALUES
    a fixed sample (positions drawn with seed 0, ascending). packet_index.npy: one float64
    row (session, y, height, type, size) per packet. Ranks above 0 add _rank<N>."""
    os.makedirs(dirname, exist_ok=True)
    rows = [(i, y, h, typ, len(data)) for i, pk in enumerate(sessions) for y, h, typ, data in pk or []]
    blob = np.frombuffer(b"".join(data for pk in sessions for _, _, _, data in pk or []), dtype=np.uint8)
    if blob.size > DUMP_MAX_VALUES:
        blob = blob[np.sort(np.random.default_rng(0).integers(0, blob.size, DUMP_MAX_VALUES))]
    suffix = f"_rank{rank}" if rank else ""
    np.save(os.path.join(dirname, f"packets{suffix}.npy"), blob.astype(np.float32))
    np.save(os.path.join(dirname, f"packet_index{suffix}.npy"), np.asarray(rows, dtype=np.float64).reshape(-1, 5))


def run_dist_bands(args, torch, dist, rank, world, local_rank):
    """One WxH session across all ranks; returns the result dict on rank 0."""
    from selkies_gstreamer_amd.parallel.dist_banded import DistBandedEncoder
    from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
    W, H = args.width, args.height
    dev = torch.device("cuda", local_rank) if args.backend == "hip" else torch.device("cpu")
    pool = None
    if rank == 0:   # the captured frames live on rank 0's GPU (the capture rank)
        src = SyntheticDesktop(W, H, kind=args.content, seed=0)
        pool = torch.empty((args.pool, H, W, 4), dtype=torch.uint8, device=dev)
        for i in range(args.pool):
            pool[i].copy_(torch.from_numpy(src.frame(i)))
    enc = DistBandedEncoder(W, H, stripe_height=args.stripe_height, backend=args.backend, qp=args.qp,
                            use_paint_over=False, deblock=deblock_arg(args), me_full=bool(args.me_full))

    def sync():
        if args.backend == "hip":
            torch.cuda.synchronize()

    nbytes, lat = 0, []
    for t in range(args.warmup):
        enc.encode(pool[t % args.pool] if rank == 0 else None, t)
    dist.barrier()
    sync()
    t0 = time.perf_counter()
    for t in range(args.warmup, args.warmup + args.steps):
        a = time.perf_counter()
        pk = enc.encode(pool[t % args.pool] if rank == 0 else None, t)
        if pk is not None:
            lat.append(time.perf_counter() - a)
            nbytes += sum(len(p.data) for p in pk)
    sync()
    dist.barrier()
    elapsed = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    elapsed = float(elapsed[0])
    enc.close()
    if rank != 0:
        return None
    if args.dump_outputs:   # rank 0 holds the whole frame's packets of the last step
        dump_outputs(args.dump_outputs, [[(p.y, p.h, int(p.key), p.data) for p in pk]])
    fps = args.steps / elapsed
    lat_ms = np.asarray(lat) * 1e3
    return {
        "metric": "encoded fps of one session split across GPUs (bands over RCCL)",
        "value": round(fps, 2),
        "unit": f"frames/s ({W}x{H} H.264, one session, {world} GPUs)",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "uint8 pixels / int32 integer transforms (bit-exact vs CPU reference)",
        "data": f"synthetic X11-like framebuffer ({args.content}) resident on rank 0's GPU",
        "p50_frame_latency_ms": round(float(np.percentile(lat_ms, 50)), 3),
        "p99_frame_latency_ms": round(float(np.percentile(lat_ms, 99)), 3),
        "kib_per_frame": round(nbytes / args.steps / 1024, 1),
        "config": {"model": f"H.264 Constrained Baseline CAVLC, stripes {args.stripe_height}px, QP {args.qp}",
                   "global_batch": 1, "seq_len": 1, "parallelism": f"bands{world} (scatter + gather per step)",
                   "resolution": f"{W}x{H}", "backend": args.backend, "bands": enc.bands},
    }


def main():
    args = parse()
    if args.gather and args.path != "encoder":
        raise SystemExit("--gather collects packets in Python: use it with --path encoder")
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch = None
    # End-to-end check first, while this process has not touched the GPU: the servers then
    # share the card with nothing else (a live HIP context here, with its hardware queues,
    # cost the sessions ~3 fps and a 59 ms p99 in measurements: profiles/r2_e2e_sessions.md).
    # Every rank checks its own GPU (servers pinned with --gpu-id); rank 0 sums the node.
    e2e = None
    if (e2e_counts(args) and (args.backend == "hip" or args.e2e_force) and args.encoder == "h264"
            and not args.gather and not args.dist_bands):
        e2e = run_e2e(args, args.width, args.height, gpu=local_rank, counts=e2e_counts(args, world))
        time.sleep(3.0)   # let the check's processes, clients and GPU contexts finish tearing down
    e2e_av1 = None
    if (world == 1 and args.e2e_av1 != "none" and args.backend == "hip" and args.encoder == "h264"
            and not args.gather and not args.dist_bands):
        e2e_av1 = run_e2e_av1(args, gpu=local_rank)
        time.sleep(2.0)
    if world > 1:
        import torch as _torch
        import torch.distributed as _dist
        torch, dist = _torch, _dist
        if args.backend == "hip":
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))   # RCCL
        else:   # CPU reference backend: rehearse the multi-rank path with gloo
            dist.init_process_group("gloo")

    def sync():
        if torch is not None and args.backend == "hip":
            torch.cuda.synchronize()

    if args.dist_bands:
        if dist is None:
            import torch as _torch
            import torch.distributed as _dist
            torch, dist = _torch, _dist
            import socket
            so = socket.socket()
            so.bind(("127.0.0.1", 0))
            url = f"tcp://127.0.0.1:{so.getsockname()[1]}"
            so.close()
            if args.backend == "hip":   # one rank: the same device-resident RCCL path as N ranks
                torch.cuda.set_device(local_rank)
                dist.init_process_group("nccl", init_method=url, rank=0, world_size=1,
                                        device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group("gloo", init_method=url, rank=0, world_size=1)
        res = run_dist_bands(args, torch, dist, rank, world, local_rank)
        if res is not None:
            print(json.dumps(res), flush=True)
        dist.destroy_process_group()
        return

    from selkies_gstreamer_amd.ops.native import H264Encoder, JpegEncoder, PinnedBuffer
    from selkies_gstreamer_amd.utils.synthetic import SyntheticDesktop
    from selkies_gstreamer_amd.parallel.numa import bind_to_gpu

    # host threads and pinned frames on the GPU's NUMA node (first touch), before any allocation
    numa_node = bind_to_gpu(local_rank) if args.backend == "hip" else None

    W, H = args.width, args.height
    S = args.sessions
    # pre-rendered capture pool in page-locked memory (an XShm segment in production)
    src = SyntheticDesktop(W, H, kind=args.content, seed=rank)
    pool = PinnedBuffer((args.pool, H, W, 4))
    for i in range(args.pool):
        src.frame(i, out=pool.array[i])
    caps = None
    last_pk = [None] * S   # --dump-outputs: every session's packets of the last timed step
    if args.path == "capture":
        caps, run_caps = run_capture_path(args, pool, local_rank,
                                          last_packets=last_pk if args.dump_outputs else None,
                                          last_frame=args.warmup + args.steps)
        encs = []
    elif args.encoder == "jpeg":
        encs = [JpegEncoder(W, H, stripe_height=args.stripe_height, quality=args.jpeg_quality, use_paint_over=False,
                            device=local_rank, backend=args.backend) for _ in range(S)]
    else:
        if args.bands > 1:
            from selkies_gstreamer_amd.parallel.banded import BandedH264Encoder
            encs = [BandedH264Encoder(W, H, [local_rank] * args.bands, stripe_height=args.stripe_height, qp=args.qp,
                                      use_paint_over=False, backend=args.backend, deblock=deblock_arg(args),
                                      me_full=bool(args.me_full))
                    for _ in range(S)]
        else:
            encs = [H264Encoder(W, H, stripe_height=args.stripe_height, fullframe=args.mode == "fullframe",
                                qp=args.qp, use_paint_over=False, device=local_rank, backend=args.backend,
                                deblock=deblock_arg(args), me_full=bool(args.me_full), num_refs=args.num_refs,
                                rate_control=args.rc, bitrate_kbps=args.kbps if args.rc == "cbr" else 0)
                    for _ in range(S)]

    lat = [[] for _ in range(S)]
    nbytes = [0] * S

    def run(i, first, count, record):
        e = encs[i]
        fr = pool.array
        if args.overlap >= 2 and hasattr(e, "upload"):
            # two frames in flight: frame t+1 is uploaded and launched before frame t's
            # packets are collected, so the GPU never waits for the host between frames
            t_up = {first: time.perf_counter()}
            e.upload(fr[(first + 3 * i) % args.pool], first)
            e.launch()
            for t in range(first, first + count):
                if t + 1 < first + count:
                    t_up[t + 1] = time.perf_counter()
                    e.upload(fr[(t + 1 + 3 * i) % args.pool], t + 1)
                    e.launch()
                pk = e.finish()
                if record:
                    lat[i].append(time.perf_counter() - t_up.pop(t))
                    nbytes[i] += sum(len(p.data) for p in pk)
                    last_pk[i] = pk
            return
        if args.overlap and hasattr(e, "upload"):
            t_up = time.perf_counter()
            e.upload(fr[(first + 3 * i) % args.pool], first)
            e.launch()
            for t in range(first, first + count):
                nxt = t + 1 < first + count
                if nxt:
                    t_next = time.perf_counter()
                    e.upload(fr[(t + 1 + 3 * i) % args.pool], t + 1)   # overlaps frame t's kernels
                pk = e.finish()
                if record:
                    lat[i].append(time.perf_counter() - t_up)
                    nbytes[i] += sum(len(p.data) for p in pk)
                    last_pk[i] = pk
                if nxt:
                    e.launch()
                    t_up = t_next
            return
        for t in range(first, first + count):
            a = time.perf_counter()
            pk = e.encode(fr[(t + 3 * i) % args.pool], t)
            if record:
                lat[i].append(time.perf_counter() - a)
                nbytes[i] += sum(len(p.data) for p in pk)
                last_pk[i] = pk

    gathered = [0]

    def run_lockstep(first, count, record):
        # single-server topology (--gather): every step, all sessions of this rank are
        # submitted, finished, and their packets gathered to rank 0 in one collective
        from selkies_gstreamer_amd.parallel.fanout import gather_packets
        fr = pool.array
        for t in range(first, first + count):
            a = time.perf_counter()
            for i, e in enumerate(encs):
                e.submit(fr[(t + 3 * i) % args.pool], t)
            step = []
            for i, e in enumerate(encs):
                pk = e.finish()
                step.extend((i, p.data) for p in pk)
                if record:
                    nbytes[i] += sum(len(p.data) for p in pk)
                    last_pk[i] = pk
            got = gather_packets(step) if dist is not None else [(0, i, d) for i, d in step]
            if record:
                dt = time.perf_counter() - a
                for i in range(S):
                    lat[i].append(dt)
                if got is not None:
                    gathered[0] += sum(len(d) for _, _, d in got)

    def run_all(first, count, record):
        if args.gather:
            run_lockstep(first, count, record)
            return
        th = [threading.Thread(target=run, args=(i, first, count, record)) for i in range(S)]
        for x in th:
            x.start()
        for x in th:
            x.join()

    if caps is not None:
        run_caps(args.warmup)
        for c in caps:
            c.latencies(reset=True)
        bytes0 = [c.stats()["bytes"] for c in caps]
    else:
        run_all(0, args.warmup, False)

    if dist is not None:
        dist.barrier()
        sync()
    t0 = time.perf_counter()
    if caps is not None:
        run_caps(args.steps)
    else:
        run_all(args.warmup, args.steps, True)
    gather_bytes = gathered[0]
    if dist is not None:
        sync()
        dist.barrier()
    elapsed = time.perf_counter() - t0

    frames = S * args.steps
    inflight_used = None
    upload_fraction = None
    if caps is not None:
        all_lat = np.concatenate([np.asarray(c.latencies(), dtype=np.float64) for c in caps])
        nbytes = [c.stats()["bytes"] - b for c, b in zip(caps, bytes0)]
        inflight_used = max(c.stats().get("frames_in_flight", 0) for c in caps)
        upload_fraction = round(float(np.mean([c.stats().get("upload_fraction", 1.0) for c in caps])), 3)
    else:
        all_lat = np.concatenate([np.asarray(x) for x in lat]) * 1e3
    stats = np.array([elapsed, frames, sum(nbytes), np.percentile(all_lat, 50), np.percentile(all_lat, 99),
                      np.max(all_lat)], dtype=np.float64)
    if dist is not None:
        t = torch.tensor(stats, device="cuda" if args.backend == "hip" else "cpu")
        mx = t.clone()
        dist.all_reduce(mx, op=dist.ReduceOp.MAX)
        sm = t.clone()
        dist.all_reduce(sm, op=dist.ReduceOp.SUM)
        elapsed = float(mx[0])
        frames = int(sm[1])
        total_bytes = float(sm[2])
        p50 = float(mx[3])
        p99 = float(mx[4])
        lat_max = float(mx[5])
    else:
        total_bytes = float(stats[2])
        p50, p99, lat_max = float(stats[3]), float(stats[4]), float(stats[5])
    fps = frames / elapsed
    if args.dump_outputs:
        if caps is None:
            last_pk = [[(p.y, p.h, int(p.key), p.data) for p in pk or []] for pk in last_pk]
        dump_outputs(args.dump_outputs, last_pk, rank)
    for e in encs:
        e.close()
    encs = []
    for c in caps or []:
        c.close()
    caps = None
    # node view of the end-to-end checks (every rank ran its own GPU's)
    e2e_ranks = [e2e]
    if dist is not None:
        e2e_ranks = [None] * world
        dist.all_gather_object(e2e_ranks, e2e)
    node_sessions = None
    if all(r and r.get("sustained") for r in e2e_ranks):
        node_sessions = sum(int(r["sessions"]) for r in e2e_ranks)
    extras = {}
    if args.extra_4k and args.backend == "hip" and not args.gather and rank == 0:
        extras["hevc_4k"] = run_extra(args, 3840, 2160, "hevc", 60, local_rank, args.extra_steps)
        # the same under CBR (the reference's x265enc runs with a bitrate, gstwebrtc_app.py:667-683)
        extras["hevc_4k_cbr"] = run_extra(args, 3840, 2160, "hevc", 60, local_rank, args.extra_steps, cbr_kbps=20000)
        extras["av1_4k"] = run_extra(args, 3840, 2160, "av1", 120, local_rank, 2 * args.extra_steps)
    if args.extra_8k and args.backend == "hip" and not args.gather and rank == 0:
        # one 8K display (MAX_W x MAX_H of the reference's resize path) on one GPU, 60 fps
        extras["hevc_8k"] = run_extra(args, 7680, 4320, "hevc", 60, local_rank, max(args.extra_steps // 2, 4))
        # rate-controlled like the reference's x265enc (and like av1_8k): the pool's wrap-around
        # frames (a full-screen change every 8 frames) no longer code at CRF size
        extras["hevc_8k_cbr"] = run_extra(args, 7680, 4320, "hevc", 60, local_rank, max(args.extra_steps // 2, 4),
                                          cbr_kbps=40000)
        extras["av1_8k"] = run_extra(args, 7680, 4320, "av1", 60, local_rank, max(args.extra_steps // 2, 4))
    if args.extra_4k and args.backend == "hip" and not args.gather and rank == 0:
        # BASELINE config 1 (640x480@30, software H.264 plumbing): the CPU reference encoder
        # through the same capture loop, no GPU involved
        extras["cpu_480p"] = run_extra(args, 640, 480, "h264", 30, local_rank, args.extra_steps, backend="cpu")
    if rank == 0:
        n_gpus = max(world, 1)
        res = {
            "metric": "encoded fps + glass-to-glass p50 ms at 1920x1080; concurrent 60fps sessions/node",
            "value": round(fps, 2),
            "unit": f"frames/s ({W}x{H} {dict(h264='H.264', hevc='HEVC', jpeg='JPEG', av1='AV1')[args.encoder]}, all sessions, all GPUs)",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": round(fps / BASELINE_FPS, 3),
            "dtype": "uint8 pixels / int32 integer transforms (bit-exact vs CPU reference)",
            "data": f"synthetic X11-like framebuffer ({args.content}), pinned host pool of {args.pool} frames"
                    + (", served through native capture sessions (step mode)" if args.path == "capture" else ""),
            "p50_encode_latency_ms": round(p50, 3),
            "p99_encode_latency_ms": round(p99, 3),
            "max_encode_latency_ms": round(lat_max, 3),
            # measured, not derived: N real sessions sustained 60 fps end to end on every GPU of
            # the node, summed over ranks (null if not run / failed anywhere)
            "concurrent_60fps_sessions": node_sessions,
            "encoder_capacity_60fps_sessions": int(fps // 60) if p99 < 1000.0 / 60 else None,
            "capture_to_client_p50_ms": e2e.get("latency_p50_ms") if e2e else None,
            "capture_to_client_p99_ms": e2e.get("latency_p99_ms") if e2e else None,
            "e2e": e2e,
            "e2e_av1_4k": e2e_av1,
            "e2e_cpu": {"cpus": round(cpu_budget()[0], 2), "source": cpu_budget()[1], "ranks": max(world, 1),
                        "cpu_per_session": E2E_CPU_PER_SESSION, "session_cap_per_rank": e2e_cpu_cap(world),
                        # the sweep was cut to what the CPU quota can drive (the GPU could take more)
                        "cpu_bound": any(n > e2e_cpu_cap(world) for n in e2e_counts_uncapped(args, world))},
            "e2e_per_gpu": ([{"gpu": i, "sessions": (r or {}).get("sessions"), "sustained": (r or {}).get("sustained"),
                              "fps_min": (r or {}).get("fps_min"), "latency_p50_ms": (r or {}).get("latency_p50_ms"),
                              "latency_p99_ms": (r or {}).get("latency_p99_ms"), "error": (r or {}).get("error")}
                             for i, r in enumerate(e2e_ranks)] if world > 1 else None),
            **extras,
            "sessions_per_gpu": S,
            "kib_per_frame": round(total_bytes / frames / 1024, 1),
            "gathered_bytes_rank0": gather_bytes,
            "config": {
                "model": (f"H.264 Constrained Baseline CAVLC, {args.mode} stripes {args.stripe_height}px, {rc_desc(args)}"
                          if args.encoder == "h264" else
                          (f"HEVC Main CABAC, CTB 32 quadtree (CU 32/16/8), WPP, slices of {args.stripe_height}px, {rc_desc(args)}"
                           if args.encoder == "hevc" else
                           (f"AV1 Main 8-bit 4:2:0, 64x64 SB, tiles, {rc_desc(args)}" if args.encoder == "av1" else
                            f"baseline JPEG 4:2:0 stripes {args.stripe_height}px, quality {args.jpeg_quality}"))),
                "global_batch": S * n_gpus,
                "seq_len": 1,
                "parallelism": f"session-parallel dp{n_gpus} x {S} sessions/GPU",
                "resolution": f"{W}x{H}",
                "backend": args.backend,
                "deblock": args.deblock if args.encoder == "h264" else None,
                "me_full": bool(args.me_full) if args.encoder == "h264" else None,
                "bands_per_session": args.bands,
                "path": args.path,
                # what the pipeline actually ran with: the capture loop keeps two frames in
                # flight only for a session that has its GPU to itself (capture.cpp overlap_now)
                "upload_overlap": (inflight_used or 0) >= 2 if args.path == "capture" else bool(args.overlap),
                "frames_in_flight": inflight_used if args.path == "capture" else (2 if args.overlap >= 2 else 1),
                # damage-driven upload: share of captured rows that crossed PCIe (the pool
                # source reports changed 16-row bands like XDamage; motion content: all)
                "upload_fraction": upload_fraction,
                "num_refs": args.num_refs,
                "numa_node_rank0": numa_node,
            },
        }
        print(json.dumps(res), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
