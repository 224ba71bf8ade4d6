"""Throughput bench: RT-DETRv2-R101vd, 640², batch 32 per GPU, images/sec (BASELINE.json).

A step = one pass of the /detect hot path over one batch of synthetic uint8
images already resident in HBM: fused preprocess (sp_preprocess_u8) → full
RT-DETRv2 forward → post_process_object_detection (sp_postprocess). Scaling
is one process per GPU with no data-path collective (replicas, "weak"); a
gloo process group only provides the barrier and the max-over-ranks time.

    python bench.py [--gpus N --steps K --warmup W --batch 32 --preset r101vd --size 640]
                    [--dump-outputs DIR] [--full]

A plain run does only what the headline figure needs: set up, W warmup steps, K timed steps, the
outputs of the last timed step to DIR (--dump-outputs), the result line. Everything else the bench
measures (HIP-event rooflines and the per-class breakdown, --detail, the CPU baseline, the
host-input leg and the p50 latency) runs with --full only.

--gpus N > 1 without a torch.distributed launcher: the parent process spawns N
replica processes BEFORE any GPU call, each pinned to one device with
HIP_VISIBLE_DEVICES (one Serve replica per GPU); under
`torch.distributed.run` (WORLD_SIZE set) each rank is already a replica and uses
cuda:LOCAL_RANK. Either way the ranks meet only in a gloo barrier and the max
of their elapsed times; value = all ranks' images / that max.

Prints ONE JSON line (rank 0) with the contract fields; with --full also `roofline` (the
dominant kernel: the fp32-accurate 3-way-split implicit-GEMM conv, HIP-event
timed inside the timed region, priced against ITS pipe ceiling: 2500/6 TFLOP/s
fp32-equivalent on the bf16 MFMA) and `cpu_baseline` (the reference HF path on
the host CPU, bs32 and bs1 legs, median of 3 timed runs each).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 (v_mfma_f32_32x32x16_bf16), not the 2:1-sparse figure
X3_MFMA_PER_BLOCK = 6  # the fp32-accurate split issues 6 bf16 MFMAs per fp32 32x32x16 product block
X3_PEAK_TFLOPS = BF16_MFMA_PEAK_TFLOPS / X3_MFMA_PER_BLOCK  # fp32-equivalent ceiling of that kernel
HBM_PEAK_GBS = 8000.0
BASELINE_METRIC = "images/sec RT-DETRv2-R101 640\u00b2 bs32 at 1/2/4/8 MI355X; p50 /detect latency"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed step returned (scores, labels, boxes, "
                         "counts, logits, pred_boxes) as DIR/<name>.npy (float32)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beside the headline figure: HIP-event rooflines and the per-class "
                         "breakdown (--detail), the CPU baseline, the host-input leg and the p50 latency (each with "
                         "its own --no-* / --latency-iters switch)")
    ap.add_argument("--cpu-baseline-seconds", type=float, default=4.0,
                    help="minimum duration of each timed bs1 CPU run (3 runs, median)")
    ap.add_argument("--cpu-baseline-batch", type=int, default=32,
                    help="batch of the CPU comparison leg (BASELINE.md §3: bs32; 0 = bs1 leg only)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-events", action="store_true", help="skip per-kernel HIP events")
    ap.add_argument("--no-input-supply", action="store_true",
                    help="skip the host-input leg (pinned-host uint8 batches uploaded each step) and host decode rates")
    ap.add_argument("--latency-iters", type=int, default=100,
                    help="bs1 /detect core requests for the p50 latency half of the metric (0 = skip)")
    ap.add_argument("--detail", default=None, help="write per-conv-shape timings (JSON) here")
    ap.add_argument("--stagger", type=int, default=1, help="block offset between micro-batch streams")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "fp32-mfma", "bf16", "bf16-convs", "bf16-all"],
                    help="GEMM operand precision: fp32 = fp32-accurate 3-way bf16 split GEMMs (SP_PREC_F32X3), "
                         "fp32-mfma = v_mfma_f32_32x32x2_f32 GEMMs; bf16 = the separately reported variant (C3/C4)")
    ap.add_argument("--winograd", default=None, choices=["off", "auto", "repvgg", "all"],
                    help="stride-1 3x3 convs as Winograd (default: the Engine's product default)")
    ap.add_argument("--wino-m", type=int, default=None, choices=[2, 4],
                    help="Winograd output tile: F(2x2,3x3) or F(4x4,3x3) (default: the Engine's)")
    ap.add_argument("--fp32-maps", action="store_true",
                    help="bf16 modes: keep the backbone maps in fp32 (A/B of the bf16 activation storage)")
    ap.add_argument("--microbatches", type=int, default=None,
                    help="concurrent per-GPU batch slices on separate streams (2 overlaps GEMM tails, "
                         "but then per-launch durations overlap)")
    ap.add_argument("--stream", default="same", choices=["same", "mixed"],
                    help="same: every source image is --size² (the 640² headline); mixed: the C5 stream, "
                         "sources cycling through MIXED_SOURCES (SURVEY.md §8 D1.3), resized on the GPU to "
                         "--size² inside the timed step, target sizes = the source sizes")
    ap.add_argument("--dist-timeout", type=float, default=300.0,
                    help="seconds the gloo rendezvous / barrier waits for a missing rank")
    ap.add_argument("--stub-step-ms", type=float, default=None, help=argparse.SUPPRESS)  # CPU launcher test
    ap.add_argument("--stub-fail-rank", type=int, default=None, help=argparse.SUPPRESS)  # CPU launcher test
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.detail and not args.full:
        ap.error("--detail needs --full (the per-shape timings come from the profiling pass)")
    return args


# the C5 mixed-resolution stream: source (h, w) sizes cycled image by image
MIXED_SOURCES = [(480, 640), (717, 1200), (720, 1280), (1080, 1920), (1280, 1280), (2160, 3840)]


def stream_plan(n_sources: int, batch: int):
    """Image pool size and, per step of one period, the pool indices of its batch: the stream cycles the
    sources image by image (image j of the stream is source j mod n_sources), so the pool holds
    lcm(n_sources, batch) images and the step pattern repeats every pool // batch steps."""
    import math

    pool = n_sources * batch // math.gcd(n_sources, batch)
    return pool, [[(k * batch + i) % pool for i in range(batch)] for k in range(pool // batch)]


# kernel class -> (bound, peak, unit); peaks from MI355X_MICROARCH.md (dense, no sparsity)
CLASS_BOUND = {
    "conv": ("mfma", None, "TFLOP/s"),  # fp32 or bf16 MFMA peak by --precision
    "attention": ("mfma", FP32_MFMA_PEAK_TFLOPS, "TFLOP/s"),  # sp_attention: v_mfma_f32_16x16x4_f32 (fp32 peak)
    "attention_bf16": ("mfma", BF16_MFMA_PEAK_TFLOPS, "TFLOP/s"),  # sp_attention_bf16: v_mfma_f32_16x16x16_bf16
    "msda": ("hbm", HBM_PEAK_GBS, "GB/s"),
    "preprocess": ("hbm", HBM_PEAK_GBS, "GB/s"),
    "topk": ("hbm", HBM_PEAK_GBS, "GB/s"),
    "postprocess": ("hbm", HBM_PEAK_GBS, "GB/s"),
    "layernorm": ("hbm", HBM_PEAK_GBS, "GB/s"),
    "elementwise": ("hbm", HBM_PEAK_GBS, "GB/s"),
    "wino_tf": ("hbm", HBM_PEAK_GBS, "GB/s"),  # Winograd F(2x2,3x3) input / output transforms
}


def union_ms(ivs):
    union, cur_a, cur_b = 0.0, None, None
    for a, b in sorted(ivs):
        if cur_b is None or a > cur_b:
            if cur_b is not None:
                union += cur_b - cur_a
            cur_a, cur_b = a, b
        else:
            cur_b = max(cur_b, b)
    if cur_b is not None:
        union += cur_b - cur_a
    return union


# the dominant kernel's operand mode per --precision: the split GEMM (x3) on the fp32 parity path
DOMINANT_MODE = {"fp32": "x3", "fp32-mfma": "f32", "bf16": "bf16", "bf16-convs": "bf16", "bf16-all": "bf16"}


class KernelEventRecorder:
    """HIP events around kernel launches, recorded on the launch's own stream (the engine makes
    each micro-batch stream torch's current stream before launching). `only(kind, shape)` limits
    the events to some launches: every event pair is a marker on the stream that costs the GPU
    a few microseconds, so the timed region brackets only the dominant kernel's launches (~1/3 of
    them) and the per-class breakdown comes from a separate, untimed pass with events everywhere."""

    def __init__(self, torch, only=None):
        self.torch = torch
        self.only = only
        self.recs = []
        self.t0 = torch.cuda.Event(enable_timing=True)
        self.t0.record()

    active = True  # the timed region records during one sampled step only (see main)

    def __call__(self, kind, launch, flops, nbytes, shape=None):
        if not self.active or (self.only is not None and not self.only(kind, shape)):
            launch()
            return
        t = self.torch
        e0 = t.cuda.Event(enable_timing=True)
        e1 = t.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        self.recs.append((kind, e0, e1, flops, nbytes, shape))

    def by_shape(self, kind="conv"):
        agg = {}
        for k, e0, e1, f, nb, shp in self.recs:
            if k != kind:
                continue
            a = agg.setdefault(str(shp), [0, 0.0, 0])
            a[0] += 1
            a[1] += e0.elapsed_time(e1)
            a[2] += f
        rows = [{"shape": k, "launches": v[0], "ms": round(v[1], 3),
                 "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 1)} for k, v in agg.items()]
        return sorted(rows, key=lambda r: -r["ms"])

    def conv_modes(self):
        """GEMM operand mode (shape[5]: f32 / bf16 / x3) -> dict(flops, ms = summed launch durations, n)."""
        out = {}
        for k, e0, e1, f, nb, shp in self.recs:
            if k != "conv" or not shp or len(shp) < 6:
                continue
            c = out.setdefault(shp[5], {"flops": 0, "bytes": 0, "ms": 0.0, "n": 0})
            c["flops"] += f
            c["bytes"] += nb
            c["ms"] += e0.elapsed_time(e1)
            c["n"] += 1
        return out

    def classes(self):
        """kind -> dict(ms = sum of launch durations, busy = union of launch intervals, flops, bytes, n)."""
        out = {}
        for k, e0, e1, f, nb, shp in self.recs:
            c = out.setdefault(k, {"ms": 0.0, "ivs": [], "flops": 0, "bytes": 0, "n": 0, "gather": 0})
            if k == "msda" and shp:
                # bytes the bilinear taps fetch (4 corners × Dh value elements per sample), L2-served: SURVEY §8 D1.4
                B_, S_, Q_, H_, Dh_, L_, P_ = shp[:7]
                esz = shp[7] if len(shp) > 7 else 4  # value-row element size (bf16 rows: 2)
                c["gather"] += B_ * Q_ * H_ * L_ * P_ * 4 * Dh_ * esz
            a, b = self.t0.elapsed_time(e0), self.t0.elapsed_time(e1)
            c["ms"] += b - a
            c["ivs"].append((a, b))
            c["flops"] += f
            c["bytes"] += nb
            c["n"] += 1
        for c in out.values():
            c["busy"] = union_ms(c.pop("ivs"))
        return out


def load_traffic(args, avg_alg_bytes, key="conv"):
    """HBM bytes per launch of kernel class `key` from the committed PMC passes
    (tools/pmc_bench.sh), if they were collected on this exact configuration; null otherwise."""
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None, None
    with open(path) as f:
        t = json.load(f)
    cfg_key = f"{args.preset}_{args.size}_bs{args.batch}_{args.precision}_mb{args.mb_eff}" + (
        "_mixed" if getattr(args, "stream", "same") == "mixed" else "")
    e = (t.get(cfg_key) or {}).get("classes", {}).get(key)
    if not e:
        return None, None
    b = e["hbm_bytes_per_launch"]
    return b, {"source": f"profiles/pmc_traffic.json[{cfg_key}].classes.{key}",
               "ratio_to_algorithmic": round(b / avg_alg_bytes, 3)}


def load_gather_ceiling(args, dec_layers):
    """The measured random row-segment gather ceiling for this config's MSDA address pattern
    (tools/microbench/gather_ceiling.py → profiles/r6/msda/gather_ceiling.json): the case with this value-row
    dtype, level maps and batch, preferring this value_all row length. (GB/s, case) or (None, None)."""
    path = os.path.join(ROOT, "profiles", "r6", "msda", "gather_ceiling.json")
    if not os.path.exists(path):
        return None, None
    with open(path) as f:
        cases = json.load(f)["cases"]
    s = args.size // 640
    dt = "bf16" if args.precision in ("bf16", "bf16-all") else "fp32"
    want_map = f"{80 * s}^2+{40 * s}^2+{20 * s}^2"
    ok = [c for c in cases if c["dtype"] == dt and c["map"] == want_map and c["B"] == args.batch]
    if not ok:
        return None, None
    ld = dec_layers * 256
    exact = [c for c in ok if c["ld"] == ld]
    best = max(exact or ok, key=lambda c: c["gather_gbps"])
    return best["gather_gbps"], {"source": "profiles/r6/msda/gather_ceiling.json",
                                 "case": f"{dt} {want_map} B{args.batch} ld{best['ld']} npt{best['npt']}"}


def cpu_baseline(cfg, weights, seconds, batch):
    """Reference CPU path (HF RTDetrImageProcessorPil → RTDetrV2ForObjectDetection fp32 →
    post_process_object_detection) on the host cores, per BASELINE.md §3: a bs1 leg as /detect
    runs it (serve.py:96-109) and a bs`batch` leg (the ≥50× comparison), each 1 warmup + 3 timed
    runs, median images/sec. `value` is the bs`batch` leg (the bs1 leg when batch <= 1)."""
    import numpy as np
    import torch
    from PIL import Image

    from oracle.hf_ref import build_hf_model, build_hf_processor
    from spotter_amd.synthetic import synthetic_image

    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    ncores = int(os.environ.get("OMP_NUM_THREADS", ncores))
    torch.set_num_threads(ncores)
    model = build_hf_model(cfg, weights)
    proc = build_hf_processor()
    S = cfg.image_size
    imgs = [Image.fromarray(synthetic_image(500 + i, S, S)) for i in range(max(4, batch))]

    def run(ims):
        inp = proc(images=ims, return_tensors="pt")
        with torch.no_grad():
            out = model(**inp)
        proc.post_process_object_detection(out, target_sizes=torch.tensor([[im.size[1], im.size[0]] for im in ims]),
                                           threshold=0.5)

    def leg(bs, min_s):
        run(imgs[:bs])  # warmup
        rates, walls = [], []
        for _ in range(3):
            n, t0 = 0, time.perf_counter()
            while True:
                run(imgs[(n // bs * bs) % len(imgs):][:bs] if bs > 1 else [imgs[n % len(imgs)]])
                n += bs
                if time.perf_counter() - t0 >= min_s:
                    break
            walls.append(time.perf_counter() - t0)
            rates.append(n / walls[-1])
        return {"value": float(np.median(rates)), "runs": [round(r, 3) for r in rates],
                "seconds": round(sum(walls), 1), "batch": bs}

    legs = {"bs1": leg(1, seconds)}
    if batch > 1:
        legs[f"bs{batch}"] = leg(batch, 0.0)  # one bs`batch` forward per timed run
    main_leg = legs[f"bs{batch}"] if batch > 1 else legs["bs1"]
    cpu_model = None
    try:
        with open("/proc/cpuinfo") as f:
            cpu_model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), None)
    except OSError:
        pass
    nt = torch.get_num_threads()
    return {"value": round(main_leg["value"], 3), "unit": "images/sec", "cores": nt, "kind": "reference",
            "cpu_model": cpu_model, "legs": legs,
            "sample": f"HF transformers RTDetrImageProcessorPil+RTDetrV2ForObjectDetection(fp32, synthetic "
                      f"{cfg.name} weights)+post_process_object_detection on {nt} host threads, "
                      f"{S}x{S} synthetic images; value = bs{main_leg['batch']} leg, median of 3 timed runs "
                      f"after 1 warmup (bs1 leg: 3 runs of >= {seconds:g} s)"}


def _visible_devices():
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v:
            return [d.strip() for d in v.split(",") if d.strip()]
    return None


def launch_replicas(args) -> int:
    """--gpus N without a distributed launcher: N replica processes, spawned before this process
    touches any GPU, replica i pinned to device i by HIP_VISIBLE_DEVICES. Rank 0's
    stdout (the JSON line) passes through; the other ranks' stdout goes to stderr."""
    import socket
    import subprocess

    n = args.gpus
    vis = _visible_devices()
    if vis is not None and len(vis) < n:
        print(f"bench.py: --gpus {n} but only {len(vis)} visible devices ({','.join(vis)})", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for i in range(n):
        env = dict(os.environ)
        dev = vis[i] if vis is not None else str(i)
        env.update(RANK=str(i), WORLD_SIZE=str(n), LOCAL_RANK=str(i), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HIP_VISIBLE_DEVICES=dev,
                   CUDA_VISIBLE_DEVICES=dev, SPOTTER_REPLICA_DEVICE="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=None if i == 0 else sys.stderr))
    # poll every child: the first non-zero exit (any rank) kills the others at once, instead of rank 0
    # sitting in the gloo rendezvous / barrier until its timeout
    rc, failed = 0, None
    try:
        live = list(range(n))
        while live:
            for i in list(live):
                code = procs[i].poll()
                if code is None:
                    continue
                live.remove(i)
                if code != 0 and failed is None:
                    rc, failed = code, i
            if failed is not None:
                break
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    if failed is not None:
        print(f"bench.py: replica rank {failed} exited with {rc}; stopped the other ranks", file=sys.stderr)
    return rc


def conv_roofline(rec, cl, args, bf, rec_timed=None):
    """The dominant kernel's roofline. fp32 (the parity path): the 3-way-split kernel (x3 mode),
    priced against its own pipe ceiling, 2500/6 TF fp32-equivalent (six bf16 MFMAs per fp32
    32x32x16 block); the fp32-MFMA figure stays as a secondary field. Other precisions: the
    whole conv class against the mode's MFMA peak. rec_timed: the events of the timed region
    (dominant launches only) — the achieved figure comes from there; rec (every launch, the
    profiling pass) gives the per-mode and conv-class context."""
    modes = {}
    per_mfma = {"x3": (X3_MFMA_PER_BLOCK, "v_mfma_f32_32x32x16_bf16", BF16_MFMA_PEAK_TFLOPS),
                "bf16": (1, "v_mfma_f32_32x32x16_bf16", BF16_MFMA_PEAK_TFLOPS),
                "f32": (1, "v_mfma_f32_32x32x2_f32", FP32_MFMA_PEAK_TFLOPS),
                "f32+ln": (1, "v_mfma_f32_32x32x2_f32 (+ fused row LayerNorm)", FP32_MFMA_PEAK_TFLOPS),
                "direct": (1, "v_fma_f32 (VALU stem conv, no MFMA)", FP32_MFMA_PEAK_TFLOPS),
                "bf16-direct": (1, "v_mfma_f32_32x32x16_bf16 (direct LDS-halo stem 3x3)", BF16_MFMA_PEAK_TFLOPS),
                "f32-direct": (1, "v_mfma_f32_32x32x2_f32 (direct LDS-halo stem 3x3)", FP32_MFMA_PEAK_TFLOPS)}
    cm = rec.conv_modes()
    for md, c in cm.items():
        a = c["flops"] / (c["ms"] * 1e-3) / 1e12
        mult, instr, pk = per_mfma[md]
        modes[md] = {"flop_share": round(c["flops"] / max(1, cl["conv"]["flops"]), 4),
                     "ms_per_step": round(c["ms"] / args.steps, 3), "launches_per_step": c["n"] // args.steps,
                     "avg_launch_ms": round(c["ms"] / c["n"], 4),
                     "achieved": round(a, 2), "unit": "TFLOP/s", "frac_of_mode_ceiling": round(a * mult / pk, 4),
                     "mfma_issue": {"instr": instr, "mfma_per_fp32_block": mult,
                                    "achieved": round(mult * a, 1), "peak": pk, "frac": round(mult * a / pk, 4)}}
    c = cl["conv"]
    # the convolutions' work in the direct (implicit-GEMM) formulation over the time of every conv-class
    # launch plus the Winograd transforms: what the Winograd path buys, apart from the kernel's own rate
    direct_flops = 0
    for k, e0, e1, f, nb, shp in rec.recs:
        if k == "conv":
            direct_flops += (2 * shp[7] * shp[1] * 9 * shp[2]) if (shp and len(shp) > 6 and shp[6] == "wino") else f
    conv_wino_ms = c["busy"] + cl.get("wino_tf", {}).get("busy", 0.0)
    timed = rec_timed is not None and bool(rec_timed.recs)
    cmt = rec_timed.conv_modes() if timed else cm
    tsteps = 1 if timed else args.steps  # the timed recorder covers one sampled step
    if args.precision == "fp32" and "x3" in cmt:
        x = cmt["x3"]
        ach = x["flops"] / (x["ms"] * 1e-3) / 1e12
        alg_bytes = x["bytes"] / x["n"]
        traffic, tnote = load_traffic(args, alg_bytes, key="conv_x3")
        roof = {"bound": "mfma", "kernel": "conv x3 kernels (fp32 operands split hi/mid/lo bf16, 6 "
                                           "v_mfma_f32_32x32x16_bf16 per fp32 32x32x16 block, implicit GEMM)",
                "achieved": round(ach, 2), "peak": round(X3_PEAK_TFLOPS, 2), "unit": "TFLOP/s",
                "frac": round(ach / X3_PEAK_TFLOPS, 4), "traffic": traffic,
                "peak_note": "fp32-equivalent ceiling of the split kernel = dense bf16 MFMA 2500 TF / 6",
                "vs_fp32_mfma_peak": {"peak": FP32_MFMA_PEAK_TFLOPS, "frac": round(ach / FP32_MFMA_PEAK_TFLOPS, 4)},
                "launches_per_step": x["n"] // tsteps, "avg_launch_ms": round(x["ms"] / x["n"], 4),
                "gflop_per_launch": round(x["flops"] / x["n"] / 1e9, 3),
                "algorithmic_bytes_per_launch": int(alg_bytes),
                "flop_share_of_conv_class": round(x["flops"] / max(1, c["flops"]), 4),
                "conv_class": {"achieved": round(c["flops"] / (c["busy"] * 1e-3) / 1e12, 2),
                               "direct_equivalent": {
                                   "tflops": round(direct_flops / (conv_wino_ms * 1e-3) / 1e12, 2),
                                   "gflop_per_step": round(direct_flops / args.steps / 1e9, 1),
                                   "ms_per_step": round(conv_wino_ms / args.steps, 3),
                                   "note": "FLOPs of the direct implicit-GEMM formulation of every conv / linear "
                                           "over the conv launches + Winograd transforms; counts the 2.25x "
                                           "multiply saving of the Winograd 3x3s as throughput"},
                               "ms_per_step": round(c["busy"] / args.steps, 3),
                               "launches_per_step": c["n"] // args.steps,
                               "gflop_per_step": round(c["flops"] / args.steps / 1e9, 2)},
                "note": "achieved = algorithmic fp32 FLOPs of the x3 launches (direct convs / linears and the "
                        "Winograd component GEMMs) / the sum of their durations (HIP events on the launch "
                        "stream, inside the timed region); traffic = HBM bytes per x3 launch from PMC "
                        "FETCH_SIZE x2 + WRITE_SIZE (MI355X_MICROARCH.md gfx950 correction)"}
    else:
        conv_peak = BF16_MFMA_PEAK_TFLOPS if bf else FP32_MFMA_PEAK_TFLOPS
        ach = c["flops"] / (c["busy"] * 1e-3) / 1e12
        alg_bytes = c["bytes"] / c["n"]
        traffic, tnote = load_traffic(args, alg_bytes)
        roof = {"bound": "mfma", "kernel": f"conv class ({args.precision})", "achieved": round(ach, 2),
                "peak": conv_peak, "unit": "TFLOP/s", "frac": round(ach / conv_peak, 4), "traffic": traffic,
                "launches_per_step": c["n"] // args.steps, "avg_launch_ms": round(c["ms"] / c["n"], 4),
                "gflop_per_launch": round(c["flops"] / c["n"] / 1e9, 3),
                "algorithmic_bytes_per_launch": int(alg_bytes),
                "gflop_per_step": round(c["flops"] / args.steps / 1e9, 2)}
    if tnote:
        roof["traffic_source"] = tnote
    roof["modes"] = modes
    return roof


def make_step(args, rank, local):
    """(step, sync, roofline_fn) for one replica. The stub (CPU launcher test) sleeps instead."""
    if args.stub_step_ms is not None:
        return (lambda: time.sleep(args.stub_step_ms / 1e3)), (lambda: None), None

    import torch

    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    from spotter_amd import ops
    from spotter_amd.config import PRESETS
    from spotter_amd.engine import Engine
    from spotter_amd.synthetic import synthetic_batch
    from spotter_amd.weights import generate

    cfg = PRESETS[args.preset].replace(image_size=args.size)
    weights = generate(cfg, seed=0)
    ekw = {} if args.winograd is None else {"winograd": False if args.winograd == "off" else args.winograd}
    if args.wino_m is not None:
        ekw["wino_m"] = args.wino_m
    if args.fp32_maps:
        ekw["bf16_store"] = False
    eng = Engine(cfg, weights, dev, precision=args.precision, **ekw)
    if args.microbatches is not None:
        eng.microbatches = args.microbatches
    args.mb_eff = eng.micro_batches_for(args.batch)
    eng.stagger = args.stagger
    B, S = args.batch, args.size
    K = cfg.num_queries
    if args.stream == "mixed":
        # C5: a pool of uint8 sources of the stream's sizes, resident in HBM; each step takes the next B of
        # the cycle (different sizes in one batch, resized on the GPU), post-processed at its source sizes
        from spotter_amd.synthetic import synthetic_image

        npool, plan = stream_plan(len(MIXED_SOURCES), B)
        pool = [torch.from_numpy(synthetic_image(1234 + 1000 * rank + j, *MIXED_SOURCES[j % len(MIXED_SOURCES)]))
                .to(dev) for j in range(npool)]
        batches = [([pool[j] for j in idx], torch.tensor([list(pool[j].shape[:2]) for j in idx], dtype=torch.int32,
                                                          device=dev)) for idx in plan]
    else:
        imgs_host = synthetic_batch(B, S, S, seed0=1234 + 1000 * rank)
        batches = [([torch.from_numpy(im).to(dev) for im in imgs_host],  # resident in HBM
                    torch.tensor([[S, S]] * B, dtype=torch.int32, device=dev))]
    px = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    scores = torch.empty((B, K), device=dev)
    labels = torch.empty((B, K), dtype=torch.int64, device=dev)
    boxes = torch.empty((B, K, 4), device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    work = torch.empty((B, K), dtype=torch.int32, device=dev)
    it = [0]
    last = {}

    def step():
        imgs, tsz = batches[it[0] % len(batches)]
        it[0] += 1
        ops.preprocess_u8(imgs, px, S, S)
        logits, pred = eng.forward(px)
        ops.postprocess(logits, pred, tsz, K, 0.5, scores, labels, boxes, counts, work)
        last["logits"], last["pred_boxes"] = logits, pred  # engine-owned, overwritten by the next forward

    def outputs():
        """What the last step returned, as host float32 arrays (--dump-outputs): the post-processed detections
        (all K sorted candidates per image; the first counts[b] pass the threshold) and the forward's outputs."""
        dev_out = dict(scores=scores, labels=labels, boxes=boxes, counts=counts, **last)
        return {k: v.detach().to("cpu", torch.float32).numpy() for k, v in dev_out.items()}

    step.outputs = outputs
    step.cfg, step.weights = cfg, weights
    step.input_supply = None
    if args.stream == "same":
        step.input_supply = lambda steps, warmup: host_input_leg(torch, ops, eng, imgs_host, dev, px, batches[0][1],
                                                                 (scores, labels, boxes, counts, work), S, K,
                                                                 steps, warmup)
    return step, torch.cuda.synchronize, ops.set_launch_hook


def host_input_leg(torch, ops, eng, imgs_host, dev, px, tsz, outs, S, K, steps, warmup):
    """The same step with its uint8 batch supplied from pinned HOST memory every step (SURVEY §8e "Risks"):
    a copy stream uploads batch i+1 into one of two device slots while the compute stream runs step i (the
    upload waits only until step i-1's preprocess has read that slot). Returns (img/s, H2D facts)."""
    import numpy as np

    B = len(imgs_host)
    pinned = torch.from_numpy(np.stack(imgs_host)).pin_memory()  # [B, S, S, 3] uint8
    slots = [torch.empty(pinned.shape, dtype=torch.uint8, device=dev) for _ in range(2)]
    copy_s, comp = torch.cuda.Stream(dev), torch.cuda.current_stream(dev)
    uploaded = [torch.cuda.Event() for _ in range(2)]
    read = [torch.cuda.Event() for _ in range(2)]

    def upload(i):
        k = i % 2
        copy_s.wait_event(read[k])  # step i-2's preprocess has consumed this slot
        with torch.cuda.stream(copy_s):
            slots[k].copy_(pinned, non_blocking=True)
        uploaded[k].record(copy_s)

    def run(n):
        upload(0)
        for i in range(n):
            if i + 1 < n:
                upload(i + 1)
            k = i % 2
            comp.wait_event(uploaded[k])
            ops.preprocess_u8([slots[k][b] for b in range(B)], px, S, S)
            read[k].record(comp)
            logits, pred = eng.forward(px)
            ops.postprocess(logits, pred, tsz, K, 0.5, *outs)

    run(max(2, warmup))
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize(dev)
    t = time.perf_counter() - t0
    # the upload alone, back to back on the copy stream
    n_up = 10
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(copy_s)
    with torch.cuda.stream(copy_s):
        for _ in range(n_up):
            slots[0].copy_(pinned, non_blocking=True)
    e1.record(copy_s)
    torch.cuda.synchronize(dev)
    up_ms = e0.elapsed_time(e1) / n_up
    nbytes = pinned.numel()
    return B * steps / t, {"bytes_per_batch": nbytes, "h2d_ms_per_batch": round(up_ms, 3),
                           "h2d_gbps": round(nbytes / up_ms / 1e6, 1), "ms_per_step": round(1000 * t / steps, 3)}


DUMP_LIMIT_BYTES = 64_000_000


def dump_outputs(out_dir, arrays):
    """--dump-outputs: each array as out_dir/<name>.npy. Within DUMP_LIMIT_BYTES in all: an array over its
    equal share of the limit is stored as a fixed seeded sample of its flattened elements (sorted indices)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_LIMIT_BYTES // max(1, len(arrays))
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if a.nbytes > share:
            idx = np.sort(np.random.default_rng(0).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def host_decode_rates(seconds=1.0):
    """Host JPEG entropy decode per core (the Huffman half of the drop-in's GPU decode, sp_jpeg_decode_coefs, one
    thread) and Pillow's whole decode (what the reference runs, serve.py:96-97), images/s per core, for the
    reference's 1200x717 fixture and a 640x640 JPEG of the bench's synthetic content (Pillow quality 75)."""
    import io

    from PIL import Image

    from spotter_amd.jpeg import decode_coefs
    from spotter_amd.synthetic import synthetic_batch

    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "tests", "golden", "test_pic.jpg"), "rb") as f:
        fixture = f.read()
    b = io.BytesIO()
    Image.fromarray(synthetic_batch(1, 640, 640, seed0=1234)[0]).save(b, "JPEG", quality=75)
    out = {}
    for name, data in (("fixture_1200x717", fixture), ("synthetic_640x640_q75", b.getvalue())):
        rates = {}
        for what, fn in (("entropy_decode", lambda d=data: decode_coefs(d)),
                         ("pillow_decode", lambda d=data: Image.open(io.BytesIO(d)).convert("RGB"))):
            fn()
            n, t0 = 0, time.perf_counter()
            while time.perf_counter() - t0 < seconds:
                fn()
                n += 1
            rates[what] = round(n / (time.perf_counter() - t0), 1)
        out[name] = {"bytes": len(data), "img_per_s_per_core": rates}
    return out


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_replicas(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("SPOTTER_REPLICA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    if args.gpus > 1 and world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        return 2
    if args.stub_fail_rank is not None and rank == args.stub_fail_rank:
        return 3  # CPU launcher test: this replica dies before the rendezvous
    dist = None
    if world > 1:
        import torch.distributed as dist

        import datetime

        # a rank that never arrives ends the run in minutes, not gloo's 30-minute default
        dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=args.dist_timeout))
    from spotter_amd.replicas import all_gather_obj, barrier, max_over_ranks

    step, sync, set_hook = make_step(args, rank, local)
    for _ in range(args.warmup):
        step()
    sync()

    rec, rec_timed = None, None
    if set_hook is not None and args.full and not args.no_events:
        import torch

        dom = DOMINANT_MODE[args.precision]
        rec_timed = KernelEventRecorder(torch, only=lambda k, shp: k == "conv" and bool(shp) and shp[5] == dom)
        set_hook(rec_timed)

    barrier()
    sync()
    sample = args.steps // 2  # the timed step whose dominant-kernel launches carry HIP events
    t0 = time.perf_counter()
    for i in range(args.steps):
        if rec_timed is not None:
            rec_timed.active = i == sample
        step()
    sync()
    t1 = time.perf_counter()
    barrier()
    if set_hook is not None:
        set_hook(None)
    if args.dump_outputs and rank == 0 and getattr(step, "outputs", None) is not None:
        dump_outputs(args.dump_outputs, step.outputs())  # before any further pass overwrites them
    mine = t1 - t0
    elapsed = max_over_ranks(mine)
    B = args.batch
    per_rank = all_gather_obj({"rank": rank, "device": os.environ.get("HIP_VISIBLE_DEVICES", str(local)),
                               "value": round(B * args.steps / mine, 2),
                               "ms_per_step": round(1000 * mine / args.steps, 3)})
    n_img = world * B * args.steps
    value = n_img / elapsed

    if rec_timed is not None:
        # profiling pass (not timed, not in `value`): events around every launch for the per-class
        # breakdown, the per-shape detail and the conv-mode context of the roofline
        import torch

        rec = KernelEventRecorder(torch)
        set_hook(rec)
        for _ in range(args.steps):
            step()
        sync()
        set_hook(None)

    roof, classes = None, None
    if rec is not None and rec.recs:
        cl = rec.classes()
        bf = args.precision.startswith("bf16")
        conv_peak = BF16_MFMA_PEAK_TFLOPS if bf else FP32_MFMA_PEAK_TFLOPS
        classes = {}
        for kind, c in sorted(cl.items(), key=lambda kv: -kv[1]["ms"]):
            bound, peak, unit = CLASS_BOUND[kind]
            peak = peak or conv_peak
            # concurrent micro-batch streams overlap launches of one class: use the busy-time union
            work = c["bytes"] / 1e9 if unit == "GB/s" else c["flops"] / 1e12
            ach = work / (c["busy"] * 1e-3)
            classes[kind] = {"bound": bound, "achieved": round(ach, 2), "peak": peak, "unit": unit,
                             "frac": round(ach / peak, 4), "ms_per_step": round(c["busy"] / args.steps, 3),
                             "launches_per_step": c["n"] // args.steps}
            tr, tnote = load_traffic(args, c["bytes"] / max(1, c["n"]), key=kind)
            if tr is not None:  # PMC HBM bytes per launch of this class, when collected on this config
                classes[kind]["traffic"] = tr
                classes[kind]["traffic_source"] = tnote
            if kind == "msda":
                # The value rows a launch touches depend on the sampled locations, so no a-priori byte count is
                # compulsory: the whole value map (what `bytes` holds) over-counts 2-4x. The HBM-bound figure is
                # the measured HBM traffic (PMC, tools/pmc_bench.sh) over the measured time when it was
                # collected on this config; the whole-map figure stays as a diagnostic upper bound.
                whole = {"achieved": round(ach, 2), "frac": round(ach / peak, 4),
                         "bytes_per_launch": c["bytes"] // max(1, c["n"]),
                         "note": "whole value map + offsets/weights/ref + output per launch: an upper bound on "
                                 "the compulsory bytes, not what the kernel reads"}
                classes[kind]["whole_value_map"] = whole
                if tr is not None:
                    a_pmc = tr * c["n"] / 1e9 / (c["busy"] * 1e-3)
                    classes[kind].update(achieved=round(a_pmc, 2), frac=round(a_pmc / peak, 4),
                                         bytes_basis="pmc_hbm_traffic")
                    classes[kind]["traffic_source"] = dict(tnote, ratio_to_algorithmic=1.0,
                                                           note="algorithmic bytes := measured HBM bytes")
                else:
                    classes[kind]["bytes_basis"] = "whole_value_map (no PMC traffic for this config)"
            if c.get("gather"):
                g_rate = c["gather"] / 1e9 / (c["busy"] * 1e-3)
                classes[kind]["l2_gather"] = {
                    "achieved": round(g_rate, 1), "unit": "GB/s",
                    "bytes_per_launch": c["gather"] // c["n"],
                    "note": "sampled-corner bytes (4 taps × Dh × element size per sample); the value map stays in "
                            "L2 / Infinity Cache, so this is an L2 gather rate, not an HBM bound"}
                gc, gnote = load_gather_ceiling(args, step.cfg.decoder_layers)
                if gc:
                    classes[kind]["gather_ceiling"] = {
                        "peak": gc, "unit": "GB/s", "frac": round(g_rate / gc, 4), **gnote,
                        "note": "measured ceiling of random 128-byte (fp32) / 64-byte (bf16) row-segment gathers in "
                                "msda's address pattern on this chip (uniform random locations, XCD-major grid); "
                                "frac = l2_gather.achieved / peak"}
        roof = conv_roofline(rec, cl, args, bf, rec_timed)
        roof["events"] = ("timed region: events around the dominant kernel's launches of one sampled step "
                          "(step K//2); kernel_classes, modes and conv_class: a separate untimed pass of the "
                          "same K steps with events on every launch")

    if rec is not None and args.detail and rank == 0:
        with open(args.detail, "w") as f:
            json.dump(rec.by_shape(), f, indent=1)

    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline and args.stub_step_ms is None:
        try:
            cpu = cpu_baseline(step.cfg, step.weights, args.cpu_baseline_seconds, args.cpu_baseline_batch)
        except Exception as e:  # keep the GPU line even if the host path is unavailable
            cpu = {"value": None, "unit": "images/sec", "cores": None, "kind": "reference",
                   "sample": f"unavailable: {type(e).__name__}: {e}"}

    supply = None
    if (rank == 0 and world == 1 and args.full and not args.no_input_supply and args.stub_step_ms is None
            and getattr(step, "input_supply", None) is not None):
        try:
            v_host, h2d = step.input_supply(args.steps, args.warmup)
            dec = host_decode_rates()
            per_core = dec["synthetic_640x640_q75"]["img_per_s_per_core"]["entropy_decode"]
            supply = {"host_input_img_s": round(v_host, 2), "resident_img_s": round(value, 2),
                      "host_vs_resident": round(v_host / value, 4), **h2d,
                      "pcie_bound_img_s": round(B / (h2d["h2d_ms_per_batch"] / 1e3), 1),
                      "host_decode": dec,
                      "host_cores_per_gpu_at_resident_rate": round(value / per_core, 1),
                      "note": "host_input: the bs32 uint8 batch uploaded from pinned host memory each step on a copy "
                              "stream overlapping the previous step's compute; host_decode: one core, images/s; "
                              "cores per GPU = resident img/s / the 640x640 entropy-decode rate (the GPU does the "
                              "rest of the decode)"}
        except Exception as e:
            supply = {"error": f"{type(e).__name__}: {e}"}

    lat = None
    if rank == 0 and world == 1 and args.full and args.latency_iters > 0 and args.stub_step_ms is None:
        try:
            from spotter_amd import SpotterForObjectDetection
            from spotter_amd.config import PRESETS
            from tools import detect_path
            from tools.latency import measure

            lat_model = SpotterForObjectDetection(PRESETS[args.preset], use_graphs=True)
            lat = measure(args.preset, args.latency_iters, graphs=True, model=lat_model)  # GPU JPEG decode
            lat["full_request"] = detect_path.measure(args.preset, args.latency_iters, model=lat_model)
            # the same core with the reference's host decode (Pillow), for the decode stage's comparison
            h = measure(args.preset, max(20, args.latency_iters // 2), graphs=True, model=lat_model, decode="host")
            lat["host_decode"] = {k: h[k] for k in ("p50_ms", "p95_ms", "stages_p50_ms")}
            # the whole request with the reference's own PIL.Image (host decode, Pillow draw + encode): the
            # comparison for the GPU decode / encode stages
            fh = detect_path.measure(args.preset, max(20, args.latency_iters // 2), model=lat_model, decode="host")
            lat["full_request_host_image"] = {k: fh[k] for k in ("p50_ms", "p95_ms", "stages_p50_ms")}
        except Exception as e:
            lat = {"error": f"{type(e).__name__}: {e}"}

    if rank == 0:
        S = args.size
        mixed = args.stream == "mixed"
        workload = f"RT-DETRv2-{args.preset} {S}x{S} batch={B}/GPU preprocess+forward+postprocess"
        if mixed:
            workload = (f"RT-DETRv2-{args.preset} mixed-resolution stream (sources cycling "
                        f"{', '.join(f'{h}x{w}' for h, w in MIXED_SOURCES)}, uint8 resident in HBM) resized on the "
                        f"GPU to {S}x{S} inside the step, batch={B}/GPU preprocess+forward+postprocess")
        line = {
            "metric": (BASELINE_METRIC if (args.preset, S, B, args.precision, mixed) == ("r101vd", 640, 32, "fp32", False)
                       else f"images/sec RT-DETRv2-{args.preset} {S}² bs{B} {args.precision}"
                       + (" mixed-resolution stream" if mixed else "")),
            "value": round(value, 2), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1000 * elapsed / args.steps, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.precision,
            "data": "synthetic uint8 RGB images (seeded), synthetic deterministic weights",
            "config": {"workload": workload, **({"stream_sources_hw": MIXED_SOURCES} if mixed else {}),
                       "model": f"rtdetr_v2_{args.preset}", "global_batch": B * world, "image_size": S,
                       "parallelism": f"replicas x{world}"},
            "per_rank": per_rank,
            "roofline": roof, "kernel_classes": classes, "cpu_baseline": cpu, "latency": lat,
            "input_supply": supply,
        }
        # vs_baseline stays null: BASELINE.md §1 holds no published number for this metric (the reference
        # publishes none). The same-run CPU reference ratio is reported beside it.
        if isinstance(cpu, dict) and cpu.get("value"):
            # against the faster CPU leg per image (bs1 runs 3-4x more images/s than bs32 on the host), with
            # the same-workload (bs32) ratio beside it
            legs = [l["value"] for l in (cpu.get("legs") or {}).values() if l.get("value")] or [cpu["value"]]
            line["vs_cpu_baseline"] = round(value / max(legs), 1)
            line["vs_cpu_baseline_same_batch"] = round(value / cpu["value"], 1)
        if args.stub_step_ms is not None:
            line["data"] = "STUB: no GPU step (launcher test)"
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
