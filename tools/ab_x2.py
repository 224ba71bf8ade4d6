"""A/B of the TF32-class tier (precision "fp32-x2": 2-way bf16 split, three MFMA products) against the 3-way split
("fp32") and the one-plane bf16 kernels, in one process: interleaved rounds, HIP events, medians and the old side's
own spread (the style of tools/ab_direct_x3.py).

    python tools/ab_x2.py layers   [--out f.json] [--rounds 5] [--reps 10] [--detail profiles/r5/x3/conv_detail_c2_r5c.json]
        per layer: "x3" vs "x2" on the same tile (and the one-plane bf16 kernel as the ceiling) for the C2 step's
        largest split-GEMM buckets of a committed `bench.py --full --detail` file, among them the stage-3 expand
        51200×1024×256 with its residual, a Winograd F(4×4) component batch and a decoder linear
    python tools/ab_x2.py e2e      [--out f.json] [--rounds 3] [--steps 5]
        Engine.forward at bs32 640² R101vd: "fp32" vs "fp32-x2" vs "bf16", alternating
    python tools/ab_x2.py expand --mode x3|x2 [--reps 20]
        the stage-3 expand alone, for a counter pass of its own (rocprofv3 --pmc ... -- python tools/ab_x2.py expand ...)
    python tools/ab_x2.py accuracy [--out f.json] [--reps 1]
        tools/bf16_delta.py's figures (recall, AP, p50 / p95 |Δscore| against the HF fp32 goldens) for "fp32-x2"
"""
import argparse
import ast
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from spotter_amd import ops
from spotter_amd.ops import V

DECODER_LINEAR = (9600, 1024, 256, 1, 1, "x3", "epi:bn")  # the decoder FFN's first linear at bs32 (32 × 300 rows)


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def buckets(detail, top):
    """The largest split-GEMM buckets (launch-hook shape tuples tagged "x3") of a bench.py --detail file, by time."""
    rows = json.load(open(os.path.join(ROOT, detail)))
    out = []
    for r in sorted(rows, key=lambda r: -r["ms"]):
        s = ast.literal_eval(r["shape"])
        if "x3" in s and "direct" not in s:
            out.append((s, r["ms"]))
    picked = [s for s, _ in out[:top]]
    for want in ((51200, 1024, 256, 1, 1, "x3", "epi:res"),):  # the stage-3 expand with its residual, always
        if want not in picked:
            picked.append(want)
    if not any("wino" in s and s[0] % 36 == 0 for s in picked):  # a Winograd F(4×4) component batch, always
        picked += [s for s, _ in out if "wino" in s and s[0] % 36 == 0][:1]
    if DECODER_LINEAR not in picked:
        picked.append(DECODER_LINEAR)
    return picked


def gemm_runs(shape, dev):
    """{mode: launch} of one bucket on the same operands: x3 / x2 / bf16 (A rounded per fragment from fp32 rows, the
    same A traffic as the split modes). The x2 plan takes the x3 plan's tile (plan_conv), so the tile is the same."""
    m, cout, kdim, k, stride = shape[:5]
    wino = "wino" in shape
    epi = next((t for t in shape if isinstance(t, str) and t.startswith("epi:")), "epi:none")
    if wino:  # (36·T, Cout, Cin, 1, 1, mode, "wino", pixels): the batched component GEMM of F(4×4); run the whole conv
        pix, cin = shape[7], kdim
        n, h = 32, int(round((pix / 32) ** 0.5))
        assert n * h * h == pix and m % 36 == 0
        x = torch.randn(pix * cin, device=dev)
        wt = torch.randn(cout, 3, 3, cin, device=dev) / (9 * cin) ** 0.5
        u = ops.winograd_weights_host(wt.cpu().numpy(), 4)
        y = torch.empty(pix * cout, device=dev)
        work = torch.empty(ops.wino_work_elems(4, m // 36, cin, cout), device=dev)
        planes = {"x3": torch.from_numpy(ops.split_bf16x3_host(u)).to(dev),
                  "x2": torch.from_numpy(ops.split_bf16x2_host(u)).to(dev),
                  "bf16": torch.from_numpy(ops.bf16_bits(u).reshape(1, -1).view(np.int16)).to(dev)}
        wk = wt.reshape(cout, -1)
        return {mode: (lambda p=p: ops.conv2d(V(x, 0, cin), n, h, h, cin, wk, cout, 3, 1, 1, V(y, 0, cout),
                                              wino=(p, work, 4))) for mode, p in planes.items()}, 2 * m * cout * cin
    cin = kdim // (k * k)
    # rows as an n × h × w map whose output has m rows: 1×1 → one row of m pixels; 3×3 → bs32 square maps
    if k == 1:
        n, h, w = 1, 1, m
    else:
        ho = int(round((m / 32) ** 0.5))
        assert 32 * ho * ho == m
        n, h, w = 32, ho * stride, ho * stride
    x = torch.randn(n * h * w * cin, device=dev)
    wt = torch.randn(cout, kdim, device=dev) / kdim ** 0.5
    y = torch.empty(m * cout, device=dev)
    kw = {}
    if epi in ("epi:res", "epi:bn"):
        kw.update(scale=torch.rand(cout, device=dev) + 0.5, shift=torch.randn(cout, device=dev), act="relu")
    if epi == "epi:res":
        kw["res1"] = V(torch.randn(m * cout, device=dev), 0, cout)
    wq = {"x3": {"wt_planes": ops.split_bf16x3(wt)}, "x2": {"wt_planes": ops.split_bf16x2(wt)},
          "bf16": {"wt16": torch.from_numpy(ops.bf16_bits(wt.cpu().numpy()).view(np.int16)).to(dev)}}
    return {mode: (lambda q=q: ops.conv2d(V(x, 0, cin), n, h, w, cin, wt, cout, k, stride, k // 2, V(y, 0, cout),
                                          **kw, **q)) for mode, q in wq.items()}, 2 * m * cout * kdim


def cmd_layers(a, dev):
    rows = []
    for shape in buckets(a.detail, a.top):
        runs, flops = gemm_runs(shape, dev)
        t = {key: [] for key in runs}
        for _ in range(a.rounds):
            for key, r in runs.items():
                r()
                torch.cuda.synchronize()
                t[key].append(round(timed(r, a.reps), 4))
        med = {key: statistics.median(v) for key, v in t.items()}
        spread = max(t["x3"]) - min(t["x3"])
        d = {"shape": list(shape), "ms": t, "median_ms": med, "x3_spread_ms": round(spread, 4),
             "x2_over_x3": round(med["x3"] / med["x2"], 3), "bf16_over_x3": round(med["x3"] / med["bf16"], 3),
             "tflops": {key: round(flops / (v * 1e-3) / 1e12, 1) for key, v in med.items()},
             "x2_faster_every_round_beyond_spread": all(n < o for n, o in zip(t["x2"], t["x3"]))
             and med["x3"] - med["x2"] > spread}
        print(json.dumps(d), flush=True)
        rows.append(d)
    return rows


def cmd_e2e(a, dev):
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRESETS

    modes = ("fp32", "fp32-x2", "bf16")
    px = torch.randn(32, 3, 640, 640, device=dev)
    eng = {}
    for p in modes:
        eng[p] = SpotterForObjectDetection(PRESETS["r101vd"], use_graphs=False, precision=p).engine
        with torch.no_grad():
            eng[p].forward(px)  # workspaces, first-launch costs
        torch.cuda.synchronize()
    t = {p: [] for p in modes}
    for _ in range(a.rounds):
        for p in modes:
            with torch.no_grad():
                eng[p].forward(px)
                torch.cuda.synchronize()
                t[p].append(round(timed(lambda: eng[p].forward(px), a.steps), 3))
    med = {p: statistics.median(v) for p, v in t.items()}
    spread = max(t["fp32"]) - min(t["fp32"])
    d = {"workload": "Engine.forward bs32 640x640 r101vd, eager, one stream", "ms_per_step": t, "median_ms": med,
         "img_per_s": {p: round(32e3 / v, 1) for p, v in med.items()}, "fp32_spread_ms": round(spread, 3),
         "x2_over_fp32": round(med["fp32"] / med["fp32-x2"], 3), "bf16_over_fp32": round(med["fp32"] / med["bf16"], 3),
         "x2_faster_every_pair_beyond_spread": all(n < o for n, o in zip(t["fp32-x2"], t["fp32"]))
         and med["fp32"] - med["fp32-x2"] > spread}
    print(json.dumps(d), flush=True)
    return d


def cmd_expand(a, dev):
    runs, flops = gemm_runs((51200, 1024, 256, 1, 1, "x3", "epi:res"), dev)
    run = runs[a.mode]
    run()
    torch.cuda.synchronize()
    ms = timed(run, a.reps)
    d = {"shape": [51200, 1024, 256], "mode": a.mode, "ms": round(ms, 4), "tflops": round(flops / (ms * 1e-3) / 1e12, 1)}
    print(json.dumps(d), flush=True)
    return d


def cmd_accuracy(a, dev):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bf16_delta import delta

    d = {p: delta(p, precision="fp32-x2", reps=a.reps) for p in ("r18vd", "r101vd")}
    d["precision"] = "fp32-x2"
    d["metric"] = "fp32-x2 delta vs HF fp32 goldens (synthetic weights), batch of %d" % (4 * a.reps)
    print(json.dumps(d), flush=True)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cmd", choices=["layers", "e2e", "expand", "accuracy"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--top", type=int, default=6)
    ap.add_argument("--mode", default="x2", choices=["x3", "x2", "bf16"])
    ap.add_argument("--detail", default="profiles/r5/x3/conv_detail_c2_r5c.json")
    a = ap.parse_args()
    a.rounds = a.rounds or (3 if a.cmd == "e2e" else 5)
    a.reps = a.reps or {"layers": 10, "expand": 20, "accuracy": 1, "e2e": 1}[a.cmd]
    dev = torch.device("cuda", 0)
    res = {"layers": cmd_layers, "e2e": cmd_e2e, "expand": cmd_expand, "accuracy": cmd_accuracy}[a.cmd](a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
