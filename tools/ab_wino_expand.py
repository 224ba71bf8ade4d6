"""A/B per launch: a bottleneck's conv2 output transform + expand as today's pair (sp_winograd_f43_output, then the
expand's planned sp_conv2d) against the fused kernel (sp_winograd_f43_expand), at the map sizes of C2 (bs32 of 640²)
and C5 (bs8 of 1280²). Every shape runs in a fresh child process; in it the rounds interleave old, control (the old
pair again) and new, following tools/ab_direct_x3.py: per shape the timings of each side, their medians, the old
pair's spread (max - min of its own timings), and the adoption rule: the fused launch faster than the pair in every
round and the median gain larger than that spread. M is filled once by the real input and gemm stages.
python tools/ab_wino_expand.py [--out f.json] [--rounds 5] [--reps 10] [--only k256|k128]
       [--shape N H W K COUT ...]   (other maps, e.g. for the engine's pixel gate)"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# n, h, w, K (conv2 Cin = Cout = K), expand Cout
SHAPES = {"k256": [(32, 40, 40, 256, 1024), (8, 80, 80, 256, 1024)],
          "k128": [(32, 80, 80, 128, 512), (8, 160, 160, 128, 512)]}


def timed(run, reps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def child(shape, rounds, reps):
    import numpy as np
    import torch

    from spotter_amd import ops
    from spotter_amd._lib import lib
    from spotter_amd.ops import view

    assert lib().sp_device_init(0) == 0
    dev = torch.device("cuda", 0)
    n, h, w, k, cout = shape
    m = n * h * w
    rng = np.random.default_rng(0)
    dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    x = torch.randn(m * k, device=dev)
    w2 = (rng.standard_normal((k, 3, 3, k)) / np.sqrt(9 * k)).astype(np.float32)
    we = dv((rng.standard_normal((cout, k)) / np.sqrt(k)).astype(np.float32))
    sc2, sh2 = torch.rand(k, device=dev) + 0.5, torch.randn(k, device=dev)
    sce, she = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
    wino = dv(ops.split_bf16x3_host(ops.winograd_weights_host(w2, 4)))
    planes = ops.split_bf16x3(we)
    frag = ops.pack_expand_frag(planes, cout, k)
    tiles = n * ((h + 3) // 4) * ((w + 3) // 4)
    work = torch.empty(ops.wino_work_elems(4, tiles, k, k), device=dev)
    t2 = torch.empty(m * k, device=dev)
    res = torch.randn(m * cout, device=dev)
    outs = {key: torch.empty(m * cout, device=dev) for key in ("old", "new")}
    d2, _ = ops.conv_desc(view(x, k), n, h, w, k, dv(w2.reshape(k, -1)), k, 3, 1, 1, view(t2, k), scale=sc2, shift=sh2,
                          act="relu")
    stages = ops.wino_desc(d2, (wino, work, 4))
    ops.wino_launch(stages, only="input")
    ops.wino_launch(stages, only="gemm")
    de = {key: ops.conv_desc(view(t2, k), n, h, w, k, we, cout, 1, 1, 0, view(o, cout), scale=sce, shift=she,
                             act="relu", res1=view(res, cout), wt_planes=planes) for key, o in outs.items()}
    plan = ops.wino_expand_plan(d2, work.numel(), de["new"][0], True, 0)
    if not plan["fused"]:  # the expand's own plan at this size is no tile the fused kernel replaces
        print("AB " + json.dumps({"shape": list(shape), "expand_plan": plan["expand"], "fused": 0}), flush=True)
        return

    def old():
        ops.wino_launch(stages, only="output")
        ops.conv_launch(*de["old"])

    def new():
        assert ops.wino_expand(stages, d2, work, de["new"][0], de["new"][1], frag, 0)

    runs = {"old": old, "ctl": old, "new": new}
    t = {key: [] for key in runs}
    for _ in range(rounds):
        for key, r in runs.items():
            r()
            torch.cuda.synchronize()
            t[key].append(round(timed(r, reps), 4))
    equal = bool(torch.equal(outs["old"], outs["new"]))
    med = {key: statistics.median(v) for key, v in t.items()}
    spread = max(t["old"]) - min(t["old"])
    d = {"shape": list(shape), "expand_plan": plan["expand"], "fused": plan["fused"], "units": plan["units"],
         "bit_identical": equal, "ms": t, "median_ms": med, "old_spread_ms": round(spread, 4),
         "ctl_vs_old_ms": round(med["old"] - med["ctl"], 4), "gain_ms": round(med["old"] - med["new"], 4),
         "speedup": round(med["old"] / med["new"], 3),
         "tflops": {key: round(2 * m * cout * k / (v * 1e-3) / 1e12, 1) for key, v in med.items()},
         "adopt": equal and all(nw < od for nw, od in zip(t["new"], t["old"])) and med["old"] - med["new"] > spread}
    print("AB " + json.dumps(d), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=sorted(SHAPES))
    ap.add_argument("--shape", type=int, nargs=5, action="append", metavar=("N", "H", "W", "K", "COUT"),
                    help="run these maps instead of the C2 / C5 ones (repeatable)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(tuple(json.loads(a.child)), a.rounds, a.reps)
    rows = []
    groups = {"given": [tuple(sh) for sh in a.shape]} if a.shape else SHAPES
    for key in sorted(groups, reverse=True):
        if a.only and not a.shape and a.only != key:
            continue
        for shape in groups[key]:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(shape), "--rounds",
                                str(a.rounds), "--reps", str(a.reps)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit(f"child for {shape} exited with {r.returncode}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB ")][-1][3:]
            print(line, flush=True)
            rows.append(json.loads(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
