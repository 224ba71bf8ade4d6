"""What the batch-invariant mode costs: same box, same process, modes alternating (as tools/ab_x2.py).

    python tools/ab_batch_invariant.py e2e   --out profiles/batch_invariant/e2e.json
    python tools/ab_batch_invariant.py fold  --out profiles/batch_invariant/fold_launch.json

e2e: forward ms and images/s of one preset per precision at every B, for the default mode, batch_invariant=1 with
the folded split-K tile, the same without it (sp_set_tuning SP_TUNE_FOLD = 1: split launch + reduce) and
batch_invariant=P2. B <= 4 replays a captured graph, as the drop-in model does; larger batches run eagerly.
fold: the folded tile against split launch + reduce per launch, on the launches of a B-image forward that fold.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, iters):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def e2e(a):
    import numpy as np
    import torch

    from spotter_amd import ops
    from spotter_amd.config import PRESETS
    from spotter_amd.engine import Engine
    from spotter_amd.graph import GraphRunner
    from spotter_amd.weights import generate

    dev = torch.device("cuda", 0)
    cfg = PRESETS[a.preset]
    w = generate(cfg, seed=0)
    out = {"preset": a.preset, "size": a.size, "rounds": a.rounds, "points": []}
    for prec in a.precision:
        engines = {"default": Engine(cfg, w, dev, precision=prec),
                   "inv1": Engine(cfg, w, dev, precision=prec, batch_invariant=1),
                   f"inv{a.p2}": Engine(cfg, w, dev, precision=prec, batch_invariant=a.p2)}
        modes = [("default", "default", None), ("inv1_folded", "inv1", None), ("inv1_split", "inv1", 1),
                 (f"inv{a.p2}", f"inv{a.p2}", None)]
        for B in a.batch:
            x = torch.rand(B, 3, a.size, a.size, device=dev)
            runs = {}
            for name, ek, fold in modes:
                eng = engines[ek]
                ops.set_tuning(ops.TUNE_FOLD, fold)
                try:
                    if B <= 4:
                        g = GraphRunner(eng, B, a.size, a.size)  # captured under this mode's knob
                        runs[name] = (lambda g=g: g(x))
                    else:
                        runs[name] = (lambda eng=eng, fold=fold: (ops.set_tuning(ops.TUNE_FOLD, fold), eng.forward(x)))
                    with torch.no_grad():
                        for _ in range(3):
                            runs[name]()
                finally:
                    ops.set_tuning(ops.TUNE_FOLD, None)
            torch.cuda.synchronize()
            ms = {name: [] for name in runs}
            iters = max(3, min(50, int(400 / (B + 3))))
            with torch.no_grad():
                for _ in range(a.rounds):
                    for name in runs:  # alternating
                        ms[name].append(_time(runs[name], iters))
            ops.set_tuning(ops.TUNE_FOLD, None)
            pt = {"precision": prec, "batch": B, "iters": iters}
            for name, v in ms.items():
                med = float(np.median(v))
                pt[name] = {"ms": round(med, 4), "img_per_s": round(B / med * 1e3, 1), "min_ms": round(min(v), 4),
                            "max_ms": round(max(v), 4)}
            for name in ms:
                if name != "default":
                    pt[name]["vs_default"] = round(pt["default"]["ms"] / pt[name]["ms"], 4)
            print(json.dumps(pt), flush=True)
            out["points"].append(pt)
        del engines
        torch.cuda.empty_cache()
    return out


def fold(a):
    import numpy as np
    import torch

    from spotter_amd import ops
    from spotter_amd.ops import view

    dev = torch.device("cuda", 0)
    # (what, rows per image, K, Cout, k, h, w): the stage-3 1×1 reduce of R101vd at 640² (40² × 1024 → 256) and the
    # decoder's 300-row 1024 → 256 linear: 4-way splits for one image that a bs8 grid (800 / 152 tiles) would not split
    shapes = [("stage-3 1x1 reduce 40x40x1024->256", 40, 40, 1024, 256, 1), ("decoder linear 300x1024->256", 1, 300, 1024, 256, 1)]
    out = {"batch": a.fold_batch, "rounds": a.rounds, "launches": []}
    B = a.fold_batch
    rng = np.random.default_rng(0)
    for what, h, w, cin, cout, k in shapes:
        for mode in a.modes:
            rows = B * h * w
            x = torch.from_numpy(rng.standard_normal((rows * cin,)).astype(np.float32)).to(dev)
            wt = torch.from_numpy((rng.standard_normal((cout, k * k * cin)) / np.sqrt(cin * k * k)).astype(np.float32)).to(dev)
            kw = {"x3": {"wt_planes": ops.split_bf16x3(wt)}, "x2": {"wt_planes": ops.split_bf16x2(wt)},
                  "bf16": {"wt16": torch.from_numpy(ops.bf16_bits(wt.cpu().numpy()).view(np.int16)).to(dev)}}[mode]
            sc = torch.ones(cout, device=dev)
            o = torch.empty(rows * cout, device=dev)
            ws = torch.empty(16 * rows * cout, device=dev)
            ops.set_plan_batch(B, 1)
            args = (view(x, cin), B, h, w, cin, wt, cout, k, 1, k // 2, view(o, cout))
            plan = ops.conv_plan(ops.conv_desc(*args, scale=sc, shift=sc, act="relu", workspace=ws, **kw)[0])

            def run(f):
                ops.set_tuning(ops.TUNE_FOLD, f)
                ops.conv2d(*args, scale=sc, shift=sc, act="relu", workspace=ws, **kw)

            res = {}
            for name, f in (("folded", None), ("split_reduce", 1)):
                run(f)
                res[name] = o.clone()
            assert torch.equal(res["folded"].view(torch.int32), res["split_reduce"].view(torch.int32))
            ms = {"folded": [], "split_reduce": []}
            for _ in range(a.rounds):
                for name, f in (("folded", None), ("split_reduce", 1)):
                    ms[name].append(_time(lambda f=f: run(f), 200))
            ops.set_tuning(ops.TUNE_FOLD, None)
            ops.set_plan_batch(0, 0)
            r = {"what": what, "mode": mode, "rows": rows, "splits": plan["splits"],
                 "folded_us": round(float(np.median(ms["folded"])) * 1e3, 2),
                 "split_reduce_us": round(float(np.median(ms["split_reduce"])) * 1e3, 2),
                 # bytes the split form moves through the workspace and the folded form does not: the slabs written
                 # by the split launch and read by the reduce (an upper bound on the HBM traffic saved: L2 may hold some)
                 "workspace_bytes_avoided": 2 * plan["splits"] * rows * cout * 4}
            r["speedup"] = round(r["split_reduce_us"] / r["folded_us"], 3)
            print(json.dumps(r), flush=True)
            out["launches"].append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["e2e", "fold"])
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32])
    ap.add_argument("--p2", type=int, default=4, help="the second plan batch measured")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fold-batch", type=int, default=8)
    ap.add_argument("--modes", nargs="+", default=["x3", "bf16"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = e2e(a) if a.what == "e2e" else fold(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
