"""A/B in one process: the fp32 path's thin 3×3 convs as the direct split-MFMA kernels (sp_conv3x3_c32_x3,
sp_conv3x3_c64_x3) vs today's paths (sp_conv3x3_c32 for the stem convs, the x3 implicit GEMM for the stage-0 3×3)
at the C2 (bs32 of 640²) and C5 (bs8 of 1280²) map sizes. Interleaved rounds; per shape the five timings of each
side, their medians, and the adoption rule: the new kernel faster in every round and the median gain larger than
the spread of the old path's own timings. python tools/ab_direct_x3.py [--out f.json] [--rounds 5] [--only c64]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from spotter_amd import ops
from spotter_amd.ops import V


def timed(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=None, choices=["c32-32", "c32-64", "c64"], help="one kernel (counter runs)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows = []
    for cin, cout in ((32, 32), (32, 64), (64, 64)):
        if a.only and a.only != ("c64" if cin == 64 else f"c32-{cout}"):
            continue
        for n, hw in ((32, 320), (8, 640)) if cin == 32 else ((32, 160), (8, 320)):
            h = w = hw
            m = n * h * w
            k = 9 * cin
            ldy = 128 if cin == 64 else cout  # the stage-0 output is a slice of the fused tail's concat rows
            sc, sh = torch.rand(cout, device=dev) + 0.5, torch.randn(cout, device=dev)
            xf = torch.randn(m * cin, device=dev)
            wf = torch.randn(cout, k, device=dev) / k ** 0.5
            planes = ops.split_bf16x3(wf)
            yf = torch.empty(m * ldy, device=dev)
            xv, yv = V(xf, 0, cin), V(yf, 0, ldy)
            if cin == 32:
                runs = {
                    "old": lambda: ops.conv3x3_c32(xv, wf, sc, sh, yv, n, h, w, cout, act="relu"),
                    "new": lambda: ops.conv3x3_c32_x3(xv, planes, sc, sh, yv, n, h, w, cout, act="relu"),
                }
            else:
                runs = {
                    "old": lambda: ops.conv2d(xv, n, h, w, 64, wf, 64, 3, 1, 1, yv, scale=sc, shift=sh, act="relu",
                                              wt_planes=planes),
                    "new": lambda: ops.conv3x3_c64_x3(xv, planes, sc, sh, yv, n, h, w, act="relu"),
                }
            t = {key: [] for key in runs}
            for _ in range(a.rounds):
                for key, r in runs.items():
                    r()
                    torch.cuda.synchronize()
                    t[key].append(round(timed(r, a.reps), 4))
            med = {key: statistics.median(v) for key, v in t.items()}
            spread = max(t["old"]) - min(t["old"])
            d = {"shape": [n, h, w, cin, cout], "old": "sp_conv3x3_c32" if cin == 32 else "x3 implicit GEMM",
                 "ms": t, "median_ms": med, "old_spread_ms": round(spread, 4),
                 "speedup": round(med["old"] / med["new"], 3),
                 "tflops": {key: round(2 * m * cout * k / (v * 1e-3) / 1e12, 1) for key, v in med.items()},
                 "adopt": all(nw < od for nw, od in zip(t["new"], t["old"])) and med["old"] - med["new"] > spread}
            print(json.dumps(d), flush=True)
            rows.append(d)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
