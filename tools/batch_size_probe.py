"""Does the engine give one image the same scores at batch 1 and inside a batch of B? (No batcher involved.)

The fixture image is repeated B times and run eagerly per precision; for every B the number of scores above the
0.5 detection threshold, image 0's scores within 0.01 of it, and the largest |Δscore| among the top 60 scores
against batch 1 and between the images of the batch. Any batcher (spotter_amd/batching.py, shared_batch.py) hands
a caller rows computed at whatever B it rode in, so this is what its outputs can differ by from a bs1 call.

    python tools/batch_size_probe.py --out profiles/shared_batch/batch_size_probe.json
    python tools/batch_size_probe.py --batch-invariant 1 --out profiles/batch_invariant/batch_size_probe_inv1.json

With --batch-invariant P every |Δscore| is 0.0 and the counts agree at every B.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from PIL import Image

    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.config import PRESETS

    ap = argparse.ArgumentParser()
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--precision", nargs="+", default=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 2, 3, 4, 6, 8, 12])
    ap.add_argument("--batch-invariant", type=int, default=0, help="Engine(batch_invariant=P); 0 = off (the default mode)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    im = Image.open(os.path.join(ROOT, "tests", "golden", "test_pic.jpg")).convert("RGB")
    x = SpotterImageProcessor()(images=im)["pixel_values"]
    out = {}
    for prec in a.precision:
        m = SpotterForObjectDetection(PRESETS[a.preset], precision=prec, use_graphs=False,
                                      batch_invariant=a.batch_invariant or None)
        rows, base = {}, None
        for b in a.batch:
            with torch.no_grad():
                o = m(pixel_values=x.repeat(b, 1, 1, 1))
            s = torch.sigmoid(o.logits.float()).cpu().numpy()
            top = np.sort(s.reshape(b, -1), axis=1)[:, ::-1][:, :60]
            base = top[0] if base is None else base
            rows[b] = {"n_over_0.5": [int((t > 0.5).sum()) for t in top],
                       "near_threshold_scores_image0": [round(float(v), 5) for v in top[0][np.abs(top[0] - 0.5) < 0.01]],
                       "max_abs_dscore_vs_image0": float(np.abs(top - top[0]).max()),
                       "max_abs_dscore_vs_bs1": float(np.abs(top[0] - base).max())}
        out[prec] = rows
        print(prec, json.dumps(rows), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
