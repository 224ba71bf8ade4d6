"""A/B of the batched JPEG decode and of the bulk pipeline, every comparison alternating inside one
process so both sides see the same box, clocks and neighbours.

    python tools/bulk_ab.py decode   [--pairs 20] [--out profiles/bulk/decode.jsonl]
    python tools/bulk_ab.py pipeline [--preset r101vd] [--precision fp32] [--images 256] [--rounds 3]
                                     [--out profiles/bulk/pipeline.jsonl]

decode: JpegDecoder.decode_many on 32 files against 32 calls of decode(), per file kind (640² 4:2:0 q75 and the
1200x717 fixture re-encoded 4:2:0 / 4:4:4 q75, as tools/jpeg_entropy_ab.py builds them): images/s of the loop, of
decode_many with the default pool and with one worker, each the median over the pairs with their min / max, and the
bytes copied host to device per image.

pipeline: images/s of BulkDetector.detect over in-memory JPEGs against (a) the same images through the one-image
public calls (open_image → processor → model → post_process_object_detection) and (b) the engine step on a
resident uint8 batch of the same decoded images (preprocess → forward → post-process, the loop bench.py times,
restated here), in alternating segments; stage A's and stage B's busy time per chunk.
"""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kinds():
    import numpy as np
    from PIL import Image

    from spotter_amd.synthetic import synthetic_image

    def enc(img, **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        return b.getvalue()

    pic = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_pic.jpg")).convert("RGB"))
    return {"synthetic 640x640 4:2:0 q75": [enc(synthetic_image(100 + i, 640, 640), quality=75) for i in range(32)],
            "fixture 1200x717 4:2:0 q75": [enc(pic, quality=75, subsampling=2)] * 32,
            "fixture 1200x717 4:4:4 q75": [enc(pic, quality=75, subsampling=0)] * 32}


def _stat(rates):
    import numpy as np

    return {"median": round(float(np.median(rates)), 1), "min": round(float(min(rates)), 1),
            "max": round(float(max(rates)), 1)}


def _emit(lines, rec):
    lines.append(json.dumps(rec))
    print(lines[-1], flush=True)


def run_decode(a, dev):
    import torch

    from spotter_amd.jpeg import JpegDecoder, default_decode_workers

    lines = []
    for name, files in kinds().items():
        loop, many, one = JpegDecoder(dev), JpegDecoder(dev), JpegDecoder(dev)
        legs = {"loop_decode": lambda: [loop.decode(d) for d in files],
                "decode_many": lambda: many.decode_many(files),
                "decode_many_1_worker": lambda: one.decode_many(files, max_workers=1)}
        outs = {k: f() for k, f in legs.items()}  # warm-up: buffers grown, pool started, code loaded
        for k in ("decode_many", "decode_many_1_worker"):
            assert all(torch.equal(x, y) for x, y in zip(outs[k], outs["loop_decode"])), (name, k)
        del outs
        rates = {k: [] for k in legs}
        h0 = many.batch_stats["h2d_bytes"]
        for _ in range(a.pairs):
            for k, f in legs.items():  # alternating
                t0 = time.perf_counter()
                f()
                rates[k].append(len(files) / (time.perf_counter() - t0))
        rec = {"files": name, "n": len(files), "jpeg_bytes": len(files[0]), "pairs": a.pairs,
               "workers": default_decode_workers(), "images_per_s": {k: _stat(v) for k, v in rates.items()},
               "decode_many_ms_per_call": {k: round(1e3 * len(files) / _stat(rates[k])["median"], 3)
                                           for k in ("decode_many", "decode_many_1_worker")},
               "h2d_bytes_per_image": (many.batch_stats["h2d_bytes"] - h0) // (a.pairs * len(files))}
        rec["many_over_loop"] = round(rec["images_per_s"]["decode_many"]["median"]
                                      / rec["images_per_s"]["loop_decode"]["median"], 3)
        _emit(lines, rec)
    return lines


def run_pipeline(a, dev):
    import numpy as np
    import torch

    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor, ops
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.config import PRESETS
    from spotter_amd.jpeg import JpegDecoder, open_image

    cfg = PRESETS[a.preset]
    model = SpotterForObjectDetection(cfg, precision=a.precision)
    proc = SpotterImageProcessor()
    eng = model.engine
    B, S, K = a.batch, cfg.image_size, cfg.num_queries
    px = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    outs = (torch.empty((B, K), device=dev), torch.empty((B, K), dtype=torch.int64, device=dev),
            torch.empty((B, K, 4), device=dev), torch.empty((B,), dtype=torch.int32, device=dev),
            torch.empty((B, K), dtype=torch.int32, device=dev))
    lines = []
    for name, files in kinds().items():
        if "4:4:4" in name:
            continue
        files = [files[i % len(files)] for i in range(a.images)]
        det = BulkDetector(model, proc, batch=B, threshold=0.5)
        resident = [t.clone() for t in JpegDecoder(dev).decode_many(files[:B])]
        tsz = torch.tensor([list(t.shape[:2]) for t in resident], dtype=torch.int32, device=dev)

        def bulk():
            return sum(1 for _ in det.detect(files))

        def one_at_a_time():
            for d in files:
                im = open_image(d).convert("RGB")
                inputs = proc(images=im, return_tensors="pt")
                with torch.no_grad():
                    out = model(**inputs)
                proc.post_process_object_detection(out, threshold=0.5, target_sizes=[(im.size[1], im.size[0])])
            return len(files)

        def engine_step():
            for _ in range(len(files) // B):
                ops.preprocess_u8(resident, px, S, S)
                logits, pred = eng.forward(px)
                ops.postprocess(logits, pred, tsz, K, 0.5, *outs)
            torch.cuda.synchronize(dev)
            return len(files) // B * B

        legs = {"bulk": bulk, "one_at_a_time": one_at_a_time, "engine_resident": engine_step}
        for f in legs.values():  # warm-up: engine workspaces, graphs, pools, buffers
            f()
        rates = {k: [] for k in legs}
        busy = {"a": [], "b": []}
        for _ in range(a.rounds):
            for k, f in legs.items():  # alternating segments
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                n = f()
                rates[k].append(n / (time.perf_counter() - t0))
                if k == "bulk":
                    for s in busy:
                        busy[s] += det.stage_seconds[s]
        med = {k: _stat(v) for k, v in rates.items()}
        _emit(lines, {"files": name, "preset": a.preset, "precision": a.precision, "batch": B, "images": len(files),
                      "rounds": a.rounds, "images_per_s": med,
                      "bulk_over_one_at_a_time": round(med["bulk"]["median"] / med["one_at_a_time"]["median"], 3),
                      "bulk_over_engine_resident": round(med["bulk"]["median"] / med["engine_resident"]["median"], 3),
                      "stage_busy_ms_per_chunk": {s: round(1e3 * float(np.median(v)), 2) for s, v in busy.items()}})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("decode", "pipeline"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0
    dev = torch.device("cuda", 0)
    lines = run_decode(a, dev) if a.what == "decode" else run_pipeline(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
