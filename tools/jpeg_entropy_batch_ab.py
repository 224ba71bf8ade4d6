"""A/B of the batched GPU entropy decode: JpegDecoder(entropy="gpu") against entropy="host" in
decode_many and in the bulk pipeline, every comparison alternating inside one process so all legs see the same box,
clocks and neighbours. The file kinds are tools/bulk_ab.py's.

    python tools/jpeg_entropy_batch_ab.py decode   [--pairs 20] [--out profiles/jpeg_entropy_batch/decode.jsonl]
    python tools/jpeg_entropy_batch_ab.py pipeline [--preset r101vd] [--precision fp32] [--images 128] [--rounds 3]
                                                   [--out profiles/jpeg_entropy_batch/pipeline.jsonl]

decode: decode_many on 32 files per kind, four legs: the GPU chain and the host pool, each with the default pool
(packing, or the Huffman decode, in up to 16 threads) and with one worker. Images/s as median (min-max) over the pairs,
bytes copied host to device per image, and the host's own work per chunk timed apart from the event wait, on one
thread: header parse + sp_jpeg_entropy_pack of the 32 files against header parse + sp_jpeg_decode_coefs.

pipeline: BulkDetector.detect with a gpu / host decoder at decode_workers 16 and 1, in alternating segments: images/s
and stage A's / stage B's busy time per chunk.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bulk_ab import _emit, _stat, kinds  # noqa: E402


def host_seconds(files, iters=5):
    """Median seconds one thread spends on a chunk's host work, per mode (no device call)."""
    import numpy as np

    from spotter_amd._lib import SpJpegLayout, SpJpegScan, lib

    L = lib()
    lay, scan = SpJpegLayout(), SpJpegScan()
    cap = max(len(d) for d in files) + (1 << 20)
    pkg = np.empty(cap, dtype=np.uint8)
    assert L.sp_jpeg_decode_coefs(files[0], len(files[0]), C.byref(lay), None, 0) == 0
    co = np.empty(lay.total_blocks * 64, dtype=np.int16)
    t = {"gpu": [], "host": []}
    for _ in range(iters):
        t0 = time.perf_counter()
        for d in files:
            rc = L.sp_jpeg_decode_coefs(d, len(d), C.byref(lay), None, 0)
            rc |= L.sp_jpeg_entropy_pack(d, len(d), C.byref(lay), C.byref(scan), pkg.ctypes.data, pkg.size)
            assert rc == 0
        t1 = time.perf_counter()
        for d in files:
            rc = L.sp_jpeg_decode_coefs(d, len(d), C.byref(lay), None, 0)
            rc |= L.sp_jpeg_decode_coefs(d, len(d), C.byref(lay), co.ctypes.data, co.size)
            assert rc == 0
        t2 = time.perf_counter()
        t["gpu"].append(t1 - t0)
        t["host"].append(t2 - t1)
    return {k: float(np.median(v)) for k, v in t.items()}


def run_decode(a, dev):
    import torch

    from spotter_amd.jpeg import JpegDecoder, default_decode_workers

    lines = []
    for name, files in kinds().items():
        decs = {k: JpegDecoder(dev, entropy=k.split("_")[0]) for k in ("gpu_pool", "host_pool", "gpu_1", "host_1")}
        legs = {k: (lambda d=d, w=(1 if k.endswith("_1") else None): d.decode_many(files, max_workers=w))
                for k, d in decs.items()}
        outs = {k: f() for k, f in legs.items()}  # warm-up: buffers grown, pools started, code loaded
        for k in legs:
            assert all(torch.equal(x, y) for x, y in zip(outs[k], outs["host_pool"])), (name, k)
        del outs
        rates = {k: [] for k in legs}
        h0 = {k: d.batch_stats["h2d_bytes"] for k, d in decs.items()}
        g0 = decs["gpu_pool"].batch_stats["gpu"]
        for _ in range(a.pairs):
            for k, f in legs.items():  # alternating
                t0 = time.perf_counter()
                f()
                rates[k].append(len(files) / (time.perf_counter() - t0))
        hs = host_seconds(files)
        rec = {"files": name, "n": len(files), "jpeg_bytes": len(files[0]), "pairs": a.pairs,
               "workers": default_decode_workers(), "images_per_s": {k: _stat(v) for k, v in rates.items()},
               "h2d_bytes_per_image": {k: (d.batch_stats["h2d_bytes"] - h0[k]) // (a.pairs * len(files))
                                       for k, d in decs.items() if k.endswith("_pool")},
               "host_thread_ms_per_chunk": {k: round(1e3 * v, 2) for k, v in hs.items()},
               "gpu_path_images": (decs["gpu_pool"].batch_stats["gpu"] - g0) // a.pairs,
               "fallback": {str(k): v for k, v in decs["gpu_pool"].batch_stats["fallback"].items()}}
        med = {k: rec["images_per_s"][k]["median"] for k in legs}
        rec["gpu_over_host_pool"] = round(med["gpu_pool"] / med["host_pool"], 3)
        rec["gpu_over_host_1_worker"] = round(med["gpu_1"] / med["host_1"], 3)
        _emit(lines, rec)
    return lines


def run_pipeline(a, dev):
    import numpy as np
    import torch

    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.config import PRESETS
    from spotter_amd.jpeg import JpegDecoder, default_decode_workers

    model = SpotterForObjectDetection(PRESETS[a.preset], precision=a.precision)
    proc = SpotterImageProcessor()
    lines = []
    for name, files in kinds().items():
        if "4:4:4" in name:
            continue
        files = [files[i % len(files)] for i in range(a.images)]
        dets = {f"{m}_{w}": BulkDetector(model, proc, batch=a.batch, threshold=0.5, decode_workers=(1 if w == "1" else None),
                                        decoder=JpegDecoder(dev, entropy=m))
                for m in ("gpu", "host") for w in ("pool", "1")}
        for det in dets.values():  # warm-up: engine workspaces, graphs, pools, buffers
            assert sum(1 for _ in det.detect(files[:2 * a.batch])) == 2 * a.batch
        rates = {k: [] for k in dets}
        busy = {k: {"a": [], "b": []} for k in dets}
        for _ in range(a.rounds):
            for k, det in dets.items():  # alternating segments
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                n = sum(1 for _ in det.detect(files))
                rates[k].append(n / (time.perf_counter() - t0))
                for s in ("a", "b"):
                    busy[k][s] += det.stage_seconds[s]
        med = {k: _stat(v) for k, v in rates.items()}
        _emit(lines, {"files": name, "preset": a.preset, "precision": a.precision, "batch": a.batch,
                      "images": len(files), "rounds": a.rounds, "workers": default_decode_workers(),
                      "images_per_s": med,
                      "gpu_over_host_pool": round(med["gpu_pool"]["median"] / med["host_pool"]["median"], 3),
                      "gpu_over_host_1_worker": round(med["gpu_1"]["median"] / med["host_1"]["median"], 3),
                      "stage_busy_ms_per_chunk": {k: {s: round(1e3 * float(np.median(v)), 2) for s, v in b.items()}
                                                  for k, b in busy.items()}})
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("decode", "pipeline"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--images", type=int, default=128)
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
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
