"""A/B of the JPEG entropy decode: JpegDecoder(entropy="host") against entropy="gpu" in one process, alternating,
per file kind. Baseline re-encodes of the reference fixture at 1200x717 (4:2:0 and 4:4:4, q75), a
640² q75 frame and a 2160x3840 q90 frame. Per kind and mode: decode() p50 / p95 in ms (call to return: the call
ends with the status readback, so the kernels are inside), host CPU time per image (time.thread_time; the call ends
in an event wait that spins, so it equals the wall time), the host's own work timed apart from that wait —
sp_jpeg_entropy_pack against sp_jpeg_decode_coefs, each into a reused buffer — and bytes copied host to device. One
JSON line per kind to stdout and to --out.

    python tools/jpeg_entropy_ab.py [--iters 100] [--out profiles/jpeg_entropy/ab.jsonl]

Kernel times come from a profiler run of their own over the same files, GPU entropy path only:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o ent -- \
        python tools/jpeg_entropy_ab.py --kernels-only --iters 20
    python tools/jpeg_entropy_ab.py --trace <dir>/.../ent_kernel_trace.csv   (mean µs per kernel and grid size)
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


def files():
    import numpy as np
    from PIL import Image

    from spotter_amd.synthetic import synthetic_image

    def enc(img, **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        return b.getvalue()

    pic = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_pic.jpg")).convert("RGB"))
    return [("fixture 1200x717 4:2:0 q75", enc(pic, quality=75, subsampling=2)),
            ("fixture 1200x717 4:4:4 q75", enc(pic, quality=75, subsampling=0)),
            ("synthetic 640x640 4:2:0 q75", enc(synthetic_image(1, 640, 640), quality=75)),
            ("synthetic 2160x3840 4:2:0 q90", enc(synthetic_image(5, 2160, 3840), quality=90))]


def host_work(data, iters):
    """p50 ms of the two modes' host halves alone: the scan pack, and the host entropy decode."""
    import ctypes as C

    import numpy as np

    from spotter_amd._lib import SpJpegLayout, SpJpegScan, lib
    L = lib()
    lay, scan = SpJpegLayout(), SpJpegScan()
    L.sp_jpeg_entropy_pack(data, len(data), C.byref(lay), C.byref(scan), None, 0)  # the size to bring
    pkg = np.empty(scan.pkg_bytes, dtype=np.uint8)
    co = np.empty(lay.total_blocks * 64, dtype=np.int16)
    t = {"pack": [], "decode_coefs": []}
    for _ in range(iters):
        t0 = time.perf_counter()
        rc = L.sp_jpeg_entropy_pack(data, len(data), C.byref(lay), C.byref(scan), pkg.ctypes.data, pkg.size)
        t1 = time.perf_counter()
        rc |= L.sp_jpeg_decode_coefs(data, len(data), C.byref(lay), None, 0)
        rc |= L.sp_jpeg_decode_coefs(data, len(data), C.byref(lay), co.ctypes.data, co.size)
        t2 = time.perf_counter()
        assert rc == 0
        t["pack"].append((t1 - t0) * 1e3)
        t["decode_coefs"].append((t2 - t1) * 1e3)
    return {k: round(float(np.percentile(v, 50)), 4) for k, v in t.items()}


def summarise_trace(path):
    """Mean duration per (kernel, grid size) of a rocprofv3 kernel trace: the grid size tells the file kinds apart
    (subsequences for the entropy kernels, blocks and pixels for sp_jpeg_to_rgb's)."""
    import csv
    import re

    acc = {}
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            m = re.search(r"(ent_\w+|jpeg_\w+_kernel)", r["Kernel_Name"])
            if not m:
                continue
            key = (m.group(1), int(r["Grid_Size_X"]))
            acc.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (name, grid), v in sorted(acc.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        v = sorted(v)
        print(json.dumps({"kernel": name, "grid_threads": grid, "calls": len(v),
                          "mean_us": round(sum(v) / len(v), 2), "p50_us": round(v[len(v) // 2], 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true", help="GPU entropy path only, for a kernel trace")
    ap.add_argument("--trace", default=None, help="summarise this kernel trace CSV instead of measuring")
    a = ap.parse_args()
    if a.trace:
        return summarise_trace(a.trace)

    import numpy as np
    import torch

    from spotter_amd._lib import lib
    from spotter_amd.jpeg import JpegDecoder, decode_coefs

    assert lib().sp_device_init(0) == 0
    dev = torch.device("cuda", 0)
    decs = {"gpu": JpegDecoder(dev, entropy="gpu")}
    if not a.kernels_only:
        decs["host"] = JpegDecoder(dev)
    lines = []
    for name, data in files():
        lay, _ = decode_coefs(data)
        outs = {m: d.decode(data) for m, d in decs.items()}  # warm-up: buffers grown, code loaded
        if "host" in outs:
            assert torch.equal(outs["gpu"], outs["host"]), name
        assert decs["gpu"].stats["fallback"] == {}, (name, decs["gpu"].stats)
        wall = {m: [] for m in decs}
        cpu = {m: [] for m in decs}
        h2d0 = decs["gpu"].stats["h2d_bytes"]
        for _ in range(a.iters):
            for m, d in decs.items():  # alternating: both modes see the same clocks and the same neighbours
                c0, t0 = time.thread_time(), time.perf_counter()
                d.decode(data, out=outs[m])
                wall[m].append((time.perf_counter() - t0) * 1e3)
                cpu[m].append((time.thread_time() - c0) * 1e3)
        h2d = {"gpu": (decs["gpu"].stats["h2d_bytes"] - h2d0) // a.iters, "host": int(lay.total_blocks) * 128}
        rec = {"file": name, "jpeg_bytes": len(data), "width": lay.width, "height": lay.height, "iters": a.iters}
        for m in decs:
            rec[m] = {"decode_p50_ms": round(float(np.percentile(wall[m], 50)), 4),
                      "decode_p95_ms": round(float(np.percentile(wall[m], 95)), 4),
                      "host_cpu_ms_per_image": round(float(np.mean(cpu[m])), 4), "h2d_bytes": int(h2d[m])}
        rec["host_work_p50_ms"] = host_work(data, a.iters)
        rec["gpu_path_counts"] = {k: v for k, v in decs["gpu"].stats.items() if k != "h2d_bytes"}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
