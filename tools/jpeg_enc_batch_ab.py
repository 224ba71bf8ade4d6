"""A/B of the batched JPEG encode and of the labelled bulk pipeline, every comparison alternating
inside one process so all sides see the same box, clocks and neighbours.

    python tools/jpeg_enc_batch_ab.py encode [--pairs 20] [--calls 10] [--out profiles/jpeg_enc_batch/encode.jsonl]
    python tools/jpeg_enc_batch_ab.py bulk   [--preset r101vd] [--precisions fp32,bf16] [--images 256] [--rounds 3]
                                             [--threshold 0.5] [--out profiles/jpeg_enc_batch/bulk.jsonl]

encode: JpegEncoder.encode_many on 32 device-resident images against 32 calls of encode(), quality 75, 4:2:0, at
640x640 (synthetic) and 1200x717 (the fixture): images/s of each leg, the median over the pairs with their min / max
(a sample is `calls` calls, ended by the call's own last stream wait), bytes copied device to host and stream waits
per chunk. The files of both legs are compared byte for byte before anything is timed.

bulk: images/s of BulkDetector.detect over in-memory JPEGs, unlabelled, labelled through encode_many and labelled
through one encode() per image (an encoder stand-in that loops, patched in here), in alternating segments; the busy
time of stages A, B and C per chunk of each.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bulk_ab import _emit, _stat, kinds  # noqa: E402


def sources(dev):
    import numpy as np
    import torch
    from PIL import Image

    from spotter_amd.synthetic import synthetic_image

    pic = np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "test_pic.jpg")).convert("RGB"))
    rng = np.random.default_rng(0)
    # 32 different images of each size: the fixture with a little seeded noise, so that no two segments are equal
    pics = [np.clip(pic.astype(np.int16) + rng.integers(-3, 4, pic.shape), 0, 255).astype(np.uint8) for _ in range(32)]
    return {"synthetic 640x640": [torch.from_numpy(synthetic_image(100 + i, 640, 640)).to(dev) for i in range(32)],
            "fixture 1200x717": [torch.from_numpy(p).to(dev) for p in pics]}


def run_encode(a, dev):
    from spotter_amd.jpeg import JpegEncoder

    lines = []
    for name, srcs in sources(dev).items():
        loop, many = JpegEncoder(dev), JpegEncoder(dev)
        legs = {"loop_encode": lambda: [loop.encode(s, 75, 2) for s in srcs],
                "encode_many": lambda: many.encode_many(srcs, quality=75, subsampling=2)}
        outs = {k: f() for k, f in legs.items()}  # warm-up: buffers grown, code loaded
        assert outs["encode_many"] == outs["loop_encode"], name
        file_bytes = sum(len(x) for x in outs["encode_many"]) // len(srcs)
        del outs
        rates = {k: [] for k in legs}
        s0 = dict(many.stats)
        for _ in range(a.pairs):
            for k, f in legs.items():  # alternating
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    f()
                rates[k].append(a.calls * len(srcs) / (time.perf_counter() - t0))
        st = {k: many.stats[k] - s0[k] for k in s0}
        rec = {"images": name, "n": len(srcs), "quality": 75, "subsampling": "4:2:0", "file_bytes": file_bytes,
               "pairs": a.pairs, "calls_per_sample": a.calls,
               "images_per_s": {k: _stat(v) for k, v in rates.items()},
               "ms_per_32_images": {k: round(1e3 * len(srcs) / _stat(v)["median"], 3) for k, v in rates.items()},
               "encode_many_per_chunk": {"chunks": st["chunks"], "d2h_bytes": st["d2h_bytes"] // st["chunks"],
                                         "h2d_bytes": st["h2d_bytes"] // st["chunks"],
                                         "stream_waits": st["waits"] / st["chunks"]},
               "loop_encode_per_32_images": {"stream_waits": 2 * len(srcs)}}
        rec["many_over_loop"] = round(rec["images_per_s"]["encode_many"]["median"]
                                      / rec["images_per_s"]["loop_encode"]["median"], 3)
        _emit(lines, rec)
    return lines


class PerImageEncoder:
    """encode_many's surface over one encode() call per image: the bulk pipeline as it would be without the batch."""

    def __init__(self, enc):
        self.enc = enc

    def encode_many(self, srcs, quality=-1, subsampling=-1, comments=None, max_workers=None):
        from spotter_amd.jpeg import DeviceRGBImage

        out = []
        for s, c in zip(srcs, comments or [None] * len(srcs)):
            if isinstance(s, DeviceRGBImage):
                s = s.spotter_device_rgb
            out.append(self.enc.encode(s, quality, subsampling, c))
        return out


def run_bulk(a, dev):
    import numpy as np
    import torch

    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.config import PRESETS
    from spotter_amd.jpeg import JpegEncoder

    cfg = PRESETS[a.preset]
    proc = SpotterImageProcessor()
    lines = []
    for precision in a.precisions.split(","):
        model = SpotterForObjectDetection(cfg, precision=precision)
        id2label = model.config.id2label
        for name, files in kinds().items():
            if "4:4:4" in name:
                continue
            files = [files[i % len(files)] for i in range(a.images)]
            kw = {"batch": a.batch, "threshold": a.threshold}
            lab = dict(kw, labelled=True, id2label=id2label)
            dets = {"unlabelled": BulkDetector(model, proc, **kw),
                    "labelled_encode_many": BulkDetector(model, proc, encoder=JpegEncoder(dev), **lab),
                    "labelled_per_image": BulkDetector(model, proc, encoder=PerImageEncoder(JpegEncoder(dev)), **lab)}
            outs = {k: list(d.detect(files)) for k, d in dets.items()}  # warm-up: workspaces, graphs, pools, buffers
            assert [r["jpeg"] for r in outs["labelled_encode_many"]] == [r["jpeg"] for r in outs["labelled_per_image"]]
            drawn = sum(len(r["scores"]) for r in outs["unlabelled"]) / len(files)
            jpeg_bytes = sum(len(r["jpeg"]) for r in outs["labelled_encode_many"]) // len(files)
            del outs
            rates = {k: [] for k in dets}
            busy = {k: {"a": [], "b": [], "c": []} for k in dets}
            for _ in range(a.rounds):
                for k, d in dets.items():  # alternating segments
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    n = sum(1 for _ in d.detect(files))
                    rates[k].append(n / (time.perf_counter() - t0))
                    for s in busy[k]:
                        busy[k][s] += d.stage_seconds[s]
            med = {k: _stat(v) for k, v in rates.items()}
            _emit(lines, {"files": name, "preset": a.preset, "precision": precision, "batch": a.batch,
                          "threshold": a.threshold, "images": len(files), "rounds": a.rounds,
                          "detections_drawn_per_image": round(drawn, 2),
                          "labelled_jpeg_bytes": jpeg_bytes, "images_per_s": med,
                          "encode_many_over_per_image": round(med["labelled_encode_many"]["median"]
                                                              / med["labelled_per_image"]["median"], 3),
                          "labelled_over_unlabelled": round(med["labelled_encode_many"]["median"]
                                                            / med["unlabelled"]["median"], 3),
                          "stage_busy_ms_per_chunk": {k: {s: round(1e3 * float(np.median(v)), 2)
                                                          for s, v in b.items() if v} for k, b in busy.items()}})
        del model
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("encode", "bulk"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0
    dev = torch.device("cuda", 0)
    lines = run_encode(a, dev) if a.what == "encode" else run_bulk(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
