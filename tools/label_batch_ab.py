"""A/B of the batched label draw and of the overlapped stage C of the labelled bulk pipeline, every
comparison alternating inside one process so all sides see the same box, clocks and neighbours.

    python tools/label_batch_ab.py bulk   [--preset r101vd] [--precisions fp32,bf16] [--images 256] [--rounds 5]
                                          [--threshold 0.5] [--out profiles/label_batch/bulk.jsonl]
    python tools/label_batch_ab.py flush  [--pairs 20] [--calls 10] [--out profiles/label_batch/flush.jsonl]
    python tools/label_batch_ab.py record [--pairs 20] [--out profiles/label_batch/record.jsonl]

bulk: images/s of BulkDetector.detect(labelled=True) over in-memory JPEGs in three legs, in alternating segments:
(a) label_draw="pillow", label_overlap=False: the Draw loop and one sp_draw_rgb launch per image, stage C at the end
of stage B (the pipeline before §5.28); (b) label_draw="batched", not overlapped; (c) batched and overlapped. The files
of the three legs are compared byte for byte before anything is timed. Also the busy time of stages A, B and C per
chunk of each leg.

flush: flush_many over the recorded labels of 32 device images against 32 flush() calls (a sample is `calls` rounds,
each ended by a stream wait; recording the lists is outside the clock).

record: host time per 32-image chunk of record_labels against the drop-in's Draw loop on the same boxes and texts
(nothing is flushed: the lists are compared and dropped).
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

LEGS = {"a_pillow_inline": {"label_draw": "pillow", "label_overlap": False},
        "b_batched_inline": {"label_draw": "batched", "label_overlap": False},
        "c_batched_overlapped": {"label_draw": "batched", "label_overlap": True}}


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
            dets = {k: BulkDetector(model, proc, batch=a.batch, threshold=a.threshold, labelled=True,
                                    id2label=id2label, encoder=JpegEncoder(dev), **kw) for k, kw in LEGS.items()}
            # warm-up, twice: workspaces, graphs, pools, buffers, and the stamps of the strings the run draws
            outs = {k: [list(d.detect(files)) for _ in range(2)][-1] for k, d in dets.items()}
            for k in dets:
                assert [r["jpeg"] for r in outs[k]] == [r["jpeg"] for r in outs["a_pillow_inline"]], k
            drawn = sum(len(r["scores"]) for r in outs["a_pillow_inline"]) / len(files)
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
                          "detections_drawn_per_image": round(drawn, 2), "images_per_s": med,
                          "b_over_a": round(med["b_batched_inline"]["median"] / med["a_pillow_inline"]["median"], 3),
                          "c_over_a": round(med["c_batched_overlapped"]["median"]
                                            / med["a_pillow_inline"]["median"], 3),
                          "stage_busy_ms_per_chunk": {k: {s: round(1e3 * float(np.median(v)), 2)
                                                          for s, v in b.items() if v} for k, b in busy.items()}})
        del model
    return lines


def _chunk_labels(seed, n_images=32, w=640, h=640, per_image=(25, 41)):
    """Boxes and amenity strings for a chunk: 25-40 detections an image, inside the image, as a threshold-0.5 run of
    the synthetic weights draws them."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_draw import AMENITY_TEXTS

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_images):
        boxes, texts = [], []
        for _ in range(int(rng.integers(*per_image))):
            x0, y0 = rng.uniform(0, 0.8 * w), rng.uniform(0, 0.8 * h)
            boxes.append([float(x0), float(y0), float(x0 + rng.uniform(10, 0.2 * w)),
                          float(y0 + rng.uniform(10, 0.2 * h))])
            texts.append(str(rng.choice(AMENITY_TEXTS)))
        out.append((boxes, texts))
    return out


def _draw_loop(image, boxes, texts):
    from spotter_amd.draw import draw_module

    draw = draw_module().Draw(image)
    for box, text in zip(boxes, texts):
        draw.rectangle(box, outline="red", width=3)
        draw.text(xy=(box[0] + 5, box[1] + 5), text=text, fill="white", stroke_width=1, stroke_fill="black")


def run_flush(a, dev):
    import torch

    from spotter_amd.draw import record_labels
    from spotter_amd.jpeg import DeviceRGBImage, _draw_stage, flush_many
    from spotter_amd.synthetic import synthetic_image

    lines = []
    for w, h in ((640, 640), (1200, 717)):
        labels = _chunk_labels(7, w=w, h=h)
        base = [torch.from_numpy(synthetic_image(100 + i, h, w)).to(dev) for i in range(len(labels))]

        def recorded():
            ims = [DeviceRGBImage(t) for t in base]  # drawn over and over in place: only the time is looked at
            for im, (boxes, texts) in zip(ims, labels):
                record_labels(im, boxes, texts)
            return ims

        def loop(ims):
            for im in ims:
                im.flush()

        legs = {"loop_flush": loop, "flush_many": flush_many}
        start, drawn = [t.clone() for t in base], {}
        for k, f in legs.items():  # warm-up, and both legs give the same pixels from the same start
            for t, s in zip(base, start):
                t.copy_(s)
            f(recorded())
            drawn[k] = [t.clone() for t in base]
        assert all(torch.equal(x, y) for x, y in zip(drawn["loop_flush"], drawn["flush_many"]))
        del start, drawn
        ms = {k: [] for k in legs}
        st0 = dict(_draw_stage(dev).stats)
        for _ in range(a.pairs):
            for k, f in legs.items():  # alternating
                sets = [recorded() for _ in range(a.calls)]
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for ims in sets:
                    f(ims)
                    torch.cuda.current_stream(dev).synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0) / a.calls)
        st = {k: _draw_stage(dev).stats[k] - st0[k] for k in st0}
        rec = {"images": f"{w}x{h}", "n": len(labels),
               "labels_per_image": round(sum(len(b) for b, _ in labels) / len(labels), 1), "pairs": a.pairs, "calls_per_sample": a.calls, "ms_per_32_images": {k: _stat(v) for k, v in ms.items()},
               "flush_many_per_call": {k: round(v / st["batch_launches"], 2) for k, v in st.items()}}
        rec["loop_over_many"] = round(rec["ms_per_32_images"]["loop_flush"]["median"]
                                      / rec["ms_per_32_images"]["flush_many"]["median"], 2)
        _emit(lines, rec)
    return lines


def run_record(a):
    import torch

    from spotter_amd import draw
    from spotter_amd.jpeg import DeviceRGBImage

    labels = _chunk_labels(8)
    t = torch.zeros((640, 640, 3), dtype=torch.uint8)  # host pixels will do: nothing is flushed

    def run(f):
        ims = [DeviceRGBImage(t) for _ in labels]
        t0 = time.perf_counter()
        for im, (boxes, texts) in zip(ims, labels):
            f(im, boxes, texts)
        return 1e3 * (time.perf_counter() - t0), ims

    legs = {"draw_loop": _draw_loop, "record_labels": draw.record_labels}
    for _ in range(3):  # warm-up: the font's memo and the stamps
        lists = {k: [im._draw_list.packed() for im in run(f)[1]] for k, f in legs.items()}
        assert lists["draw_loop"] == lists["record_labels"]
    ms = {k: [] for k in legs}
    s0 = dict(draw.stamp_stats)
    for _ in range(a.pairs):
        for k, f in legs.items():
            ms[k].append(run(f)[0])
    rec = {"n": len(labels), "labels_per_chunk": sum(len(b) for b, _ in labels), "pairs": a.pairs,
           "host_ms_per_chunk": {k: _stat(v) for k, v in ms.items()},
           "stamp_stats": {k: draw.stamp_stats[k] - s0[k] for k in s0}}
    rec["loop_over_record"] = round(rec["host_ms_per_chunk"]["draw_loop"]["median"]
                                    / rec["host_ms_per_chunk"]["record_labels"]["median"], 2)
    lines = []
    _emit(lines, rec)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("bulk", "flush", "record"))
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--precisions", default="fp32,bf16")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    if a.what == "record":
        lines = run_record(a)
    else:
        import torch

        from spotter_amd._lib import lib

        assert lib().sp_device_init(0) == 0
        dev = torch.device("cuda", 0)
        lines = run_bulk(a, dev) if a.what == "bulk" else run_flush(a, dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
