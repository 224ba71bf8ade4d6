"""Bulk detection from files: JPEG bytes in, detections out, at batch size, with the decode of the next chunk
overlapped with the forward of the current one.

    det = BulkDetector(model, processor, batch=32)
    for res in det.detect(paths_or_bytes):
        ...  # {"size": (w, h), "scores", "labels", "boxes"} or {"error": str}, in input order

    python -m spotter_amd.bulk --model NAME [--precision P] [--batch 32] [--threshold 0.5]
                               [--jpeg-entropy {host,gpu,auto}] --out results.jsonl PATH...

Per chunk of `batch` files, stage A (one host thread with a stream of its own) reads the files and decodes them with
JpegDecoder.decode_many: one H2D copy, two launches and one status readback for the chunk. What decode_many returns
as UnsupportedJpeg (PNG, CMYK, malformed files, ...) goes through Pillow's Image.open(...).convert("RGB"), exactly as
the drop-in leaves such files to Pillow, and joins the same batch as a host array; what Pillow refuses too becomes
that file's {"error"} and the chunk runs without it. Stage B (the caller's thread and stream) waits for A's event and
runs processor → model → post_process_object_detection on the whole chunk. A of chunk i+1 runs while B of chunk i
does, so two RGB arenas are alive at a time. One process, two threads and the decode pool; a failure of the GPU step
propagates as the exception it is.
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import io
import json
import os
import sys
import time


def _read(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    with open(os.fspath(item), "rb") as f:
        return f.read()


def _pillow_rgb(data: bytes):
    """The reference's host decode (serve.py:96-97) as a uint8 [H, W, 3] array."""
    import numpy as np
    from PIL import Image

    with Image.open(io.BytesIO(data)) as im:
        return np.asarray(im.convert("RGB"))


class BulkDetector:
    """model / processor: a SpotterForObjectDetection (any precision, batch_invariant or not) and a
    SpotterImageProcessor, or anything with their call surface. decoder: the JpegDecoder to use (default: the
    device's shared decoder of entropy mode jpeg_entropy: "host", the default, or "gpu" / "auto", which decode the
    baseline files of a chunk in one GPU launch chain); decode_workers: decode_many's max_workers.
    `stage_seconds` keeps the busy time of stage A and stage B of every chunk of the last detect() ("a" / "b",
    seconds)."""

    def __init__(self, model, processor, batch=32, threshold=0.5, decode_workers=None, decoder=None, device=None,
                 jpeg_entropy="host"):
        from .config import check_jpeg_entropy

        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        self.jpeg_entropy = check_jpeg_entropy(jpeg_entropy)
        self.model, self.processor = model, processor
        self.batch, self.threshold, self.decode_workers = int(batch), float(threshold), decode_workers
        self._decoder, self._device = decoder, device
        self._stream = None  # stage A's stream
        self.stage_seconds = {"a": [], "b": []}

    # -- stage A: the decode thread ---------------------------------------------------------------------------
    def _gpu(self):
        """(device, stage A's stream) when the decoder works on a GPU, else None (a host stand-in)."""
        import torch

        if self._decoder is None:
            from .jpeg import decoder

            self._decoder = decoder(self._device, self.jpeg_entropy)
        dev = getattr(self._decoder, "dev", None)
        if dev is None or torch.device(dev).type != "cuda":
            return None
        if self._stream is None:
            self._stream = torch.cuda.Stream(dev)
        return torch.device(dev), self._stream

    def _stage_a(self, chunk, gpu):
        from .jpeg import UnsupportedJpeg

        t0 = time.perf_counter()
        res = [None] * len(chunk)  # {"error"} for the files nothing could open
        datas = [None] * len(chunk)
        for k, item in enumerate(chunk):
            try:
                datas[k] = _read(item)
            except OSError as e:
                res[k] = {"error": f"{type(e).__name__}: {e}"}
        live = [k for k, d in enumerate(datas) if d]  # an empty file goes straight to Pillow's refusal
        images = [None] * len(chunk)
        event = None
        if live:
            if gpu is None:
                decoded = self._decoder.decode_many([datas[k] for k in live], max_workers=self.decode_workers)
            else:
                import torch

                dev, stream = gpu
                with torch.cuda.device(dev), torch.cuda.stream(stream):
                    decoded = self._decoder.decode_many([datas[k] for k in live], max_workers=self.decode_workers)
                    event = torch.cuda.Event()
                    event.record(stream)
            for k, d in zip(live, decoded):
                if not isinstance(d, UnsupportedJpeg):
                    images[k] = d
        for k, d in enumerate(datas):
            if images[k] is None and res[k] is None:
                try:
                    images[k] = _pillow_rgb(d)
                except Exception as e:  # noqa: BLE001 - whatever Pillow raises for a file it refuses
                    res[k] = {"error": f"{type(e).__name__}: {e}"}
        self.stage_seconds["a"].append(time.perf_counter() - t0)
        return res, images, event

    # -- stage B: the caller's thread and stream --------------------------------------------------------------
    def _stage_b(self, res, images, event, gpu):
        import torch

        t0 = time.perf_counter()
        keep = [k for k, im in enumerate(images) if im is not None]
        if keep:
            batch = [images[k] for k in keep]
            if gpu is not None:
                cur = torch.cuda.current_stream(gpu[0])
                if event is not None:
                    cur.wait_event(event)
                for im in batch:
                    if torch.is_tensor(im) and im.is_cuda:
                        im.record_stream(cur)  # the arena came from stage A's stream and is read on this one
            sizes = [(int(im.shape[1]), int(im.shape[0])) for im in batch]
            inputs = self.processor(images=batch, return_tensors="pt")
            with torch.no_grad():
                outputs = self.model(pixel_values=inputs["pixel_values"])
            dets = self.processor.post_process_object_detection(
                outputs, threshold=self.threshold, target_sizes=[(h, w) for w, h in sizes])
            for k, size, d in zip(keep, sizes, dets):
                res[k] = {"size": size, "scores": d["scores"], "labels": d["labels"], "boxes": d["boxes"]}
        self.stage_seconds["b"].append(time.perf_counter() - t0)
        return res

    def detect(self, items):
        """items: an iterable of bytes or paths. Yields one result per item, in input order."""
        it = iter(items)

        def take():
            chunk = []
            for item in it:
                chunk.append(item)
                if len(chunk) == self.batch:
                    break
            return chunk

        self.stage_seconds = {"a": [], "b": []}
        chunk = take()
        if not chunk:
            return
        gpu = self._gpu()
        with cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="spotter-bulk") as ex:
            fut = ex.submit(self._stage_a, chunk, gpu)
            while fut is not None:
                res, images, event = fut.result()
                chunk = take()
                fut = ex.submit(self._stage_a, chunk, gpu) if chunk else None
                yield from self._stage_b(res, images, event, gpu)


def walk(paths):
    """The files the CLI reads: each path itself, or every file below a directory in sorted order."""
    out = []
    for p in paths:
        if os.path.isdir(p):
            for root, dirs, files in os.walk(p):
                dirs.sort()
                out += [os.path.join(root, f) for f in sorted(files)]
        else:
            out.append(p)
    return out


def _detector(args):
    from . import SpotterForObjectDetection, SpotterImageProcessor

    model = SpotterForObjectDetection.from_pretrained(args.model, precision=args.precision)
    proc = SpotterImageProcessor.from_pretrained(args.model)
    return BulkDetector(model, proc, batch=args.batch, threshold=args.threshold,
                        jpeg_entropy=args.jpeg_entropy), model.config.id2label


def main(argv=None, make_detector=_detector) -> int:
    """make_detector(args) → (BulkDetector, id2label): the tests put a host stand-in here."""
    from .config import JPEG_ENTROPY_MODES, jpeg_entropy_from_env

    ap = argparse.ArgumentParser(prog="python -m spotter_amd.bulk", description=__doc__.split("\n\n")[0])
    ap.add_argument("--model", required=True, help="as from_pretrained: a directory, a cached hub id, synthetic:<preset>")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--jpeg-entropy", choices=JPEG_ENTROPY_MODES, default=jpeg_entropy_from_env(),
                    help="where baseline JPEGs are Huffman-decoded (default: SPOTTER_JPEG_ENTROPY, i.e. host)")
    ap.add_argument("--out", required=True, help="JSON lines, one per file")
    ap.add_argument("paths", nargs="+", metavar="PATH", help="files, or directories walked in sorted order")
    args = ap.parse_args(argv)
    files = walk(args.paths)
    det, id2label = make_detector(args)
    with open(args.out, "w") as out:
        for path, r in zip(files, det.detect(files)):
            if "error" in r:
                line = {"file": path, "error": r["error"]}
            else:
                line = {"file": path, "width": r["size"][0], "height": r["size"][1], "detections": [
                    {"label": id2label[int(lab)], "score": float(s), "box": [float(v) for v in box]}
                    for s, lab, box in zip(r["scores"], r["labels"], r["boxes"])]}
            out.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
