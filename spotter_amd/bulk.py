"""Bulk detection from files: JPEG bytes in, detections out, at batch size, with the decode of the next chunk
overlapped with the forward of the current one.

    det = BulkDetector(model, processor, batch=32)
    for res in det.detect(paths_or_bytes):
        ...  # {"size": (w, h), "scores", "labels", "boxes"} or {"error": str}, in input order

    python -m spotter_amd.bulk --model NAME [--precision P] [--batch 32] [--threshold 0.5]
                               [--jpeg-entropy {host,gpu,auto}] [--labelled-dir DIR] --out results.jsonl PATH...

Per chunk of `batch` files, stage A (one host thread with a stream of its own) reads the files and decodes them with
JpegDecoder.decode_many: one H2D copy, two launches and one status readback for the chunk. What decode_many returns
as UnsupportedJpeg (PNG, CMYK, malformed files, ...) goes through Pillow's Image.open(...).convert("RGB"), exactly as
the drop-in leaves such files to Pillow, and joins the same batch as a host array; what Pillow refuses too becomes
that file's {"error"} and the chunk runs without it. Stage B (the caller's thread and stream) waits for A's event and
runs processor → model → post_process_object_detection on the whole chunk. A of chunk i+1 runs while B of chunk i
does, so two RGB arenas are alive at a time. One process, two threads and the decode pool; a failure of the GPU step
propagates as the exception it is.

With labelled=True every result also carries "jpeg", the labelled image /detect returns (serve.py:119-142): stage C
records each chunk image's boxes and texts (spotter_amd/draw.py record_labels), applies the chunk's draws in place on
the device with one launch and encodes the chunk, both inside one JpegEncoder.encode_many.
With label_overlap=True stage C runs on a thread and stream of its own while stage B of the next chunk runs (off by
default: measured no faster, §5.28).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import contextlib
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


def _file_info(data: bytes) -> dict:
    """What of the file's Pillow `info` its JPEG save writes back: the comment (JpegImagePlugin._save)."""
    from PIL import Image

    try:
        with Image.open(io.BytesIO(data)) as im:
            c = im.info.get("comment")
    except Exception:  # noqa: BLE001 - a file Pillow refuses carries nothing
        return {}
    return {} if c is None else {"comment": c}


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
    labelled: every successful result also carries "jpeg", the bytes /detect puts into labeled_image_base64 before
    base64: for each detection whose label name (id2label[label], required) is a key of label_map, or for every
    detection when label_map is None, a red rectangle of width 3 and the text (label_map's value, or the name) at
    (x0 + 5, y0 + 5) in white with a black stroke of 1, then the image saved as JPEG at Pillow's defaults with the
    source file's comment, as DeviceRGBImage.save writes it. A label_map key that is none of id2label's names is a
    ValueError. encoder: the JpegEncoder to use (default: the device's shared one), or anything with encode_many.
    label_draw: "batched" records the labels with record_labels, so that encode_many applies a chunk's draws with one
    launch; "pillow" makes the drop-in's ImageDraw calls and one sp_draw_rgb launch per image, as before §5.28.
    label_overlap: stage C of chunk i runs on a worker thread with a stream of its own while the caller's thread runs
    stage B of chunk i + 1 (its results are then yielded one stage B later); False: C runs at the end of B, on its
    thread and stream. Both choices give the same results; the defaults are what measured faster: the batched draw
    does, the overlap does not (both threads are Python-bound and share the interpreter lock).
    `stage_seconds` keeps the busy time of stage A and stage B of every chunk of the last detect() ("a" / "b",
    seconds), and with labelled=True that of the draw-plus-encode part ("c", not counted in "b")."""

    def __init__(self, model, processor, batch=32, threshold=0.5, decode_workers=None, decoder=None, device=None,
                 jpeg_entropy="host", labelled=False, id2label=None, label_map=None, encoder=None,
                 label_draw="batched", label_overlap=False):
        from .config import check_jpeg_entropy

        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        if label_draw not in ("batched", "pillow"):
            raise ValueError("label_draw must be 'batched' or 'pillow'")
        self.label_draw, self.label_overlap = label_draw, bool(label_overlap)
        self._stream_c = None  # stage C's stream (label_overlap)
        if labelled and id2label is None:
            raise ValueError("labelled=True needs id2label (the model's config.id2label)")
        if label_map is not None and id2label is not None:
            unknown = sorted(set(label_map) - set(id2label.values()))
            if unknown:
                raise ValueError(f"label_map names labels id2label does not have: {unknown}")
        self.labelled, self.id2label, self.label_map, self._encoder = bool(labelled), id2label, label_map, encoder
        self.jpeg_entropy = check_jpeg_entropy(jpeg_entropy)
        self.model, self.processor = model, processor
        self.batch, self.threshold, self.decode_workers = int(batch), float(threshold), decode_workers
        self._decoder, self._device = decoder, device
        self._stream = None  # stage A's stream
        self.stage_seconds = {"a": [], "b": [], "c": []}

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
        infos = [_file_info(d) if im is not None else None for d, im in zip(datas, images)] if self.labelled else None
        self.stage_seconds["a"].append(time.perf_counter() - t0)
        return res, images, event, infos

    # -- stage B: the caller's thread and stream --------------------------------------------------------------
    def _stage_b(self, res, images, event, gpu, infos=None):
        import torch

        t0 = time.perf_counter()
        work = None  # what stage C needs of this chunk
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
            if self.labelled:
                fwd = None
                if gpu is not None and self.label_overlap:
                    # the forward's reads of the chunk's pixels are enqueued: stage C's stream draws after them
                    fwd = torch.cuda.Event()
                    fwd.record(cur)
                work = (keep, batch, infos, fwd)
        self.stage_seconds["b"].append(time.perf_counter() - t0)
        return res, work

    # -- stage C: draw and encode, after stage B of its chunk -------------------------------------------------
    def _stage_c(self, res, work, gpu):
        """Stage C of one chunk, timed, on the calling thread: B's own (its current stream), or with label_overlap the
        worker's, where it runs on stage C's stream behind the event B recorded after the forward."""
        t0 = time.perf_counter()
        keep, batch, infos, fwd = work
        if fwd is None:
            self._label_chunk(res, keep, batch, infos, gpu)
        else:
            import torch

            dev = gpu[0]
            if self._stream_c is None:
                self._stream_c = torch.cuda.Stream(dev)
            sc = self._stream_c
            with torch.cuda.device(dev), torch.cuda.stream(sc):
                sc.wait_event(fwd)
                for im in batch:
                    if torch.is_tensor(im) and im.is_cuda:
                        im.record_stream(sc)  # the arena is A's, read on B's stream and drawn on here
                self._label_chunk(res, keep, batch, infos, gpu)
        self.stage_seconds["c"].append(time.perf_counter() - t0)
        return res

    def _label_chunk(self, res, keep, batch, infos, gpu):
        """serve.py:119-142 over the chunk: the labels recorded on a DeviceRGBImage over the chunk's own pixels (drawn
        in place: the forward has read them, and the arena is the chunk's), then one encode_many, which applies the
        chunk's draws with one launch. An image whose save the GPU encoder does not take (an unusual comment) is saved
        on its own, by the rule DeviceRGBImage.save applies."""
        from .draw import draw_module, record_labels
        from .jpeg import _gpu_jpeg_options

        draw_mod = draw_module()
        pictures = []
        for k, im in zip(keep, batch):
            picture = self._picture(im, infos[k], gpu)
            boxes, texts = [], []
            for lab, box in zip(res[k]["labels"].tolist(), res[k]["boxes"].tolist()):
                text = self.id2label[int(lab)]
                if self.label_map is not None:
                    if text not in self.label_map:
                        continue
                    text = self.label_map[text]
                boxes.append(box)
                texts.append(text)
            if self.label_draw == "batched":
                record_labels(picture, boxes, texts)
            else:
                draw = draw_mod.Draw(picture)
                for box, text in zip(boxes, texts):
                    draw.rectangle(box, outline="red", width=3)
                    draw.text(xy=(box[0] + 5, box[1] + 5), text=text, fill="white", stroke_width=1,
                              stroke_fill="black")
                if hasattr(picture, "flush"):
                    picture.flush()  # one sp_draw_rgb launch per image, as before encode_many batched the draws
            pictures.append(picture)
        opts = [_gpu_jpeg_options(p, io.BytesIO(), "JPEG", {}) for p in pictures]
        together = [i for i, o in enumerate(opts) if o is not None]
        enc = self._encoder
        if enc is None:
            from .jpeg import encoder

            enc = self._encoder = encoder(gpu[0] if gpu is not None else None)
        files = enc.encode_many([pictures[i] for i in together], comments=[opts[i][2] for i in together],
                                max_workers=self.decode_workers)
        for i, data in zip(together, files):
            res[keep[i]]["jpeg"] = data
        for i, o in enumerate(opts):
            if o is None:
                b = io.BytesIO()
                pictures[i].save(b, format="JPEG")
                res[keep[i]]["jpeg"] = b.getvalue()

    def _picture(self, im, info, gpu):
        """The chunk image as the PIL image the draws and the save work on: a DeviceRGBImage over the device pixels
        (a host array from the Pillow fallback is uploaded), or, with a host stand-in for the decoder, Pillow's."""
        import numpy as np

        if gpu is None:
            from PIL import Image

            picture = Image.fromarray(np.ascontiguousarray(im))
            picture.info.update(info)
            return picture
        import torch

        from .jpeg import DeviceRGBImage

        if not torch.is_tensor(im):
            im = torch.tensor(np.asarray(im))  # a copy: Pillow's array is read-only
        return DeviceRGBImage(im.to(gpu[0]), info=info)

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

        self.stage_seconds = {"a": [], "b": [], "c": []}
        chunk = take()
        if not chunk:
            return
        gpu = self._gpu()
        overlap = self.labelled and self.label_overlap
        with contextlib.ExitStack() as stack:  # (leaving it, an early close() included, joins the threads)
            ex = stack.enter_context(cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="spotter-bulk"))
            ex_c = stack.enter_context(cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="spotter-bulk-c")) \
                if overlap else None
            fut = ex.submit(self._stage_a, chunk, gpu)
            before = None  # label_overlap: the previous chunk's stage C, yielded after this chunk's stage B
            try:
                while fut is not None:
                    res, images, event, infos = fut.result()
                    chunk = take()
                    fut = ex.submit(self._stage_a, chunk, gpu) if chunk else None
                    res, work = self._stage_b(res, images, event, gpu, infos)
                    if ex_c is None:
                        if work is not None:
                            self._stage_c(res, work, gpu)
                        yield from res
                        continue
                    now = ex_c.submit(self._stage_c, res, work, gpu) if work is not None else res
                    if before is not None:
                        yield from (before.result() if isinstance(before, cf.Future) else before)
                    before = now
                if before is not None:
                    yield from (before.result() if isinstance(before, cf.Future) else before)
            finally:
                if ex_c is not None:
                    ex_c.shutdown(wait=True, cancel_futures=True)  # nothing new starts after an error or a close()


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
    return BulkDetector(model, proc, batch=args.batch, threshold=args.threshold, jpeg_entropy=args.jpeg_entropy,
                        labelled=args.labelled_dir is not None, id2label=model.config.id2label), model.config.id2label


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
    ap.add_argument("--labelled-dir", metavar="DIR", default=None,
                    help="also write every file's labelled image (boxes and label names drawn, as /detect returns it) "
                         "to DIR/<index:06d>_<basename>.jpg")
    ap.add_argument("--out", required=True, help="JSON lines, one per file")
    ap.add_argument("paths", nargs="+", metavar="PATH", help="files, or directories walked in sorted order")
    args = ap.parse_args(argv)
    files = walk(args.paths)
    det, id2label = make_detector(args)
    if args.labelled_dir is not None:
        os.makedirs(args.labelled_dir, exist_ok=True)
    with open(args.out, "w") as out:
        for index, (path, r) in enumerate(zip(files, det.detect(files))):
            if args.labelled_dir is not None and "jpeg" in r:
                name = f"{index:06d}_{os.path.splitext(os.path.basename(path))[0]}.jpg"
                with open(os.path.join(args.labelled_dir, name), "wb") as f:
                    f.write(r["jpeg"])
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
