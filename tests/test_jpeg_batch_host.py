"""CPU: the host half of the batched JPEG decode (sp_jpeg_batch_plan over layouts of real files) and the bulk
pipeline's control flow (spotter_amd.bulk.BulkDetector and its CLI) with host stand-ins for decoder, processor and
model: numpy functions of the bytes, the way tests/test_shared_batch.py stubs its forward."""
import ctypes as C
import io
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
from jpeg_entropy_cases import cases, non_eligible  # noqa: E402

from spotter_amd._lib import (SP_JPEG_BATCH_COLOR_PX, SP_JPEG_BATCH_IDCT_BLOCKS, SP_JPEG_BATCH_MAX,  # noqa: E402
                              SpJpegBatchItem, SpJpegBatchTotals, SpJpegLayout, lib)


@pytest.fixture(scope="module")
def layouts():
    from spotter_amd.jpeg import decode_coefs

    return [decode_coefs(d)[0] for _, d in cases() + non_eligible()]


def _plan(lays):
    n = len(lays)
    arr = (SpJpegLayout * max(n, 1))(*lays)
    items = (SpJpegBatchItem * max(n, 1))()
    tot = SpJpegBatchTotals()
    rc = lib().sp_jpeg_batch_plan(arr, n, items, C.byref(tot))
    return rc, items, tot


def _disjoint(ranges, total):
    ranges = sorted(ranges)
    assert ranges[0][0] >= 0 and ranges[-1][1] <= total
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a0 < a1 <= b0 < b1


@pytest.mark.parametrize("n", [1, 2, 7, SP_JPEG_BATCH_MAX])
def test_plan_offsets_and_prefix_columns(layouts, n):
    lays = [layouts[(3 * i + n) % len(layouts)] for i in range(n)]
    rc, items, tot = _plan(lays)
    assert rc == 0, lib().sp_last_error()
    wg_i = wg_c = 0
    for i, lay in enumerate(lays):
        it = items[i]
        assert bytes(it.lay) == bytes(lay)
        assert it.work_off % 16 == 0 and it.rgb_off % 256 == 0 and it.coef_off >= 0
        assert all((it.work_off + lay.plane_off[c]) % 8 == 0 for c in range(lay.ncomp))
        assert it.rgb_stride == 3 * lay.width
        # exclusive prefix sums of the per-image counts: the single-image IDCT launch's own count, and the batched
        # colour pass's 1024 pixels per workgroup
        assert (it.first_wg_idct, it.first_wg_color) == (wg_i, wg_c)
        wg_i += -(-lay.total_blocks // 32)
        wg_c += -(-lay.width * lay.height // 1024)
    assert (SP_JPEG_BATCH_IDCT_BLOCKS, SP_JPEG_BATCH_COLOR_PX) == (32, 1024)
    assert (tot.wg_idct, tot.wg_color) == (wg_i, wg_c)
    _disjoint([(it.coef_off, it.coef_off + it.lay.total_blocks * 64) for it in items[:n]], tot.coef_elems)
    _disjoint([(it.work_off, it.work_off + it.lay.plane_bytes) for it in items[:n]], tot.work_bytes)
    _disjoint([(it.rgb_off, it.rgb_off + it.rgb_stride * it.lay.height) for it in items[:n]], tot.rgb_bytes)


def test_plan_refusals(layouts):
    L = lib()
    one = layouts[:1]
    rc, _, _ = _plan([])
    assert rc == -1 and b"n = 0" in L.sp_last_error()
    rc, _, _ = _plan([layouts[i % len(layouts)] for i in range(SP_JPEG_BATCH_MAX + 1)])
    assert rc == -1 and f"n = {SP_JPEG_BATCH_MAX + 1}".encode() in L.sp_last_error()
    arr, items, tot = (SpJpegLayout * 1)(*one), (SpJpegBatchItem * 1)(), SpJpegBatchTotals()
    for args in ((None, 1, items, C.byref(tot)), (arr, 1, None, C.byref(tot)), (arr, 1, items, None)):
        assert L.sp_jpeg_batch_plan(*args) == -1 and b"null" in L.sp_last_error()
    narrow = SpJpegLayout.from_buffer_copy(bytes(next(lay for lay in layouts if lay.width > 16)))
    narrow.bw[0] = (narrow.width - 1) // 8  # bw * 8 < the component's width
    rc, _, _ = _plan([layouts[0], narrow])
    assert rc == -1 and b"image 1: inconsistent layout" in L.sp_last_error()
    rc, _, _ = _plan(one)  # and the same arguments with nothing wrong pass
    assert rc == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_plan_is_sanitizer_clean(tmp_path):
    """tools/sanitize/jpeg_batch_plan.cpp, a stand-alone ASan + UBSan program, over the layouts of the corrupt
    corpus (as tests/test_jpeg_corpus.py runs the parser's harness)."""
    from jpeg_corpus import corpus, pack

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "jpeg_batch_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(root, "tools", "sanitize", "jpeg_batch_plan.cpp"), "-o",
                    str(exe)], check=True, timeout=300)
    blob = tmp_path / "corpus.bin"
    blob.write_bytes(pack(corpus()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    layouts, plans, refused = (int(x) for x in r.stdout.split())
    assert layouts > 1000 and plans > 1000 and refused > 1000


# ------------------------------------------------------------------------------------------- the bulk pipeline
def _png(value, h=5, w=7):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.full((h, w, 3), value, np.uint8)).save(b, "PNG")
    return b.getvalue()


def _raw(value, h=4, w=6):
    """The stand-in decoder's own format: b"RAW" + h + w + value."""
    return b"RAW" + bytes([h, w, value])


class StubDecoder:
    """decode_many over the stand-in format; everything else is UnsupportedJpeg, returned and not raised."""

    def __init__(self):
        self.calls = []

    def decode_many(self, datas, max_workers=None):
        from spotter_amd.jpeg import UnsupportedJpeg

        self.calls.append(len(datas))
        return [np.full((d[3], d[4], 3), d[5], np.uint8) if d[:3] == b"RAW" else UnsupportedJpeg("not RAW")
                for d in datas]


class StubProcessor:
    def __init__(self):
        self.batches = []

    def __call__(self, images=None, return_tensors="pt"):
        self.batches.append(len(images))
        return {"pixel_values": np.stack([np.float32(im.mean()) for im in images])}

    def post_process_object_detection(self, outputs, threshold=0.5, target_sizes=None):
        return [{"scores": torch.tensor([float(v) / 255]), "labels": torch.tensor([int(v) % 3]),
                 "boxes": torch.tensor([[0.0, 0.0, float(w), float(h)]])} for v, (h, w) in zip(outputs, target_sizes)]


def _model(pixel_values=None):
    return pixel_values


def _detector(batch=3, model=_model):
    from spotter_amd.bulk import BulkDetector

    dec, proc = StubDecoder(), StubProcessor()
    return BulkDetector(model, proc, batch=batch, decoder=dec), dec, proc


def _value(res):
    return round(float(res["scores"][0]) * 255)


def test_bulk_order_chunks_and_partial_last_chunk():
    det, dec, proc = _detector(batch=3)
    items = [_raw(10 + i, h=4 + i, w=6) for i in range(8)]
    out = list(det.detect(iter(items)))
    assert [_value(r) for r in out] == [10 + i for i in range(8)]
    assert [r["size"] for r in out] == [(6, 4 + i) for i in range(8)]
    assert dec.calls == [3, 3, 2] and proc.batches == [3, 3, 2]  # the last chunk at its own size
    assert len(det.stage_seconds["a"]) == len(det.stage_seconds["b"]) == 3
    assert list(det.detect([])) == [] and dec.calls == [3, 3, 2]


def test_bulk_pillow_fallback_and_errors(tmp_path):
    det, dec, proc = _detector(batch=4)
    p = tmp_path / "seven.raw"
    p.write_bytes(_raw(70))
    items = [_raw(1), _png(50), b"neither", _raw(4), str(p), b"", str(tmp_path / "missing.jpg"), _raw(9)]
    out = list(det.detect(items))
    assert [("error" in r) for r in out] == [False, False, True, False, False, True, True, False]
    assert [_value(r) for r in out if "error" not in r] == [1, 50, 4, 70, 9]
    assert out[1]["size"] == (7, 5)  # the PNG went through Pillow and was batched with the rest
    assert proc.batches == [3, 2]  # each chunk ran without the files nothing could open
    assert "UnidentifiedImageError" in out[2]["error"] and "FileNotFoundError" in out[6]["error"]
    # the neighbours' results are what they are without the bad files
    alone = list(_detector(batch=4)[0].detect([items[i] for i in (0, 1, 3, 4, 7)]))
    for a, b in zip(alone, [r for r in out if "error" not in r]):
        assert a["size"] == b["size"] and all(torch.equal(a[k], b[k]) for k in ("scores", "labels", "boxes"))


def test_bulk_model_exception_propagates():
    class Boom(RuntimeError):
        pass

    calls = []

    def model(pixel_values=None):
        calls.append(len(pixel_values))
        if len(calls) == 2:
            raise Boom("forward failed")
        return pixel_values

    det, _, _ = _detector(batch=2, model=model)
    gen = det.detect([_raw(i) for i in range(6)])
    assert [_value(next(gen)) for _ in range(2)] == [0, 1]
    with pytest.raises(Boom):
        next(gen)
    assert calls == [2, 2]  # not retried, not converted


def test_bulk_rejects_a_bad_batch_size():
    from spotter_amd.bulk import BulkDetector

    with pytest.raises(ValueError):
        BulkDetector(_model, StubProcessor(), batch=0)


def test_cli_writes_one_json_line_per_file_in_sorted_order(tmp_path):
    from spotter_amd import bulk

    root = tmp_path / "in"
    (root / "b").mkdir(parents=True)
    (root / "a").mkdir()
    (root / "b" / "2.raw").write_bytes(_raw(22))
    (root / "b" / "1.png").write_bytes(_png(21))
    (root / "a" / "9.raw").write_bytes(_raw(19))
    (root / "a" / "bad.txt").write_bytes(b"text")
    (root / "0.raw").write_bytes(_raw(5))
    single = tmp_path / "z.raw"
    single.write_bytes(_raw(99))
    out = tmp_path / "results.jsonl"
    seen = {}

    def make(args):
        seen.update(vars(args))
        return _detector(batch=args.batch)[0], {0: "zero", 1: "one", 2: "two"}

    rc = bulk.main(["--model", "synthetic:r18vd", "--batch", "2", "--out", str(out), str(single), str(root)],
                   make_detector=make)
    assert rc == 0 and seen["model"] == "synthetic:r18vd" and seen["threshold"] == 0.5 and seen["precision"] == "fp32"
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    want = [single, root / "0.raw", root / "a" / "9.raw", root / "a" / "bad.txt", root / "b" / "1.png",
            root / "b" / "2.raw"]
    assert [x["file"] for x in lines] == [str(p) for p in want]
    assert set(lines[3]) == {"file", "error"}
    for x, v in zip([lines[i] for i in (0, 1, 2, 4, 5)], (99, 5, 19, 21, 22)):
        assert set(x) == {"file", "width", "height", "detections"}
        (d,) = x["detections"]
        assert d["label"] == ["zero", "one", "two"][v % 3] and round(d["score"] * 255) == v
        assert d["box"] == [0.0, 0.0, float(x["width"]), float(x["height"])]
