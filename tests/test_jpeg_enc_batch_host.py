"""CPU: the host half of the batched JPEG encode (sp_jpeg_enc_batch_plan over mixed layouts and its refusals) and the
labelled output of the bulk pipeline's control flow (BulkDetector(labelled=True) and the CLI's --labelled-dir) with
the host stand-ins of tests/test_jpeg_batch_host.py for decoder, processor and model, and one for the encoder."""
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
from test_jpeg_batch_host import StubDecoder, StubProcessor, _disjoint, _model, _png, _raw  # noqa: E402

from spotter_amd._lib import (SP_JPEG_BATCH_MAX, SP_JPEG_ENC_FDCT_MCUS, SP_JPEG_ENC_WG_MCUS,  # noqa: E402
                              SpJpegEncBatchItem, SpJpegEncBatchTotals, SpJpegEncLayout, lib)

# (width, height, quality, Pillow subsampling code): one MCU, MCU counts around 4 and 256, every sampling, edges
SHAPES = [(1, 1, 75, 2), (8, 8, 50, 0), (17, 9, 90, 1), (640, 640, -1, -1), (1200, 717, 75, 2), (2048, 8, 100, 0),
          (257 * 8, 8, 1, 0), (33, 47, 60, 2), (16, 16, 75, 2), (4 * 8, 8, 75, 0), (5 * 8, 8, 75, 0)]


def _lay(w, h, q, sub):
    lay = SpJpegEncLayout()
    assert lib().sp_jpeg_enc_plan(w, h, q, sub, C.byref(lay)) == 0, lib().sp_last_error()
    return lay


def _plan(lays):
    n = len(lays)
    arr = (SpJpegEncLayout * max(n, 1))(*lays)
    items = (SpJpegEncBatchItem * max(n, 1))()
    tot = SpJpegEncBatchTotals()
    return lib().sp_jpeg_enc_batch_plan(arr, n, items, C.byref(tot)), items, tot


@pytest.mark.parametrize("n", [1, 2, 11, SP_JPEG_BATCH_MAX])
def test_plan_offsets_and_prefix_columns(n):
    lays = [_lay(*SHAPES[(3 * i + n) % len(SHAPES)]) for i in range(n)]
    rc, items, tot = _plan(lays)
    assert rc == 0, lib().sp_last_error()
    assert (SP_JPEG_ENC_FDCT_MCUS, SP_JPEG_ENC_WG_MCUS) == (4, 256)
    wg_f = wg_m = cap = 0
    for i, lay in enumerate(lays):
        it = items[i]
        assert bytes(it.lay) == bytes(lay)
        assert it.work_off % 256 == 0 and it.reserved == 0
        assert (it.first_wg_fdct, it.first_wg_mcu) == (wg_f, wg_m)
        nmcu = lay.mcux * lay.mcuy
        wg_f += -(-nmcu // 4)
        wg_m += -(-nmcu // 256)
        cap += -(-lay.bits_cap // 16) * 16
    assert (tot.wg_fdct, tot.wg_mcu, tot.bits_cap) == (wg_f, wg_m, cap)
    # each image's range is exactly its single-image workspace; the ranges are disjoint and inside the total
    _disjoint([(it.work_off, it.work_off + it.lay.work_bytes) for it in items[:n]], tot.work_bytes)


def test_plan_leaves_the_callers_source_fields_alone():
    lays = [_lay(*SHAPES[1]), _lay(*SHAPES[2])]
    arr = (SpJpegEncLayout * 2)(*lays)
    items, tot = (SpJpegEncBatchItem * 2)(), SpJpegEncBatchTotals()
    for k, it in enumerate(items):
        it.src, it.row_stride, it.pixel_bytes = 4096 * (k + 1), 100 + k, 3 + k
    assert lib().sp_jpeg_enc_batch_plan(arr, 2, items, C.byref(tot)) == 0
    assert [(it.src, it.row_stride, it.pixel_bytes) for it in items] == [(4096, 100, 3), (8192, 101, 4)]


def test_plan_refusals():
    L = lib()
    one = [_lay(*SHAPES[3])]
    rc, _, _ = _plan([])
    assert rc == -1 and b"n = 0" in L.sp_last_error()
    rc, _, _ = _plan([_lay(*SHAPES[i % len(SHAPES)]) for i in range(SP_JPEG_BATCH_MAX + 1)])
    assert rc == -1 and f"n = {SP_JPEG_BATCH_MAX + 1}".encode() in L.sp_last_error()
    arr, items, tot = (SpJpegEncLayout * 1)(*one), (SpJpegEncBatchItem * 1)(), SpJpegEncBatchTotals()
    for args in ((None, 1, items, C.byref(tot)), (arr, 1, None, C.byref(tot)), (arr, 1, items, None)):
        assert L.sp_jpeg_enc_batch_plan(*args) == -1 and b"null" in L.sp_last_error()
    # one byte changed: in a quantiser table, in the geometry, in a size the kernels index by
    for off in (SpJpegEncLayout.quant.offset + 5, SpJpegEncLayout.mcux.offset, SpJpegEncLayout.bits_cap.offset,
                SpJpegEncLayout.shift.offset + 255):
        raw = bytearray(bytes(one[0]))
        raw[off] ^= 1
        rc, _, _ = _plan([_lay(*SHAPES[0]), SpJpegEncLayout.from_buffer_copy(bytes(raw))])
        assert rc == -1 and b"image 1: layout is not sp_jpeg_enc_plan's" in L.sp_last_error(), off
    rc, _, _ = _plan(one)  # and the same arguments with nothing wrong pass
    assert rc == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_plan_and_check_are_sanitizer_clean(tmp_path):
    """tools/sanitize/jpeg_enc_batch_plan.cpp, a stand-alone ASan + UBSan program over the plan and the table check
    (as tests/test_jpeg_batch_host.py runs the decode side's)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "jpeg_enc_batch_plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(root, "tools", "sanitize", "jpeg_enc_batch_plan.cpp"),
                    "-o", str(exe)], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    layouts, accepted, refused = (int(x) for x in r.stdout.split())
    assert layouts > 500 and accepted > 50 and refused > 1000


# ------------------------------------------------------------------------------------- labelled bulk output
ID2LABEL = {0: "zero", 1: "one", 2: "two"}


class StubEncoder:
    """encode_many as a function of what it is handed: size, comment and the pixels' checksum."""

    def __init__(self):
        self.calls = []

    def encode_many(self, srcs, quality=-1, subsampling=-1, comments=None, max_workers=None):
        self.calls.append(len(srcs))
        assert (quality, subsampling) == (-1, -1) and len(comments) == len(srcs)
        return [b"JPG %dx%d %d %r" % (*im.size, int(np.asarray(im, dtype=np.int64).sum()), c)
                for im, c in zip(srcs, comments)]


def _detector(batch=3, **kw):
    from spotter_amd.bulk import BulkDetector

    enc = StubEncoder()
    det = BulkDetector(_model, StubProcessor(), batch=batch, decoder=StubDecoder(), encoder=enc, **kw)
    return det, enc


def _drawn(value, h, w, text):
    """What stage C draws on a flat stand-in image whose one box is the whole image."""
    from PIL import Image, ImageDraw

    im = Image.fromarray(np.full((h, w, 3), value, np.uint8))
    if text is not None:
        d = ImageDraw.Draw(im)
        d.rectangle([0.0, 0.0, float(w), float(h)], outline="red", width=3)
        d.text(xy=(5.0, 5.0), text=text, fill="white", stroke_width=1, stroke_fill="black")
    return im


def test_labelled_needs_id2label_and_known_names():
    from spotter_amd.bulk import BulkDetector

    with pytest.raises(ValueError, match="id2label"):
        BulkDetector(_model, StubProcessor(), labelled=True)
    with pytest.raises(ValueError, match="nine"):
        BulkDetector(_model, StubProcessor(), labelled=True, id2label=ID2LABEL, label_map={"one": "1", "nine": "9"})
    BulkDetector(_model, StubProcessor(), labelled=True, id2label=ID2LABEL, label_map={"one": "1"})


def test_labelled_results_carry_the_drawn_image_per_chunk():
    det, enc = _detector(batch=3, labelled=True, id2label=ID2LABEL, label_map={"zero": "nil", "two": "deux"})
    items = [_raw(9, h=40, w=60), _png(50, h=30, w=50), b"neither", _raw(4, h=32, w=48), _raw(11, h=24, w=64)]
    out = list(det.detect(items))
    plain = list(_detector(batch=3)[0].detect(items))
    assert enc.calls == [2, 2]  # one encode_many per chunk, without the file nothing could open
    assert len(det.stage_seconds["c"]) == len(det.stage_seconds["b"]) == 2
    assert "jpeg" not in out[2] and "error" in out[2] and all("jpeg" not in r for r in plain)
    # labels are value % 3: 9 -> zero -> "nil", 50 and 11 -> two -> "deux", 4 -> one: not in the map, nothing drawn
    for i, (v, h, w, text) in {0: (9, 40, 60, "nil"), 1: (50, 30, 50, "deux"), 3: (4, 32, 48, None),
                               4: (11, 24, 64, "deux")}.items():
        want = _drawn(v, h, w, text)
        assert out[i]["jpeg"] == b"JPG %dx%d %d %r" % (w, h, int(np.asarray(want, dtype=np.int64).sum()), None), i
        assert all(torch.equal(out[i][k], plain[i][k]) for k in ("scores", "labels", "boxes"))
        assert out[i]["size"] == plain[i]["size"]


def test_labelled_without_a_map_draws_every_name_and_keeps_the_files_comment():
    from PIL import Image

    gif = io.BytesIO()
    Image.fromarray(np.full((24, 32), 7, np.uint8)).save(gif, "GIF", comment=b"hello")
    det, enc = _detector(batch=4, labelled=True, id2label=ID2LABEL)
    out = list(det.detect([_raw(4, h=24, w=40), gif.getvalue()]))
    want = _drawn(4, 24, 40, "one")
    assert out[0]["jpeg"] == b"JPG 40x24 %d %r" % (int(np.asarray(want, dtype=np.int64).sum()), None)
    assert out[1]["jpeg"].startswith(b"JPG 32x24 ") and out[1]["jpeg"].endswith(b"%r" % b"hello")


def test_cli_writes_the_labelled_files(tmp_path):
    from spotter_amd import bulk

    root = tmp_path / "in"
    (root / "b").mkdir(parents=True)
    (root / "b" / "2.raw").write_bytes(_raw(22, h=30, w=40))
    (root / "b" / "1.png").write_bytes(_png(21, h=20, w=30))
    (root / "bad.txt").write_bytes(b"text")
    single = tmp_path / "z.raw"
    single.write_bytes(_raw(99, h=16, w=24))
    out, ldir = tmp_path / "results.jsonl", tmp_path / "labelled" / "deep"
    seen = {}

    def make(args):
        seen.update(vars(args))
        return _detector(batch=args.batch, labelled=args.labelled_dir is not None, id2label=ID2LABEL)[0], ID2LABEL

    rc = bulk.main(["--model", "synthetic:r18vd", "--batch", "2", "--labelled-dir", str(ldir), "--out", str(out),
                    str(single), str(root)], make_detector=make)
    assert rc == 0 and seen["labelled_dir"] == str(ldir)
    lines = [json.loads(x) for x in out.read_text().splitlines()]
    assert [os.path.basename(x["file"]) for x in lines] == ["z.raw", "bad.txt", "1.png", "2.raw"]
    assert all("jpeg" not in x for x in lines) and set(lines[1]) == {"file", "error"}
    # <index in the walk:06d>_<file name without its extension>.jpg; nothing for the refused file
    assert sorted(os.listdir(ldir)) == ["000000_z.jpg", "000002_1.jpg", "000003_2.jpg"]
    assert (ldir / "000000_z.jpg").read_bytes().startswith(b"JPG 24x16 ")
    assert (ldir / "000003_2.jpg").read_bytes().startswith(b"JPG 40x30 ")
    # without the option nothing is made and the detector is built unlabelled
    out2 = tmp_path / "r2.jsonl"
    assert bulk.main(["--model", "m", "--out", str(out2), str(single)], make_detector=make) == 0
    assert seen["labelled_dir"] is None and out2.read_text() == out.read_text().splitlines()[0] + "\n"
