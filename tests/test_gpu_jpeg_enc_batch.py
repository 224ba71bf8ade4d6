"""GPU: the batched JPEG encode (sp_jpeg_enc_batch_rgb, JpegEncoder.encode_many, BulkDetector(labelled=True)).

  bytes       every case of tests/jpeg_enc_cases.py through encode_many, grouped by (quality, subsampling), in chunks of
              64 in table order and reversed: Pillow's bytes
  boundaries  image borders inside a launch: MCU counts 1, 3, 4, 5, 255, 256, 257, 1025 in one chunk and reversed (the
              FDCT launch's 4 MCUs and the per-MCU launches' 256 per workgroup: tail waves and threads of one image
              next to the first of the next), 64 one-MCU images (every workgroup another row of the search), n = 1
  stages      one C-ABI call into a pattern-filled allocation with guards: per image the workspace (coefficients,
              per-MCU bit counts, offsets, total) and the segment are what a single sp_jpeg_enc_rgb call leaves; the
              packed layout; nothing else written
  the rest    stale buffers, the source forms in one chunk on a side stream, the refusals (nothing launched), the
              chunk rule, and the bulk pipeline's labelled images against the one-image path."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image, ImageDraw  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_enc_cases as ec  # noqa: E402
from test_gpu_jpeg_enc_stages import GUARD, _plan, _up, run_stages  # noqa: E402

from spotter_amd._lib import SP_JPEG_BATCH_MAX, SpJpegEncBatchItem, SpJpegEncBatchTotals  # noqa: E402
from spotter_amd._lib import SpJpegEncLayout, lib  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def enc(dev):
    from spotter_amd.jpeg import JpegEncoder

    return JpegEncoder(dev)


@pytest.fixture(scope="module")
def grouped():
    """{(quality, subsampling): [(id, rgb, Pillow's file)]} over every case, in table order."""
    out = {}
    for cid, rgb, q, sub in ec.all_cases():
        out.setdefault((q, sub), []).append((cid, rgb, ec.pillow(rgb, q, sub)))
    return out


def _dev(rgb, dev):
    return torch.from_numpy(np.ascontiguousarray(rgb)).to(dev)


def _same_files(got, want, names):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, names):
        assert isinstance(g, bytes), name
        if g != w:
            k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            raise AssertionError(f"{name}: {len(g)} bytes for {len(w)}, first difference at byte {k}")


# ------------------------------------------------------------------------------------------------------ bytes
@pytest.mark.parametrize("reverse", [False, True], ids=["table order", "reversed"])
def test_every_case_equals_pillow(dev, enc, grouped, reverse):
    for (q, sub), group in grouped.items():
        group = group[::-1] if reverse else group
        for k in range(0, len(group), SP_JPEG_BATCH_MAX):
            part = group[k:k + SP_JPEG_BATCH_MAX]
            got = enc.encode_many([_dev(rgb, dev) for _, rgb, _ in part], quality=q, subsampling=sub)
            _same_files(got, [w for _, _, w in part], [cid for cid, _, _ in part])


# ------------------------------------------------------------------------------------------------- boundaries
BOUNDARY_MCUS = (1, 3, 4, 5, 255, 256, 257, 1025)


@pytest.fixture(scope="module")
def boundary_images():
    imgs = [ec.mcu_count_image(n, 1, 1, 1, 100 + n) for n in BOUNDARY_MCUS]
    return imgs, [ec.pillow(im, 90, 0) for im in imgs]


def test_image_boundaries_inside_a_launch(dev, enc, boundary_images):
    imgs, want = boundary_images
    names = [f"{n} MCUs" for n in BOUNDARY_MCUS]
    before = dict(enc.stats)
    got = enc.encode_many([_dev(im, dev) for im in imgs], quality=90, subsampling=0)
    _same_files(got, want, names)
    got = enc.encode_many([_dev(im, dev) for im in imgs[::-1]], quality=90, subsampling=0)
    _same_files(got, want[::-1], names[::-1])
    assert enc.stats["chunks"] - before["chunks"] == 2 and enc.stats["images"] - before["images"] == 16


def test_64_one_mcu_images_and_a_single_image(dev, enc):
    rng = np.random.default_rng(64)
    imgs = [rng.integers(0, 256, (8, 8, 3), dtype=np.uint8) for _ in range(SP_JPEG_BATCH_MAX)]
    imgs[0][:] = 3  # the first, the middle and the last row of the search stand out from their neighbours
    imgs[31][:] = 200
    imgs[63][:] = 90
    got = enc.encode_many([_dev(im, dev) for im in imgs], quality=75, subsampling=0)
    _same_files(got, [ec.pillow(im, 75, 0) for im in imgs], [f"image {i}" for i in range(len(imgs))])
    one = rng.integers(0, 256, (37, 53, 3), dtype=np.uint8)
    assert enc.encode_many([_dev(one, dev)]) == [ec.pillow(one, 75, 2)]
    assert enc.encode_many([]) == []


# ----------------------------------------------------------------------------------------------------- stages
STAGE_CASES = ("geo 17x9 s2", "mcus 257 x1", "flat 77 s0", "runs gray 420", "mcus 5 x1", "sat noise q100 s0",
               "geo 1x1 s1", "mcus 1025 x5 420", "sat by q1 s1")


class BatchArena:
    """One device allocation filled with a position-dependent byte pattern:
    [guard 256][work: totals.work_bytes][guard 256] .. [guard 256][bits: totals.bits_cap][guard 256] and 512 spare
    bytes, work and bits 256-byte aligned; the table and `result` (pattern-filled too) are tensors of their own."""

    def __init__(self, dev, cases):
        self.n = n = len(cases)
        self.pixels = [_dev(rgb, dev) for _, rgb, _, _ in cases]
        self.lays = [_plan(rgb.shape[1], rgb.shape[0], q, sub) for _, rgb, q, sub in cases]
        self.items, self.totals = (SpJpegEncBatchItem * n)(), SpJpegEncBatchTotals()
        arr = (SpJpegEncLayout * n)(*self.lays)
        assert lib().sp_jpeg_enc_batch_plan(arr, n, self.items, C.byref(self.totals)) == 0, lib().sp_last_error()
        for it, px in zip(self.items, self.pixels):
            it.src, it.row_stride, it.pixel_bytes = px.data_ptr(), px.stride(0), 3
        t = self.totals
        self.work_off = GUARD
        self.bits_off = _up(self.work_off + t.work_bytes + GUARD, 256) + GUARD
        self.size = self.bits_off + t.bits_cap + GUARD + 512
        raw = torch.empty(self.size + 256, dtype=torch.uint8, device=dev)
        skew = -raw.data_ptr() % 256
        self.buf = raw[skew:skew + self.size]
        self.pattern = ((np.arange(self.size, dtype=np.int64) * 37 + 11) & 255).astype(np.uint8)
        self.buf.copy_(torch.from_numpy(self.pattern))
        self.result = torch.full((2 * n + 1,), -12345, dtype=torch.int64, device=dev)
        self.work_ptr = self.buf.data_ptr() + self.work_off
        self.bits_ptr = self.buf.data_ptr() + self.bits_off
        assert self.work_ptr % 256 == 0 and self.bits_ptr % 256 == 0

    def table(self, items=None):
        raw = np.frombuffer(bytes(self.items if items is None else items), dtype=np.uint8).copy()
        return torch.from_numpy(raw).to(self.buf.device)

    def run(self, items=None, totals=None, work_ptr=None, work_bytes=None, bits_cap=None, n=None):
        items = self.items if items is None else items
        self._table = self.table(items)  # kept alive until the caller has synchronised
        return lib().sp_jpeg_enc_batch_rgb(
            self._table.data_ptr(), items, self.n if n is None else n, C.byref(totals or self.totals),
            self.work_ptr if work_ptr is None else work_ptr,
            self.totals.work_bytes if work_bytes is None else work_bytes, self.bits_ptr,
            self.totals.bits_cap if bits_cap is None else bits_cap, self.result.data_ptr(),
            torch.cuda.current_stream().cuda_stream)

    def untouched(self):
        torch.cuda.synchronize()
        return (np.array_equal(self.buf.cpu().numpy(), self.pattern)
                and bool((self.result == -12345).all().item()))

    def copy_items(self):
        return (SpJpegEncBatchItem * self.n).from_buffer_copy(bytes(self.items))


@pytest.fixture(scope="module")
def stage_cases():
    return [ec.case_by_id(cid) for cid in STAGE_CASES]


def test_stages_equal_the_single_image_call(dev, stage_cases):
    ar = BatchArena(dev, stage_cases)
    assert ar.run() == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    host = ar.buf.cpu().numpy()
    res = ar.result.cpu().numpy()
    n, t = ar.n, ar.totals
    nbits, seg, used = res[:n], res[n:2 * n], int(res[2 * n])
    touched = np.zeros(ar.size, bool)  # every byte the call may have written
    pos = 0
    for i, (cid, rgb, q, sub) in enumerate(stage_cases):
        one = run_stages(dev, rgb, q, sub)
        it, lay = ar.items[i], ar.lays[i]
        nmcu = lay.mcux * lay.mcuy
        w0 = ar.work_off + it.work_off
        work = host[w0:w0 + lay.work_bytes]
        touched[w0:w0 + lay.work_bytes] = True
        coef_off = _up(8 + 12 * nmcu, 256)
        # the FDCT launch, the bit-count launch, the scan launch: the single-image call's workspace, array by array
        # (the padding between the counts and the coefficients belongs to neither)
        assert np.array_equal(work[coef_off:].view(np.int16).reshape(-1, 64), one.coefs), f"{cid}: coefficients"
        assert np.array_equal(work[8 + 8 * nmcu:8 + 12 * nmcu].view(np.int32), one.mbits), f"{cid}: MCU bit counts"
        assert np.array_equal(work[8:8 + 8 * nmcu].view(np.int64), one.off), f"{cid}: offsets"
        assert int(work[:8].view(np.int64)[0]) == one.total == one.nbits == int(nbits[i]), f"{cid}: total"
        assert np.array_equal(work[8 + 12 * nmcu:coef_off], ar.pattern[w0 + 8 + 12 * nmcu:w0 + coef_off]), cid
        # the packed layout: input order, multiples of 16, each part its zeroed words rounded up to 16
        zeroed = 4 * (-(-one.nbits // 32) + 1)
        assert int(seg[i]) == pos and pos % 16 == 0, f"{cid}: seg_off {int(seg[i])}, expected {pos}"
        assert zeroed <= lay.bits_cap
        b0 = ar.bits_off + pos
        nbytes = -(-one.nbits // 8)
        assert np.array_equal(host[b0:b0 + nbytes], one.bits[:nbytes]), f"{cid}: segment bytes"
        if one.nbits % 8:
            assert host[b0 + nbytes - 1] & (0xFF >> (one.nbits % 8)) == 0, f"{cid}: unused bits of the last byte"
        assert not host[b0 + nbytes:b0 + zeroed].any(), f"{cid}: zeroed words past the data"
        touched[b0:b0 + zeroed] = True
        pos += _up(zeroed, 16)
    assert used == pos and used <= t.bits_cap
    # guards, the gaps between the workspaces, the bytes between the segments beyond each one's zeroed words and the
    # rest of the packed buffer
    bad = np.flatnonzero((host != ar.pattern) & ~touched)
    assert bad.size == 0, f"{bad.size} bytes written outside the images' parts, first at {int(bad[0])}"


def test_refused_calls_launch_nothing(dev, stage_cases):
    L = lib()
    ar = BatchArena(dev, stage_cases[:4])

    def refused(what, **kw):
        assert ar.run(**kw) == -1, what
        msg = L.sp_last_error()
        assert ar.untouched(), what
        return msg

    it = ar.copy_items()
    it[2].work_off = it[1].work_off
    assert b"overlap" in refused("overlapping workspaces", items=it)
    it = ar.copy_items()
    it[3].first_wg_mcu += 1
    assert b"first workgroups" in refused("a wrong prefix entry", items=it)
    it = ar.copy_items()
    it[1].first_wg_fdct -= 1
    assert b"first workgroups" in refused("a wrong prefix entry", items=it)
    assert b"too small" in refused("a short packed buffer", bits_cap=ar.totals.bits_cap - 1)
    msg = refused("a short workspace", work_bytes=ar.totals.work_bytes - 1)  # the last range, or the total
    assert b"too small" in msg or b"outside work's" in msg
    assert b"misaligned" in refused("a misaligned workspace", work_ptr=ar.work_ptr + 16)
    it = ar.copy_items()
    it[1].work_off += 16
    assert b"misaligned" in refused("a misaligned workspace range", items=it)
    it = ar.copy_items()
    it[0].src = None
    assert b"null source" in refused("a NULL source", items=it)
    it = ar.copy_items()
    it[3].row_stride = 3 * it[3].lay.width - 1
    assert b"row_stride" in refused("a short row stride", items=it)
    it = ar.copy_items()
    it[0].lay.quant[1][7] += 1
    assert b"layout is not" in refused("a changed layout", items=it)
    tot = SpJpegEncBatchTotals.from_buffer_copy(bytes(ar.totals))
    tot.wg_fdct += 1
    assert b"totals" in refused("wrong totals", totals=tot)
    assert b"n = 0" in refused("n = 0", n=0)
    assert ar.run() == 0, L.sp_last_error()  # and the same arguments with nothing wrong pass
    torch.cuda.synchronize()
    assert int(ar.result[-1].item()) > 0


# ----------------------------------------------------------------------------------- stale buffers, source forms
def test_small_flat_images_after_large_noisy_ones(dev):
    from spotter_amd.jpeg import JpegEncoder

    e = JpegEncoder(dev)
    rng = np.random.default_rng(9)
    noisy = [rng.integers(0, 256, (200 + 8 * i, 264, 3), dtype=np.uint8) for i in range(4)]
    flat = [np.full((40, 56 + 8 * i, 3), 30 * i, np.uint8) for i in range(5)]
    _same_files(e.encode_many([_dev(im, dev) for im in noisy], quality=95, subsampling=0),
                [ec.pillow(im, 95, 0) for im in noisy], [f"noisy {i}" for i in range(4)])
    _same_files(e.encode_many([_dev(im, dev) for im in flat], quality=95, subsampling=0),
                [ec.pillow(im, 95, 0) for im in flat], [f"flat {i}" for i in range(5)])
    assert e.stats["chunks"] == 2 and e.stats["waits"] == 4


def test_source_forms_in_one_chunk_on_a_side_stream(dev, enc):
    from spotter_amd.draw import draw_module
    from spotter_amd.jpeg import DeviceRGBImage

    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, (45, 70, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (33, 41, 3), dtype=np.uint8)
    big = rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)
    d = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    p = rng.integers(0, 256, (29, 35, 3), dtype=np.uint8)
    rgbx = torch.full((33, 41, 4), 77, dtype=torch.uint8, device=dev)
    rgbx[..., :3] = _dev(b, dev)
    crop = _dev(big, dev)[7:50, 1:66]  # row stride 270 > 3 * 65, base address odd
    assert crop.stride(0) > 3 * crop.shape[1] and crop.data_ptr() % 2 == 1
    drawn = Image.fromarray(d.copy())
    ImageDraw.Draw(drawn).rectangle([3, 4, 40, 30], outline="red", width=3)
    pil = Image.fromarray(p)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        dimg = DeviceRGBImage(_dev(d, dev))
        draw_module().Draw(dimg).rectangle([3, 4, 40, 30], outline="red", width=3)
        assert len(dimg._draw_list) > 0  # still pending: encode_many flushes it
        got = enc.encode_many([_dev(a, dev), rgbx, crop, dimg, pil], quality=85, subsampling=1,
                              comments=[None, b"x", None, b"a comment", None])
        assert len(dimg._draw_list) == 0
    side.synchronize()

    def pillow(img, comment):
        buf = io.BytesIO()
        im = img if isinstance(img, Image.Image) else Image.fromarray(img)
        im.save(buf, "JPEG", quality=85, subsampling=1, **({"comment": comment} if comment else {}))
        return buf.getvalue()

    want = [pillow(a, None), pillow(b, b"x"), pillow(big[7:50, 1:66], None), pillow(drawn, b"a comment"),
            pillow(pil, None)]
    _same_files(got, want, ["packed RGB", "RGBX", "cropped view", "DeviceRGBImage", "PIL"])
    # and each is what encode() gives for the same source
    single = [enc.encode(s, 85, 1, c) for s, c in zip([_dev(a, dev), rgbx, crop, pil], [None, b"x", None, None])]
    assert single == [got[0], got[1], got[2], got[4]]


# --------------------------------------------------------------------------------------------------- chunking
def test_65_images_make_two_chunks(dev):
    from spotter_amd.jpeg import JpegEncoder

    e = JpegEncoder(dev)
    rng = np.random.default_rng(65)
    imgs = [rng.integers(0, 256, (9 + i % 5, 11 + i % 7, 3), dtype=np.uint8) for i in range(65)]
    got = e.encode_many([_dev(im, dev) for im in imgs])
    _same_files(got, [ec.pillow(im, 75, 2) for im in imgs], [f"image {i}" for i in range(65)])
    st = e.stats
    assert (st["calls"], st["chunks"], st["images"], st["single"], st["waits"]) == (1, 2, 65, 0, 4)
    assert st["d2h_bytes"] > 0 and st["h2d_bytes"] >= 65 * C.sizeof(SpJpegEncBatchItem)


def test_an_image_above_a_cap_takes_encode_and_caps_close_chunks(dev, monkeypatch):
    from spotter_amd import jpeg as J

    e = J.JpegEncoder(dev)
    rng = np.random.default_rng(3)
    small = [rng.integers(0, 256, (16, 16, 3), dtype=np.uint8) for _ in range(5)]
    large = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    cap_small, cap_large = (_plan(s, s, 75, 2).bits_cap for s in (16, 64))
    # two small images fit the packed capacity, three do not, the large one never does
    monkeypatch.setattr(J, "KEEP_ENC_BITS", 2 * J._a16(cap_small) + 8)
    assert cap_large > J.KEEP_ENC_BITS
    imgs = small[:3] + [large] + small[3:]
    got = e.encode_many([_dev(im, dev) for im in imgs])
    _same_files(got, [ec.pillow(im, 75, 2) for im in imgs], [f"image {i}" for i in range(len(imgs))])
    st = e.stats
    assert (st["chunks"], st["images"], st["single"]) == (3, 5, 1)  # [0, 1] [2] encode(3) [4, 5]


# ------------------------------------------------------------------------------------------------------- bulk
def _draw_as_detect(image, res, id2label, label_map):
    """serve.py:119-134 with the drop-in's ImageDraw."""
    from spotter_amd.draw import draw_module

    draw = draw_module().Draw(image)
    for lab, box in zip(res["labels"].tolist(), res["boxes"].tolist()):
        label = id2label[int(lab)]
        if label_map is not None:
            if label not in label_map:
                continue
            label = label_map[label]
        draw.rectangle(box, outline="red", width=3)
        draw.text(xy=(box[0] + 5, box[1] + 5), text=label, fill="white", stroke_width=1, stroke_fill="black")


@pytest.fixture(scope="module")
def bulk_setup(dev):
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.config import PRESETS
    from spotter_amd.synthetic import synthetic_image

    def jpeg(img, **kw):
        b = io.BytesIO()
        Image.fromarray(img).save(b, "JPEG", **kw)
        return b.getvalue()

    imgs = [synthetic_image(41, 120, 200), synthetic_image(42, 233, 177), synthetic_image(43, 64, 96)]
    b = io.BytesIO()
    Image.fromarray(synthetic_image(44, 50, 70)).save(b, "PNG")
    files = [jpeg(imgs[0], quality=90, subsampling=2, comment=b"from the camera"), b.getvalue(),
             b"\xff\xd8\xff\xe0 not a picture", jpeg(imgs[1], quality=85, subsampling=0),
             jpeg(imgs[2], quality=80, subsampling=1, progressive=True)]
    from spotter_amd.bulk import BulkDetector

    model = SpotterForObjectDetection(PRESETS["r18vd"], precision="fp32", use_graphs=False)
    proc = SpotterImageProcessor()
    plain = list(BulkDetector(model, proc, batch=2, threshold=0.0).detect(files))  # the unlabelled run, shared
    return files, model, proc, plain


@pytest.mark.parametrize("mapped", [False, True], ids=["every label", "label_map"])
def test_bulk_labelled_images_equal_the_one_image_path(dev, bulk_setup, mapped):
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.jpeg import open_image

    files, model, proc, plain = bulk_setup
    id2label = model.config.id2label
    label_map = None
    if mapped:  # the names of every other class the run detected, renamed
        seen = sorted({id2label[int(v)] for r in plain if "error" not in r for v in r["labels"].tolist()})
        label_map = {name: name.upper() + "!" for name in seen[::2]}
        assert label_map and len(label_map) < len(seen)
    det = BulkDetector(model, proc, batch=2, threshold=0.0, labelled=True, id2label=id2label, label_map=label_map)
    got = list(det.detect(files))
    assert len(got) == 5 and set(got[2]) == {"error"} and "jpeg" not in plain[0]
    assert len(det.stage_seconds["c"]) == len(det.stage_seconds["b"]) == 3
    for i in (0, 1, 3, 4):
        assert got[i]["size"] == plain[i]["size"] and len(got[i]["scores"]) > 0
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(got[i][k], plain[i][k]), (i, k)
        image = open_image(files[i]).convert("RGB")
        _draw_as_detect(image, got[i], id2label, label_map)
        buf = io.BytesIO()
        image.save(buf, format="JPEG")
        _same_files([got[i]["jpeg"]], [buf.getvalue()], [f"file {i}"])
    assert b"from the camera" in got[0]["jpeg"]
