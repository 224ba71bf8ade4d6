"""GPU: the batched label draw (sp_draw_batch_rgb behind flush_many) against Pillow's own ImageDraw
on the same pixels and against the single-image path, bit for bit: one launch per group whatever the number of
images, image boundaries inside a launch, the batch limits, the entry point's refusals, staging reuse across streams,
encode_many over drawn images and the bulk pipeline with stage C inline and on its own thread and stream."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image, ImageDraw  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from draw_helpers import (AMENITY_TEXTS, OP_DT, SIZES, TILE_DT, execute, label as _label,  # noqa: E402
                          random_box as _box)


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


@pytest.fixture
def launches(monkeypatch):
    """Counts the sp_draw_rgb and sp_draw_batch_rgb calls made through the library handle."""
    from spotter_amd._lib import lib

    L = lib()
    calls = {"single": [], "batch": []}
    for key, name in (("single", "sp_draw_rgb"), ("batch", "sp_draw_batch_rgb")):
        def counted(*a, _real=getattr(L, name), _log=calls[key]):
            _log.append(a)
            return _real(*a)

        monkeypatch.setattr(L, name, counted)
    return calls


def _counts(launches):
    return len(launches["single"]), len(launches["batch"])


def _mix(rng, w, h, draws, rep=0):
    """The label and rectangle mix of tests/test_gpu_draw.py::test_kernel_draws_pillows_pixels on every draw of
    `draws` (labels as serve.py draws them, outlines of width 0 / 1 / 3 / 5, fills, boxes outside the image)."""
    for k in range(int(rng.integers(4, 9))):
        _label(draws, _box(rng, w, h, narrow=rep % 3 == 2), str(rng.choice(AMENITY_TEXTS)))
        box, width = _box(rng, w, h, narrow=True), (0, 1, 3, 5)[k % 4]
        for d in draws:
            if k % 2:
                d.rectangle(box, outline=(200, 10, 30), width=width)
            else:
                d.rectangle(box, fill=(1, 250, 99), outline="blue", width=width)
    for d in draws:  # (so that no image of a batch is left without a touched tile by chance)
        d.rectangle([0, 0, w - 1, h - 1], outline=(9, 8, 7), width=1)


def _pair(arr, dev, offset=None):
    """(Pillow image, DeviceRGBImage over the same pixels, backing allocation); offset: the tensor is a slice starting
    `offset` bytes into a larger allocation filled with 0xA5."""
    from spotter_amd.jpeg import DeviceRGBImage

    h, w, _ = arr.shape
    if offset is None:
        flat = t = torch.from_numpy(arr).to(dev)
    else:
        flat = torch.full((offset + arr.size + 7,), 0xA5, dtype=torch.uint8, device=dev)
        t = flat[offset:offset + arr.size].view(h, w, 3)
        t.copy_(torch.from_numpy(arr).to(dev))
    return Image.fromarray(arr), DeviceRGBImage(t), flat


def _drawn_set(dev, seed, sizes=SIZES, offsets=(None, 1, None, 3, None, 4, None)):
    """One drawn (reference, device image, allocation, offset, source array) per size; nothing flushed yet."""
    from spotter_amd.draw import DeviceDraw, draw_module

    rng = np.random.default_rng(seed)
    out = []
    for i, (w, h) in enumerate(sizes):
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref, im, flat = _pair(arr, dev, offsets[i % len(offsets)])
        d = draw_module().Draw(im)
        assert type(d) is DeviceDraw
        _mix(rng, w, h, (ImageDraw.Draw(ref), d), rep=i)
        assert len(im._draw_list) > 0 and im._im is None
        out.append((ref, im, flat, offsets[i % len(offsets)], arr))
    return out


def _pixels(im):
    assert im._im is None and len(im._draw_list) == 0
    return im._dev.cpu().numpy()


def test_seven_sizes_in_one_launch_draw_pillows_pixels(dev, launches):
    """1x1 to 90x70 (rows of 3 to 270 bytes, a one-pixel image, tiles cut on both axes), every second image an
    unaligned slice of a larger allocation: one sp_draw_batch_rgb, no sp_draw_rgb, Pillow's pixels, guards intact;
    and the same lists through flush() one by one on clones give the same tensors."""
    from spotter_amd.jpeg import DeviceRGBImage, flush_many

    items = _drawn_set(dev, 71)
    singles = []
    for _, im, _, _, _ in items:  # clones carrying the same lists, for the single-image path below
        c = DeviceRGBImage(im._dev.clone())
        c._draw_list.ops, c._draw_list.masks = list(im._draw_list.ops), list(im._draw_list.masks)
        c._draw_list.mask_bytes, c._draw_list._mask_at = im._draw_list.mask_bytes, dict(im._draw_list._mask_at)
        singles.append(c)
    flush_many([im for _, im, _, _, _ in items])
    assert _counts(launches) == (0, 1) and launches["batch"][0][2] == len(SIZES)
    for (ref, im, flat, offset, arr), (w, h) in zip(items, SIZES):
        got = _pixels(im)
        bad = np.argwhere(np.asarray(ref) != got)
        assert bad.size == 0, f"{w}x{h}: {len(bad)} samples differ, first at {bad[:3].tolist()}"
        if offset is not None:
            assert im._dev.data_ptr() == flat.data_ptr() + offset  # drawn in place
            g = flat.cpu().numpy()
            assert np.all(g[:offset] == 0xA5) and np.all(g[offset + arr.size:] == 0xA5)
    for c, (_, im, _, _, _) in zip(singles, items):
        c.flush()
        assert torch.equal(c._dev, im._dev)
    assert _counts(launches) == (len(SIZES), 1)


def test_image_boundaries_inside_one_launch(dev, launches):
    """Images carved back to back out of one arena, as decode_many returns them: one with a single touched tile
    between two with many, one without draws (left out, unchanged); every byte between and around them is unchanged."""
    from spotter_amd.draw import draw_module
    from spotter_amd.jpeg import DeviceRGBImage, flush_many

    rng = np.random.default_rng(72)
    sizes = [(200, 40), (30, 6), (130, 33), (64, 8), (70, 20)]  # (30, 6) is one tile; (64, 8) gets no draws
    host = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    arena = torch.from_numpy(host.copy()).to(dev)
    want = host.copy()
    ims, off, spans = [], 5, []
    for i, (w, h) in enumerate(sizes):
        n = 3 * w * h
        im = DeviceRGBImage(arena[off:off + n].view(h, w, 3))
        ref = Image.fromarray(want[off:off + n].reshape(h, w, 3).copy())
        if (w, h) != (64, 8):
            _mix(rng, w, h, (ImageDraw.Draw(ref), draw_module().Draw(im)), rep=i)
            want[off:off + n] = np.asarray(ref).reshape(-1)
        ims.append(im)
        spans.append((off, off + n))
        off += n + (0, 1, 0, 3, 0)[i]  # back to back, or a byte or three of somebody else's in between
    from spotter_amd._lib import SpDrawTable

    tiles = [SpDrawTable.from_buffer_copy(im._draw_list.packed()).n_tiles if len(im._draw_list) else 0 for im in ims]
    assert tiles[1] == 1 and tiles[0] > 4 and tiles[2] > 4 and tiles[3] == 0
    flush_many(ims)
    assert _counts(launches) == (0, 1) and launches["batch"][0][2] == 4  # the image without draws is not in the table
    got = arena.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {bad[:5].tolist()} (images at {spans})"
    assert not np.array_equal(got, host)
    assert all(im._dev.data_ptr() == arena.data_ptr() + a for im, (a, _) in zip(ims, spans))  # in place, no clone


@pytest.mark.parametrize("n", [1, 64, 65])
def test_batch_limits(dev, launches, n):
    """64 one-pixel images go in one launch, 65 in two, one image alone in one."""
    from spotter_amd.draw import draw_module
    from spotter_amd.jpeg import DeviceRGBImage, flush_many

    rng = np.random.default_rng(n)
    arr = rng.integers(0, 256, (n, 1, 1, 3), dtype=np.uint8)
    inks = rng.integers(0, 256, (n, 3))
    ims = [DeviceRGBImage(torch.from_numpy(arr[i]).to(dev)) for i in range(n)]
    want = arr.copy()
    for i, im in enumerate(ims):
        ref = Image.fromarray(arr[i])
        for d in (draw_module().Draw(im), ImageDraw.Draw(ref)):
            d.rectangle([0, 0, 0, 0], fill=tuple(int(v) for v in inks[i]))
            if i % 2 == 0:  # and the corner of a label's mask blended over it
                d.text((-2.5 - i % 3, -3.25), "TV", fill=(250, 240, 230), stroke_width=1, stroke_fill=(9, 9, 9))
        want[i] = np.asarray(ref)
        assert len(im._draw_list) > 0
    flush_many(ims)
    # (flush_many sends a single image, and the 65th, through the batch entry point as well)
    assert _counts(launches) == (0, 2 if n == 65 else 1) and sum(c[2] for c in launches["batch"]) == n
    got = np.stack([_pixels(im) for im in ims])
    assert np.array_equal(got, want) and not np.array_equal(got, arr)


def test_refused_calls_launch_nothing(dev):
    """sp_draw_batch_rgb on its own over three images: a good table gives the numpy executor's pixels; every malformed
    form returns < 0 with a message and leaves all pixels as they were."""
    from spotter_amd._lib import SP_DRAW_BATCH_MAX, SpDrawBatchItem, SpDrawTable, lib
    from spotter_amd.draw import DrawList

    L = lib()
    rng = np.random.default_rng(73)
    shapes = [(40, 30), (90, 70), (64, 8)]  # (width, height)
    arrs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in shapes]
    imgs = [torch.from_numpy(a).to(dev) for a in arrs]
    tables = []
    for w, h in shapes:
        lst = DrawList(w, h)
        lst.fill(3, 4, w - 10, h - 30 if h > 40 else h - 2, 0x0000FF)
        # (on the 90x70 image the three operations are those of tests/test_gpu_draw.py's entry point test: this mask
        # lies whole inside the image, so that one byte more of mask_off reads past the mask bytes)
        lst.blend(w - 30, 30 if h > 50 else h - 8, bytes(rng.integers(0, 256, 400, dtype=np.uint8)), 20, 20, 0xFFFFFF)
        lst.blend(-5, -3, bytes(rng.integers(0, 256, 400, dtype=np.uint8)), 20, 20, 0x10C020)
        tables.append(lst.packed())
    offs = [0, len(tables[0]), len(tables[0]) + len(tables[1])]
    good_buf = b"".join(tables)

    def rows(n=3):
        items = (SpDrawBatchItem * max(n, 1))()
        wg = 0
        for i in range(min(n, 3)):
            it, hd = items[i], SpDrawTable.from_buffer_copy(tables[i])
            (w, h), it.rgb = shapes[i], imgs[i].data_ptr()
            it.height, it.width, it.row_stride = h, w, 3 * w
            it.table_off, it.table_bytes, it.n_tiles, it.first_wg = offs[i], len(tables[i]), hd.n_tiles, wg
            wg += hd.n_tiles
        return items

    def run(items, n=3, buf=good_buf):
        host = ctypes.create_string_buffer(bytes(buf), len(buf))
        up = bytes(buf) + bytes(items)
        both = torch.frombuffer(bytearray(up), dtype=torch.uint8).to(dev)
        rc = L.sp_draw_batch_rgb(both.data_ptr() + len(buf), items, n, host, both.data_ptr(), len(buf), None)
        torch.cuda.synchronize()
        return rc

    def unchanged():
        return all(np.array_equal(t.cpu().numpy(), a) for t, a in zip(imgs, arrs))

    def refused(items, n=3, buf=good_buf, what=""):
        assert run(items, n, buf) < 0 and L.sp_last_error(), what
        assert unchanged(), what

    assert len(good_buf) % 16 == 0 and all(o % 16 == 0 for o in offs)
    refused(rows(), n=0, what="n = 0")
    refused(rows(SP_DRAW_BATCH_MAX + 1), n=SP_DRAW_BATCH_MAX + 1, what="n = 65")
    for field, delta in (("first_wg", 1), ("first_wg", -1), ("n_tiles", 1), ("n_tiles", -1), ("table_off", 8),
                         ("height", 1), ("row_stride", -1)):
        items = rows()
        setattr(items[1], field, getattr(items[1], field) + delta)
        refused(items, what=f"{field} {delta:+d}")
    items = rows()
    items[2].first_wg += 1  # the last row's, which no later row would contradict
    refused(items, what="last first_wg")
    items = rows()  # overlapping tables: row 2 reads row 1's table (same shape needed, so give it row 1's shape too)
    items[2].table_off, items[2].table_bytes = items[1].table_off, items[1].table_bytes
    items[2].height, items[2].width, items[2].row_stride = items[1].height, items[1].width, items[1].row_stride
    items[2].rgb = torch.zeros(70 * 90 * 3, dtype=torch.uint8, device=dev).data_ptr()
    items[2].n_tiles = items[1].n_tiles
    refused(items, what="overlapping tables")
    items = rows()
    items[1].table_bytes += 16  # reaches into the next table
    refused(items, what="table ranges overlap by 16 bytes")
    items = rows()
    items[2].table_bytes = len(good_buf)  # past the end of the buffer
    refused(items, what="table past the buffer")
    # two rows over overlapping pixels: row 2 (64x8) placed inside row 1's image
    items = rows()
    items[2].rgb = imgs[1].data_ptr() + 3 * 90 * 69  # its first row is row 1's last
    refused(items, what="overlapping pixels")
    items = rows()
    items[0].rgb = None
    refused(items, what="null pixels")

    # each malformed-table form of test_entry_point_applies_good_tables_and_refuses_malformed_ones, in row 1
    hd = SpDrawTable.from_buffer_copy(tables[1])

    def patched(dt, off, idx, **fields):
        t = bytearray(good_buf)
        a = np.frombuffer(t, dt, idx + 1, offs[1] + off)
        for k, v in fields.items():
            a[idx][k] = v
        return t

    for what, buf in (("x1", patched(OP_DT, hd.ops_off, 0, x1=90)), ("y1", patched(OP_DT, hd.ops_off, 0, y1=70)),
                      ("mask_off", patched(OP_DT, hd.ops_off, 1, mask_off=401)),
                      ("mask_stride", patched(OP_DT, hd.ops_off, 2, mask_stride=40)),
                      ("tile first", patched(TILE_DT, hd.tiles_off, 1, first=0)),
                      ("tile twice", patched(TILE_DT, hd.tiles_off, 1, tx=0, ty=0))):
        assert run(rows(), buf=buf) < 0 and b"image 1" in L.sp_last_error(), what
        assert unchanged(), what

    assert run(rows()) == 0, L.sp_last_error()
    for t, a, table in zip(imgs, arrs, tables):
        want = a.copy()
        execute(table, want)
        assert np.array_equal(t.cpu().numpy(), want) and not np.array_equal(want, a)


def test_side_stream_and_staging_reuse(dev, launches):
    """Two flush_many calls back to back on a non-default stream, the second with a table larger than the staging
    buffers hold, so they are replaced while the first launch may still be in flight: both results are Pillow's."""
    from spotter_amd import jpeg
    from spotter_amd.draw import draw_module

    stage = jpeg._draw_stage(dev)
    torch.cuda.synchronize()
    stage._stage = stage._table = None  # start from nothing: the first call allocates the 1 MiB minimum
    small = _drawn_set(dev, 74)
    rng = np.random.default_rng(75)
    big = []
    for i in range(3):  # three 700x500 images, each with a full-image ramp bitmap: 350 000 mask bytes apiece
        arr = rng.integers(0, 256, (500, 700, 3), dtype=np.uint8)
        ref, im, _ = _pair(arr, dev)
        ramp = Image.fromarray(rng.integers(0, 256, (500, 700), dtype=np.uint8), "L")
        for d in (ImageDraw.Draw(ref), draw_module().Draw(im)):
            d.bitmap((i - 1, 1 - i), ramp, fill=(200 - i, 100, 50 + i))
            _label((d,), [20.5 + i, 30.25, 600.0, 400.0], "dining area")
        assert im._im is None
        big.append((ref, im))
    before = dict(stage.stats)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        jpeg.flush_many([im for _, im, _, _, _ in small])
        first = stage._stage
        jpeg.flush_many([im for _, im in big])
    side.synchronize()
    assert stage._stage is not first and stage._stage.numel() > 1 << 20
    assert _counts(launches) == (0, 2)
    assert stage.stats["batch_launches"] == before["batch_launches"] + 2
    assert stage.stats["batch_images"] == before["batch_images"] + len(small) + 3
    assert stage.stats["batch_h2d_bytes"] > before["batch_h2d_bytes"] + 3 * 350000
    for ref, im, _, _, _ in small:
        assert np.array_equal(np.asarray(ref), _pixels(im))
    for ref, im in big:
        assert np.array_equal(np.asarray(ref), _pixels(im))


def test_encode_many_flushes_the_drawn_images_with_one_launch(dev, launches):
    """Three drawn DeviceRGBImages, one undrawn tensor and one PIL image in one encode_many: Pillow's save of the
    Pillow-drawn references, one batch draw launch."""
    from spotter_amd.draw import draw_module
    from spotter_amd.jpeg import JpegEncoder

    rng = np.random.default_rng(76)
    srcs, refs = [], []
    for i, (w, h) in enumerate([(90, 70), (33, 17), (200, 120)]):
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref, im, _ = _pair(arr, dev)
        _mix(rng, w, h, (ImageDraw.Draw(ref), draw_module().Draw(im)), rep=i)
        srcs.append(im), refs.append(ref)
    plain = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)
    srcs.append(torch.from_numpy(plain).to(dev)), refs.append(Image.fromarray(plain))
    pil = Image.fromarray(rng.integers(0, 256, (24, 31, 3), dtype=np.uint8))
    ImageDraw.Draw(pil).rectangle([2, 3, 20, 15], outline="red", width=3)
    srcs.append(pil), refs.append(pil)
    files = JpegEncoder(dev).encode_many(srcs)
    assert _counts(launches) == (0, 1) and launches["batch"][0][2] == 3
    for k, (got, ref) in enumerate(zip(files, refs)):
        b = io.BytesIO()
        ref.save(b, format="JPEG")
        assert got == b.getvalue(), f"source {k}"


# ------------------------------------------------------------------------------------------------------- bulk
@pytest.fixture(scope="module")
def bulk_setup(dev):
    """The five files and the r18vd fp32 model of tests/test_gpu_jpeg_enc_batch.py's bulk test (3 chunks of 2: a PNG,
    a refused file, a progressive file), the unlabelled run and the one-image path's labelled files, made once."""
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.config import PRESETS
    from spotter_amd.draw import draw_module
    from spotter_amd.jpeg import open_image
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
    model = SpotterForObjectDetection(PRESETS["r18vd"], precision="fp32", use_graphs=False)
    proc = SpotterImageProcessor()
    plain = list(BulkDetector(model, proc, batch=2, threshold=0.0).detect(files))
    id2label = model.config.id2label
    want = {}
    for i in (0, 1, 3, 4):  # serve.py:96-142 with the drop-in, one image at a time
        image = open_image(files[i]).convert("RGB")
        draw = draw_module().Draw(image)
        for lab, box in zip(plain[i]["labels"].tolist(), plain[i]["boxes"].tolist()):
            draw.rectangle(box, outline="red", width=3)
            draw.text(xy=(box[0] + 5, box[1] + 5), text=id2label[int(lab)], fill="white", stroke_width=1,
                      stroke_fill="black")
        buf = io.BytesIO()
        image.save(buf, format="JPEG")
        want[i] = buf.getvalue()
    return files, model, proc, plain, want


@pytest.mark.parametrize("overlap", [False, True], ids=["inline", "overlapped"])
def test_bulk_batched_labels_equal_the_one_image_path(dev, bulk_setup, launches, overlap):
    from spotter_amd.bulk import BulkDetector

    files, model, proc, plain, want = bulk_setup
    det = BulkDetector(model, proc, batch=2, threshold=0.0, labelled=True, id2label=model.config.id2label,
                       label_draw="batched", label_overlap=overlap)
    for _ in range(2):  # the second run replays the stamps the first one learned
        del launches["single"][:], launches["batch"][:]
        got = list(det.detect(files))
        assert len(got) == 5 and set(got[2]) == {"error"}
        assert len(det.stage_seconds["a"]) == len(det.stage_seconds["b"]) == len(det.stage_seconds["c"]) == 3
        for i in (0, 1, 3, 4):
            assert got[i]["size"] == plain[i]["size"] and len(got[i]["scores"]) > 0
            for k in ("scores", "labels", "boxes"):
                assert torch.equal(got[i][k], plain[i][k]), (i, k)
            assert got[i]["jpeg"] == want[i], f"file {i}: {len(got[i]['jpeg'])} bytes against {len(want[i])}"
        # chunks [0, 1] [refused, 3] [4]: one batch launch each, of 2, 1 and 1 images; no single-image launch
        assert _counts(launches) == (0, 3) and [c[2] for c in launches["batch"]] == [2, 1, 1]
    assert b"from the camera" in got[0]["jpeg"]
