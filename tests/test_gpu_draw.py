"""GPU: label drawing on the device image (sp_draw_rgb behind DeviceRGBImage / the drop-in's ImageDraw) against
Pillow's own ImageDraw on the same pixels, bit for bit; the whole serve.py tail without the pixels ever reaching
the host; copies, the processor, the hand-over to Pillow and the entry point's refusal of malformed tables."""
import base64
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
from draw_helpers import (AMENITY_TEXTS, OP_DT, SIZES, TILE_DT, coloured, execute, label as _label,  # noqa: E402
                          random_box as _box)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "test_pic.jpg")


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


@pytest.fixture
def launches(monkeypatch):
    """Counts the sp_draw_rgb calls made through the library handle."""
    from spotter_amd._lib import lib

    L = lib()
    real, calls = L.sp_draw_rgb, []

    def counted(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(L, "sp_draw_rgb", counted)
    return calls


def _device_pair(arr, dev, offset=None):
    """(Pillow image, DeviceRGBImage, their two draws, backing allocation) on the same pixels; offset: the tensor
    is a slice starting `offset` bytes into a larger allocation (guard bytes either side)."""
    from spotter_amd.draw import DeviceDraw, draw_module
    from spotter_amd.jpeg import DeviceRGBImage

    h, w, _ = arr.shape
    if offset is None:
        flat = t = torch.from_numpy(arr).to(dev)
    else:
        flat = torch.full((offset + arr.size + 7,), 0xA5, dtype=torch.uint8, device=dev)
        t = flat[offset:offset + arr.size].view(h, w, 3)
        t.copy_(torch.from_numpy(arr).to(dev))
    ref, im = Image.fromarray(arr), DeviceRGBImage(t)
    d = draw_module().Draw(im)
    assert type(d) is DeviceDraw and im._im is None
    return ref, im, ImageDraw.Draw(ref), d, flat


def _same(ref, im, what):
    assert im._im is None, what
    a, b = np.asarray(ref), im.spotter_device_rgb.cpu().numpy()
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_draws_pillows_pixels(dev, size):
    """The CPU test's sizes and mixes (labels as serve.py draws them, outlines of width 0/1/3/5, fills, boxes
    outside the image and narrower than the outline), rows of 21, 99 and 195 bytes among them; every second image
    is an unaligned slice of a larger allocation, whose guard bytes must stay untouched."""
    w, h = size
    rng = np.random.default_rng(w * 31 + h)
    for rep in range(6):
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        offset = (None, 1, None, 3, None, 4)[rep]
        ref, im, dr, dd, flat = _device_pair(arr, dev, offset)
        for k in range(int(rng.integers(4, 9))):
            _label((dr, dd), _box(rng, w, h, narrow=rep % 3 == 2), str(rng.choice(AMENITY_TEXTS)))
            box, width = _box(rng, w, h, narrow=True), (0, 1, 3, 5)[k % 4]
            for d in (dr, dd):
                if k % 2:
                    d.rectangle(box, outline=(200, 10, 30), width=width)
                else:
                    d.rectangle(box, fill=(1, 250, 99), outline="blue", width=width)
        _same(ref, im, f"{size} rep {rep} offset {offset}")
        if offset is not None:
            assert im.spotter_device_rgb.data_ptr() == flat.data_ptr() + offset  # drawn in place
            g = flat.cpu().numpy()
            assert np.all(g[:offset] == 0xA5) and np.all(g[offset + arr.size:] == 0xA5)


def test_coloured_inks_blend_as_pillow(dev):
    rng = np.random.default_rng(14)
    for rep in range(4):
        arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
        ref, im, dr, dd, _ = _device_pair(arr, dev, (None, 1)[rep % 2])
        coloured((dr, dd), 70)
        _same(ref, im, f"coloured inks, rep {rep}")


def test_order_in_one_flush(dev, launches):
    rng = np.random.default_rng(5)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    ref, im, dr, dd, _ = _device_pair(arr, dev)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "dining area")
    _label((dr, dd), [6.9, 9.1, 85.5, 60.0], "refrigerator")
    for d in (dr, dd):
        d.rectangle([0, 12, 89, 22], fill=(0, 90, 200))
    _label((dr, dd), [8.4, 8.4, 70.1, 33.3], "microwave")
    assert len(launches) == 0
    _same(ref, im, "order")
    assert len(launches) == 1


def test_serve_tail_never_leaves_the_device(dev, launches, monkeypatch):
    """serve.py:96-142 after the drop-in: Image.open → convert("RGB") → ImageDraw.Draw → 16 labels →
    save(format="JPEG") → base64 is the reference's string, with one sp_draw_rgb launch, no host pixels (load()
    never runs, `_im` stays None) and no pixel upload in the encoder."""
    from spotter_amd import jpeg
    from spotter_amd.draw import draw_module

    counts = {"load": 0, "upload": 0}
    real_load, real_pixels = jpeg.DeviceRGBImage.load, jpeg.pil_pixels

    def load(self):
        counts["load"] += 1
        return real_load(self)

    def pixels(im):
        counts["upload"] += 1
        return real_pixels(im)

    monkeypatch.setattr(jpeg.DeviceRGBImage, "load", load)
    monkeypatch.setattr(jpeg, "pil_pixels", pixels)
    Img, Draw = jpeg.image_module(dev), draw_module()
    data = open(GOLDEN, "rb").read()
    rng = np.random.default_rng(16)
    labels = []
    for i in range(16):
        x0, y0 = rng.uniform(-30, 1100), rng.uniform(-30, 650)
        labels.append(([x0, y0, x0 + rng.uniform(20, 500), y0 + rng.uniform(20, 400)], AMENITY_TEXTS[i % 15]))
    outs = []
    with Img.open(io.BytesIO(data)) as raw, Image.open(io.BytesIO(data)) as raw_ref:
        image, ref = raw.convert("RGB"), raw_ref.convert("RGB")
        assert isinstance(image, jpeg.DeviceRGBImage)
        for im, draw in ((image, Draw.Draw(image)), (ref, ImageDraw.Draw(ref))):
            for box, text in labels:
                _label((draw,), box, text)
            b = io.BytesIO()
            im.save(b, format="JPEG")
            outs.append(base64.b64encode(b.getvalue()).decode("utf-8"))
        assert outs[0] == outs[1]
        assert image._im is None and raw._im is None
        assert len(launches) == 1 and counts == {"load": 0, "upload": 0}


def test_copies_are_independent(dev):
    from spotter_amd.draw import draw_module

    Draw = draw_module()
    rng = np.random.default_rng(9)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    _, raw, _, _, _ = _device_pair(arr, dev)
    image = raw.convert("RGB")
    assert image._dev.data_ptr() == raw._dev.data_ptr()  # lazy: one tensor until somebody draws
    ref_copy, ref_raw = Image.fromarray(arr), Image.fromarray(arr)
    _label((Draw.Draw(image), ImageDraw.Draw(ref_copy)), [3.2, 4.7, 80.0, 40.0], "sofa")
    _same(ref_copy, image, "the copy")
    _same(ref_raw, raw, "the original after a draw on its copy")
    _label((Draw.Draw(raw), ImageDraw.Draw(ref_raw)), [20.5, 30.25, 88.0, 66.0], "oven")
    _same(ref_raw, raw, "the original")
    _same(ref_copy, image, "the copy after a draw on the original")
    again = image.copy()  # a copy of a drawn-on image carries the drawing
    _same(ref_copy, again, "a copy of the copy")


@pytest.mark.parametrize("how", ["copy", "convert"])
def test_copy_with_pending_draws_is_independent(dev, how):
    """Draw, copy with nothing reading the pixels in between, then draw on the original again and on the copy:
    the copy carries the first draw only, the original never shows the copy's, both equal Pillow's. With the
    original owning its tensor the pending draw is applied in place (no clone) and both then share that tensor."""
    from spotter_amd.draw import draw_module

    Draw = draw_module()
    rng = np.random.default_rng(13)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    ref_raw, raw, dr, dd, flat = _device_pair(arr, dev)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "sofa")
    assert len(raw._draw_list) > 0
    c = raw.copy() if how == "copy" else raw.convert("RGB")
    ref_c = ref_raw.copy()
    assert len(raw._draw_list) == 0 and c._im is None and raw._im is None
    assert c._dev.data_ptr() == raw._dev.data_ptr() == flat.data_ptr() and not raw._owns and not c._owns
    _label((dd, dr), [20.5, 30.25, 88.0, 66.0], "oven")  # the original's draw object, after the copy
    _label((Draw.Draw(c), ImageDraw.Draw(ref_c)), [10.75, 2.5, 60.0, 55.5], "bed")
    _same(ref_c, c, "the copy")
    _same(ref_raw, raw, "the original")
    assert c._dev.data_ptr() != raw._dev.data_ptr()
    # a second round on both, now that each owns its tensor
    _label((dd, dr), [1.5, 40.25, 50.0, 69.0], "TV")
    _label((Draw.Draw(c), ImageDraw.Draw(ref_c)), [45.0, 5.5, 89.0, 30.0], "sink")
    _same(ref_raw, raw, "the original, second round")
    _same(ref_c, c, "the copy, second round")


def test_processor_sees_the_drawn_pixels(dev):
    from spotter_amd import SpotterImageProcessor

    rng = np.random.default_rng(10)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    ref, im, dr, dd, _ = _device_pair(arr, dev)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "kitchen")
    proc = SpotterImageProcessor()
    a = proc(images=im)["pixel_values"]
    assert im._im is None
    b = proc(images=torch.from_numpy(np.asarray(ref).copy()).to(dev))["pixel_values"]
    assert torch.equal(a, b)
    assert not torch.equal(a, proc(images=torch.from_numpy(arr).to(dev))["pixel_values"])


def test_line_after_labels_falls_back_to_pillow(dev, launches):
    rng = np.random.default_rng(11)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    ref, im, dr, dd, _ = _device_pair(arr, dev)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "toaster")
    _label((dr, dd), [20.9, 15.1, 95.5, 60.0], "chair")
    for d in (dr, dd):
        d.line([2.5, 3, 80, 60], fill="yellow", width=2)
    assert im._im is not None and len(launches) == 1
    _label((dr, dd), [30.0, 30.5, 60.0, 66.0], "TV")
    assert np.array_equal(np.asarray(im), np.asarray(ref)) and len(launches) == 1
    a, b = io.BytesIO(), io.BytesIO()
    im.save(a, format="JPEG")  # a host-drawn image: its host pixels go up, as before
    ref.save(b, format="JPEG")
    assert a.getvalue() == b.getvalue()


def test_entry_point_applies_good_tables_and_refuses_malformed_ones(dev):
    """sp_draw_rgb on its own: a packed table gives the numpy executor's pixels; a table with an operation outside
    the image, a mask range outside the mask bytes or unordered tile ranges returns an error, launches nothing
    and leaves the image as it was."""
    from spotter_amd._lib import SpDrawTable, lib
    from spotter_amd.draw import DrawList

    L = lib()
    rng = np.random.default_rng(12)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    lst = DrawList(90, 70)
    lst.fill(3, 4, 80, 40, 0x0000FF)
    lst.blend(60, 30, bytes(rng.integers(0, 256, 400, dtype=np.uint8)), 20, 20, 0xFFFFFF)
    lst.blend(-5, -3, bytes(rng.integers(0, 256, 400, dtype=np.uint8)), 20, 20, 0x10C020)
    good = lst.packed()
    hd = SpDrawTable.from_buffer_copy(good)
    img = torch.from_numpy(arr).to(dev)

    def run(table):
        host = ctypes.create_string_buffer(bytes(table), len(table))
        table_dev = torch.frombuffer(bytearray(table), dtype=torch.uint8).to(dev)
        rc = L.sp_draw_rgb(img.data_ptr(), 70, 90, 270, host, table_dev.data_ptr(), len(table), None)
        torch.cuda.synchronize()
        return rc

    def patched(dt, off, idx, **fields):
        t = bytearray(good)
        a = np.frombuffer(t, dt, idx + 1, off)
        for k, v in fields.items():
            a[idx][k] = v
        return t

    for table in (patched(OP_DT, hd.ops_off, 0, x1=90), patched(OP_DT, hd.ops_off, 0, y1=70),
                  patched(OP_DT, hd.ops_off, 1, mask_off=401), patched(OP_DT, hd.ops_off, 2, mask_stride=40),
                  patched(TILE_DT, hd.tiles_off, 1, first=0), patched(TILE_DT, hd.tiles_off, 1, tx=0, ty=0)):
        assert run(table) < 0 and L.sp_last_error()
        assert np.array_equal(img.cpu().numpy(), arr)
    assert run(good) == 0, L.sp_last_error()
    want = arr.copy()
    execute(good, want)
    assert np.array_equal(img.cpu().numpy(), want) and not np.array_equal(want, arr)
