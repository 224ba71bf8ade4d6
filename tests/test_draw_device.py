"""CPU: the recording half of the GPU label drawing (spotter_amd/draw.py DeviceDraw / DrawList, sp_draw_pack).

A stand-in image carries a numpy array where DeviceRGBImage carries its device tensor, and "flushes" by
interpreting the packed table (operations, tile bins, mask bytes — exactly what sp_draw_rgb's kernel reads) with
the numpy executor of tests/draw_helpers.py (shared with the GPU tests, as are the label and box generators),
tile by tile, each tile's operations in list order. What comes out must be Pillow's pixels for the same calls:
Pillow's own ImageDraw on the same array is the judge."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image, ImageDraw

sys.path.insert(0, os.path.dirname(__file__))
from draw_helpers import (AMENITY_TEXTS, OP_DT, SIZES, TILE_DT, coloured, execute, label as _label,  # noqa: E402
                          random_box as _box)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StandIn(Image.Image):
    """What DeviceDraw needs of a device image, without a device: `_draw_list`, `_im`, load()."""

    def __init__(self, arr):
        from spotter_amd.draw import DrawList

        super().__init__()
        self._mode, self._size = "RGB", (arr.shape[1], arr.shape[0])
        self._arr = arr.copy()
        self._draw_list = DrawList(*self._size)
        self.flushes = 0

    def flush(self):
        if len(self._draw_list):
            execute(self._draw_list.packed(), self._arr)
            self._draw_list.clear()
            self.flushes += 1

    def load(self):
        if self._im is None:
            self.flush()
            self.im = Image.fromarray(self._arr).im
        return super().load()

    def pixels(self):
        if self._im is not None:
            return np.asarray(self)
        self.flush()
        return self._arr


def _pair(rng, w, h):
    from spotter_amd.draw import DeviceDraw, draw_module

    arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ref, dev = Image.fromarray(arr), StandIn(arr)
    d = draw_module().Draw(dev)
    assert type(d) is DeviceDraw and isinstance(d, ImageDraw.ImageDraw) and dev._im is None
    return ref, dev, ImageDraw.Draw(ref), d


def _same(ref, dev, what):
    a, b = np.asarray(ref), dev.pixels()
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_recorded_labels_equal_pillows(size):
    """4-8 overlapping labels per image as serve.py draws them, every amenity string, random float boxes (partly
    or wholly outside, negative, narrower than twice the outline): one flush per image."""
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    texts = list(AMENITY_TEXTS)
    for rep in range(12):
        ref, dev, dr, dd = _pair(rng, w, h)
        for k in range(int(rng.integers(4, 9))):
            text = texts.pop() if texts else str(rng.choice(AMENITY_TEXTS))
            _label((dr, dd), _box(rng, w, h, narrow=rep % 3 == 2), text)
        assert dev._im is None
        _same(ref, dev, f"{size} rep {rep}")
        assert dev.flushes <= 1 and dev._im is None
    assert not texts


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_recorded_rectangles_equal_pillows(size):
    """Single outlines of width 0, 1, 3, 5 and filled rectangles, boxes narrower than 6 pixels included, through
    ImageDraw.rectangle and (width 0 means 1 there) straight through the core object's draw_rectangle."""
    w, h = size
    rng = np.random.default_rng(w * 77 + h)
    for rep in range(150):
        ref, dev, dr, dd = _pair(rng, w, h)
        box = _box(rng, w, h, narrow=rep % 2 == 0)
        if rep % 5 == 0:
            box = [float(int(v)) for v in box]
        width = (0, 1, 3, 5)[rep % 4]
        kind = rep % 3
        for d in (dr, dd):
            if kind == 0:
                d.rectangle(box, outline=(200, 10, 30), width=width)
            elif kind == 1:
                d.rectangle([tuple(box[:2]), tuple(box[2:])], fill=(1, 250, 99), outline="blue", width=width)
            else:
                d.draw.draw_rectangle(box, d.draw.draw_ink((9, 8, 7)), 0, width)
        _same(ref, dev, f"{size} rep {rep} box {box} width {width} kind {kind}")
    assert dev._im is None


def test_order_is_kept_per_pixel():
    rng = np.random.default_rng(5)
    ref, dev, dr, dd = _pair(rng, 90, 70)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "dining area")
    _label((dr, dd), [6.9, 9.1, 85.5, 60.0], "refrigerator")
    for d in (dr, dd):
        d.rectangle([0, 12, 89, 22], fill=(0, 90, 200))
    _label((dr, dd), [8.4, 8.4, 70.1, 33.3], "microwave")
    _same(ref, dev, "order")
    assert dev.flushes == 1


def test_coloured_inks_blend_as_pillow():
    rng = np.random.default_rng(14)
    for rep in range(4):
        ref, dev, dr, dd = _pair(rng, 90, 70)
        coloured((dr, dd), 70)
        _same(ref, dev, f"coloured inks, rep {rep}")
        assert dev._im is None


def test_errors_are_raised_at_the_call():
    rng = np.random.default_rng(6)
    ref, dev, dr, dd = _pair(rng, 33, 17)
    for d in (dr, dd):
        with pytest.raises(ValueError, match="x1 must be greater than or equal to x0"):
            d.rectangle([10, 2, 9.5, 8], outline="red", width=3)
        with pytest.raises(ValueError, match="y1 must be greater than or equal to y0"):
            d.rectangle([1, 8, 9, 7.5], fill="red")
        with pytest.raises(ValueError):
            d.rectangle([1, 2, 3, 4], outline="no such colour")
        with pytest.raises(ValueError):
            d.rectangle([1, 2, 3], outline="red")
    assert len(dev._draw_list) == 0 and dev._im is None
    _same(ref, dev, "after errors")


def _handover_case(name, dr, dd):
    if name == "line":
        for d in (dr, dd):
            d.line([2.5, 3, 80, 60], fill="yellow", width=2)
    elif name == "ellipse":
        for d in (dr, dd):
            d.ellipse([10, 5, 70, 50], outline="green", width=2)
    else:
        for d in (dr, dd):
            d.text((12.3, 20.6), "sofa", fill=(250, 240, 20), embedded_color=True, stroke_width=1, stroke_fill="black")


@pytest.mark.parametrize("name", ["line", "ellipse", "embedded_color"])
def test_other_calls_hand_over_to_pillow(name):
    """Calls the recorder does not implement flush what was recorded, load the image and go to Pillow's core
    object, as do all later ones: the final pixels are Pillow's for the same sequence."""
    rng = np.random.default_rng(7)
    ref, dev, dr, dd = _pair(rng, 90, 70)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "hair dryer")
    _label((dr, dd), [20.9, 15.1, 95.5, 60.0], "bathroom")
    assert dev._im is None and len(dev._draw_list) > 0
    _handover_case(name, dr, dd)
    assert dev._im is not None and dev.flushes == 1 and len(dev._draw_list) == 0
    _label((dr, dd), [30.0, 30.5, 60.0, 66.0], "TV")
    assert len(dev._draw_list) == 0
    _same(ref, dev, name)


def test_rgba_mode_and_later_pillow_draws_hand_over():
    from spotter_amd.draw import DeviceDraw, draw_module

    rng = np.random.default_rng(8)
    ref, dev, dr, dd = _pair(rng, 90, 70)
    _label((dr, dd), [3.2, 4.7, 80.0, 40.0], "workspace")
    d2 = draw_module().Draw(dev, "RGBA")
    assert type(d2) is ImageDraw.ImageDraw and dev._im is not None and dev.flushes == 1
    r2 = ImageDraw.Draw(ref, "RGBA")
    for d in (r2, d2):
        d.rectangle([10, 10, 60, 50], fill=(255, 0, 0, 90))
    # the first draw object now finds the image loaded: its later calls go to Pillow too
    _label((dr, dd), [40.0, 20.5, 88.0, 66.0], "parking")
    assert len(dev._draw_list) == 0 and type(draw_module().Draw(dev)) is not DeviceDraw
    _same(ref, dev, "RGBA")


def test_mask_bytes_are_kept_only_with_the_memo_fonts_own_masks():
    """The bytes of a blended mask are kept exactly as long as the memoising default font keeps the mask itself
    (its memo and its bounded exact cache): another font's fresh renders and a caller's bitmap are read every
    time and nothing of them is retained; a bitmap changed between two draws draws its new content."""
    from PIL import ImageFont

    from spotter_amd.draw import _MemoFont, memo_default_font

    font = memo_default_font()
    assert isinstance(font, _MemoFont)
    rng = np.random.default_rng(9)
    ref, dev, dr, dd = _pair(rng, 90, 70)
    for _ in range(3):
        _label((dr, dd), [3.25, 4.5, 80.0, 40.0], "chair")
    held = {id(v[0]) for v in font._exact.values()} | {id(v[0]) for v in font._memo.values()}
    assert set(font._held) == held and font._memo_ids == {id(v[0]) for v in font._memo.values()}
    assert sum(b is not None for b in font._held.values()) >= 2  # the stroke and the fill of "chair"
    before = dict(font._held)
    own = ImageFont.load_default()
    bmp = Image.new("L", (9, 7), 0)
    for i in range(4):
        bmp.paste(60 * i + 20, (i, i, i + 3, i + 3))  # the caller's bitmap changes between the draws
        for d in (dr, dd):
            d.text((5.5 + i, 30.25), "oven", font=own, fill="white", stroke_width=1, stroke_fill="black")
            d.bitmap((40 + 10 * i, 50), bmp, fill=(10 * i, 200, 90))
    assert font._held == before and dev._im is None
    _same(ref, dev, "own font and bitmaps")
    small = ImageFont.load_default()
    small.__class__ = _MemoFont
    small._memo_init()
    small.EXACT_CAP = 4
    kw = dict(direction=None, features=None, language=None, stroke_width=0, stroke_filled=True, anchor="la", ink=255)
    for i in range(12):
        m, _ = small.getmask2(f"bed {i}", "L", start=(0.3, 0.3), **kw)
        assert small.mask_bytes(m) == bytes(m)
    assert len(small._held) == len(small._exact) == 4  # evicted masks take their bytes with them
    assert small.mask_bytes(own.getmask2("bed", "L", start=(0.3, 0.3), **kw)[0]) is None


def test_shim_on_a_plain_image_is_pillows_draw():
    from spotter_amd.draw import DeviceDraw, draw_module, memo_default_font

    im, ref = Image.new("RGB", (40, 30), (5, 6, 7)), Image.new("RGB", (40, 30), (5, 6, 7))
    d = draw_module().Draw(im)
    assert type(d) is ImageDraw.ImageDraw and not isinstance(d, DeviceDraw)
    assert d.font is memo_default_font() and d.im is im.im
    _label((ImageDraw.Draw(ref), d), [2.5, 3.5, 30, 25], "bed")
    assert np.array_equal(np.asarray(im), np.asarray(ref))


def test_ctypes_draw_structs_match_the_header_layout(tmp_path):
    from spotter_amd import _lib
    from spotter_amd.draw import _OP

    structs = {"sp_draw_op": _lib.SpDrawOp, "sp_draw_tile": _lib.SpDrawTile, "sp_draw_table": _lib.SpDrawTable}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spotter_hip.h"', "int main(void) {"]
    for cname, py in structs.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('  printf("tile w %d\\n  tile h %d\\n", SP_DRAW_TILE_W, SP_DRAW_TILE_H);')
    lines.append('  printf("kind fill %d\\n  kind blend %d\\n", SP_DRAW_FILL, SP_DRAW_BLEND);')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        cname, f, v = ln.split()
        got[(cname, f)] = int(v)
    for cname, py in structs.items():
        assert got[(cname, "sizeof")] == ctypes.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert (got[("tile", "w")], got[("tile", "h")]) == (_lib.SP_DRAW_TILE_W, _lib.SP_DRAW_TILE_H)
    assert (got[("kind", "fill")], got[("kind", "blend")]) == (_lib.SP_DRAW_FILL, _lib.SP_DRAW_BLEND)
    # the recorder's packed record and the numpy view of it are that struct
    assert _OP.size == ctypes.sizeof(_lib.SpDrawOp) == OP_DT.itemsize
    op = _lib.SpDrawOp.from_buffer_copy(_OP.pack(1, 2, 3, 4, 5, 0xA0B0C0, 1 << 40, 7, 8, 9, 0))
    assert [getattr(op, f) for f, _ in op._fields_] == [1, 2, 3, 4, 5, 0xA0B0C0, 1 << 40, 7, 8, 9, 0]
    for f, _ in _lib.SpDrawOp._fields_:
        assert OP_DT.fields[f][1] == getattr(_lib.SpDrawOp, f).offset, f


def test_malformed_tables_are_refused_without_a_gpu():
    """sp_draw_rgb validates the packed table on the host before it launches anything: an operation outside the
    image, a mask range outside the mask bytes, unordered tile ranges each return < 0 with a message."""
    from spotter_amd import _lib
    from spotter_amd.draw import DrawList

    L = _lib.load()
    lst = DrawList(90, 70)
    lst.fill(3, 4, 80, 40, 0x0000FF)
    lst.blend(60, 30, bytes(range(200)), 20, 10, 0xFFFFFF)
    good = lst.packed()
    hd = _lib.SpDrawTable.from_buffer_copy(good)
    assert hd.n_ops == 2 and hd.n_tiles > 2

    def run(table, h=70, w=90):
        buf = ctypes.create_string_buffer(bytes(table), len(table))
        return L.sp_draw_rgb(ctypes.c_void_p(256), h, w, w * 3, buf, ctypes.c_void_p(256), len(table), None)

    def patched(dt, off, idx, **fields):
        t = bytearray(good)
        a = np.frombuffer(t, dt, idx + 1, off)
        for k, v in fields.items():
            a[idx][k] = v
        return t

    cases = {
        "outside": patched(OP_DT, hd.ops_off, 0, x1=90),
        "outside the": patched(OP_DT, hd.ops_off, 0, y0=-1),
        "mask byte": patched(OP_DT, hd.ops_off, 1, mask_off=5),
        "mask": patched(OP_DT, hd.ops_off, 1, sy=1),
        "negative mask": patched(OP_DT, hd.ops_off, 1, sx=-1),
        "kind": patched(OP_DT, hd.ops_off, 1, kind=2),
        "unordered reference range": patched(TILE_DT, hd.tiles_off, 1, first=0),
        "reference range": patched(TILE_DT, hd.tiles_off, hd.n_tiles - 1, count=2000),
        "out of order": patched(TILE_DT, hd.tiles_off, 1, tx=0, ty=0),
        "outside the image": patched(TILE_DT, hd.tiles_off, 0, tx=2),
    }
    for msg, table in cases.items():
        assert run(table) < 0, msg
        assert msg.encode() in L.sp_last_error(), (msg, L.sp_last_error())
    assert run(good, h=71) < 0 and b"packed for" in L.sp_last_error()
    assert run(good[:64]) < 0
    swapped = bytearray(good)
    r = np.frombuffer(swapped, "<i4", hd.n_refs, hd.refs_off)
    tiles = np.frombuffer(good, TILE_DT, hd.n_tiles, hd.tiles_off)
    two = next(t for t in tiles if t["count"] == 2)
    r[two["first"]], r[two["first"] + 1] = 1, 0
    assert run(swapped) < 0 and b"out of order" in L.sp_last_error()
    need = ctypes.c_int64()
    bad = _lib.SpDrawOp(kind=0, x0=0, y0=0, x1=90, y1=3)
    assert L.sp_draw_pack(ctypes.byref(bad), 1, None, 0, 70, 90, None, 0, ctypes.byref(need)) < 0
