"""CPU: the host half of the batched label draw. record_labels against the same calls through the
drop-in's ImageDraw, list for list; its fallbacks; sp_draw_batch_plan; the batch buffer's layout with the numpy
stand-in of tests/draw_helpers.py for the kernel; and the bulk pipeline's control flow with stage C inline and on its
worker thread, over the host stand-ins of tests/test_jpeg_enc_batch_host.py."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")
from PIL import Image, ImageDraw, ImageFont  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from draw_helpers import AMENITY_TEXTS, SIZES, execute, label as _label, random_box as _box  # noqa: E402
from test_jpeg_batch_host import _png, _raw  # noqa: E402
from test_jpeg_enc_batch_host import ID2LABEL, _detector  # noqa: E402

from spotter_amd import draw as D  # noqa: E402
from spotter_amd._lib import SP_DRAW_BATCH_MAX, SpDrawBatchItem, SpDrawTable, lib  # noqa: E402

# start fractions: exactly 0, both class boundaries (31.5/64 for x, 32.5/64 for y) and 1e-5 either side of them (inside
# that band the memo is not used), just above 0, just under 1, and a dense grid in between
_EDGES = [0.0, 1e-7, 2e-5, 31.5 / 64 - 2e-5, 31.5 / 64 - 1e-5, 31.5 / 64, 31.5 / 64 + 1e-5, 31.5 / 64 + 2e-5,
          32.5 / 64 - 2e-5, 32.5 / 64 - 1e-5, 32.5 / 64, 32.5 / 64 + 1e-5, 32.5 / 64 + 2e-5, 1 - 1e-5, 1 - 1e-9]
FRACTIONS = _EDGES + [i / 16 + 0.013 for i in range(16)]


def _device_image(w, h):
    """A DeviceRGBImage without host pixels over a host tensor: nothing here flushes it."""
    from spotter_amd.jpeg import DeviceRGBImage

    return DeviceRGBImage(torch.zeros((h, w, 3), dtype=torch.uint8))


def _labels(rng, w, h, n, k0):
    """n boxes of draw_helpers.random_box (outside and partly negative ones among them) whose text starts
    (box + 5) are moved onto the fraction grid, and the amenity strings in turn from k0 on."""
    boxes, texts = [], []
    for k in range(n):
        b = _box(rng, w, h)
        fx, fy = FRACTIONS[(k0 + k) % len(FRACTIONS)], FRACTIONS[(k0 + 3 * k + 1) % len(FRACTIONS)]
        dx, dy = np.floor(b[0]) + fx - b[0], np.floor(b[1]) + fy - b[1]
        boxes.append([float(b[0] + dx), float(b[1] + dy), float(b[2] + dx), float(b[3] + dy)])
        texts.append(AMENITY_TEXTS[(k0 + k) % len(AMENITY_TEXTS)])
    return boxes, texts


def _both(w, h, boxes, texts):
    """(the list record_labels leaves, the list the same calls through draw_module().Draw leave), packed."""
    a, b = _device_image(w, h), _device_image(w, h)
    D.record_labels(a, boxes, texts)
    d = D.draw_module().Draw(b)
    assert type(d) is D.DeviceDraw
    for box, text in zip(boxes, texts):
        _label((d,), box, text)
    assert a._im is None and b._im is None
    assert (len(a._draw_list) == 0) == (len(b._draw_list) == 0)
    if not len(b._draw_list):
        return b"", b""
    return a._draw_list.packed(), b._draw_list.packed()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_record_labels_leaves_the_list_the_draw_calls_leave(size):
    """Every amenity string over the fraction grid, cold (keys being learned: every text goes through Pillow) and warm
    (stamps replayed): the packed tables, i.e. operations, tile bins and mask bytes at their offsets, are equal."""
    w, h = size
    rng = np.random.default_rng(w * 131 + h)
    k0 = 0
    for warm in (False, True, True):
        before = dict(D.stamp_stats)
        for rep in range(12):
            boxes, texts = _labels(rng, w, h, 6 + rep % 3, k0)
            k0 += len(boxes)
            got, want = _both(w, h, boxes, texts)
            assert got == want, f"{size} warm={warm} rep {rep}"
        if warm:
            assert D.stamp_stats["hits"] > before["hits"]
    assert D.stamp_stats["hits"] > 0 and D.stamp_stats["captures"] > 0 and D.stamp_stats["fallbacks"] > 0


def test_all_positive_grid_hits_every_class_pair():
    """Boxes inside a 640 x 640 image with starts on the full fraction grid, x against y: after two passes that teach
    the keys, a third is served from stamps for every start that has a class, and stays equal."""
    boxes = [[10.0 + 7 * i + fx - 5, 20.0 + 5 * j + fy - 5, 300.0 + i, 400.0 + j]
             for i, fx in enumerate(FRACTIONS) for j, fy in enumerate(FRACTIONS)]
    for text in ("TV", "dining area"):
        texts = [text] * len(boxes)
        shifted = [[b[0] + 0.001, b[1] + 0.001, b[2], b[3]] for b in boxes]
        for bs in (boxes, shifted, boxes):
            before = dict(D.stamp_stats)
            got, want = _both(640, 640, bs, texts)
            assert got == want
        # the last pass: only the starts without a class (boundaries, below 1e-5) and the (0, 0) start, whose key is
        # never seen at a second fraction, went through Pillow
        assert D.stamp_stats["hits"] - before["hits"] > len(boxes) // 2
        assert D.stamp_stats["captures"] - before["captures"] <= 1


def test_fallbacks_record_what_pillow_records():
    before = dict(D.stamp_stats)
    for _ in range(3):  # often enough to have taught the key, were it taught
        got, want = _both(90, 70, [[-5.75, 3.25, 40.0, 30.0]], ["sofa"])  # box[0] + 5 < 0
        assert got == want and got
    assert D.stamp_stats["hits"] == before["hits"] and D.stamp_stats["fallbacks"] == before["fallbacks"] + 3
    # a NaN in the box: Pillow's own casts decide, so the image is handed over to Pillow (load(), which on this
    # stand-in image only says so) at the same call, with the same operations recorded before it, on both paths
    from spotter_amd.jpeg import DeviceRGBImage

    class HandedOver(Exception):
        pass

    class NoLoad(DeviceRGBImage):
        def load(self):
            raise HandedOver(len(self._draw_list))

    nan = float("nan")
    good = [3.25, 4.5, 60.0, 50.0]
    # (in x only: with a NaN in y Pillow's own rectangle loops over 2^31 rows of its clip, for seconds)
    for box in ([nan, 3.0, 40.0, 30.0], [2.0, 3.0, nan, 30.0]):
        outcomes = []
        for record in (True, False):
            im = NoLoad(torch.zeros((70, 90, 3), dtype=torch.uint8))
            with pytest.raises(HandedOver) as e:
                if record:
                    D.record_labels(im, [good, box], ["sofa", "sofa"])
                else:
                    d = D.draw_module().Draw(im)
                    _label((d,), good, "sofa")
                    _label((d,), box, "sofa")
            outcomes.append((e.value.args, im._draw_list.packed()))
        assert outcomes[0] == outcomes[1] and outcomes[0][0][0] > 0


def test_another_default_font_is_left_to_pillow(monkeypatch):
    other = ImageFont.load_default(size=13)
    monkeypatch.setattr(ImageDraw.ImageDraw, "font", other)
    before = dict(D.stamp_stats)
    boxes, texts = [[3.25, 4.5, 60.0, 50.0]] * 4, ["oven"] * 4
    got, want = _both(90, 70, boxes, texts)
    assert got == want and got
    assert D.stamp_stats["hits"] == before["hits"] and D.stamp_stats["captures"] == before["captures"]
    assert D.stamp_stats["fallbacks"] == before["fallbacks"] + 4


def test_a_key_whose_captures_differ_is_never_stamped(monkeypatch):
    """The second capture of a key is made to differ from the first (one pixel further right): the key is dropped for
    good, every later label of it is recorded by Pillow, and the lists stay Pillow's."""
    real, n = D._capture_text, [0]

    def skewed(*a):
        got = real(*a)
        n[0] += 1
        if got is not None and n[0] % 2 == 0:
            got = tuple(e[:4] + (e[4] + 1,) + e[5:] for e in got)
        return got

    monkeypatch.setattr(D, "_capture_text", skewed)
    text = "a string no other test draws"
    before = dict(D.stamp_stats)
    for i in range(6):
        got, want = _both(90, 70, [[3.1 + 0.05 * i, 4.2, 60.0, 50.0]], [text])
        assert got == want and got
    assert (text, 1, 1) in D._stamp_never and (text, 1, 1) not in D._stamps
    assert D.stamp_stats["hits"] == before["hits"]
    assert D.stamp_stats["captures"] == before["captures"] + 2 and D.stamp_stats["fallbacks"] == before["fallbacks"] + 4


def test_record_labels_on_a_host_image_draws_with_pillow():
    rng = np.random.default_rng(3)
    arr = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    a, b = Image.fromarray(arr), Image.fromarray(arr)
    boxes, texts = _labels(rng, 90, 70, 6, 0)
    D.record_labels(a, boxes, texts)
    d = ImageDraw.Draw(b)
    for box, text in zip(boxes, texts):
        _label((d,), box, text)
    assert np.array_equal(np.asarray(a), np.asarray(b)) and not np.array_equal(np.asarray(a), arr)


# --------------------------------------------------------------------------------------------- the batch buffer
def _batch_buffer(lists):
    """The batch buffer as DESIGN.md §5.28 lays it out, built here independently of spotter_amd.jpeg: the packed
    tables back to back, then the rows. (buffer, rows, end of the tables)."""
    tables = [lst.packed() for lst in lists]
    items = (SpDrawBatchItem * len(lists))()
    off = 0
    for it, t, lst in zip(items, tables, lists):
        it.table_off, it.table_bytes, it.height, it.width = off, len(t), lst.height, lst.width
        off += len(t)
    return bytearray(b"".join(tables)), items, off


def _list_with_tiles(w, h, tiles):
    """A DrawList over w x h whose operations touch exactly `tiles` 64 x 8 tiles."""
    lst = D.DrawList(w, h)
    for t in range(tiles):
        lst.fill(64 * t + 3, 1, 64 * t + 9, 5, 0x0000FF)
    return lst


def test_batch_plan_prefix_sums_and_refusals():
    L = lib()
    lists = [_list_with_tiles(300, 20, 1), _list_with_tiles(300, 20, 3), _list_with_tiles(64, 8, 1)]
    buf, items, end = _batch_buffer(lists)
    host = (C.c_char * len(buf)).from_buffer(buf)
    for it in items:
        it.rgb, it.row_stride = 4096, 1234
    assert L.sp_draw_batch_plan(items, 3, host, end) == 5, L.sp_last_error()
    assert [(it.n_tiles, it.first_wg) for it in items] == [(1, 0), (3, 1), (1, 4)]
    assert all((it.rgb, it.row_stride) == (4096, 1234) for it in items)  # the caller's fields are left alone
    assert L.sp_draw_batch_plan(items, 1, host, end) == 1
    # a table without a touched tile (every operation clipped away) is refused: such an image is left out
    empty = D.DrawList(300, 20)
    empty.fill(400, 1, 500, 5, 0x00FF00)
    assert len(empty) == 0 and SpDrawTable.from_buffer_copy(empty.packed()).n_tiles == 0
    buf0, items0, end0 = _batch_buffer([lists[1], empty])
    host0 = (C.c_char * len(buf0)).from_buffer(buf0)
    assert L.sp_draw_batch_plan(items0, 2, host0, end0) == -1 and b"image 1" in L.sp_last_error()
    assert (items0[0].n_tiles, items0[0].first_wg) == (0, 0)  # a refused call writes nothing
    assert L.sp_draw_batch_plan(items, 0, host, end) == -1 and b"n = 0" in L.sp_last_error()
    many = (SpDrawBatchItem * (SP_DRAW_BATCH_MAX + 1))()
    assert L.sp_draw_batch_plan(many, SP_DRAW_BATCH_MAX + 1, host, end) == -1 and b"n = 65" in L.sp_last_error()
    assert L.sp_draw_batch_plan(None, 1, host, end) == -1 and b"null" in L.sp_last_error()
    assert L.sp_draw_batch_plan(items, 1, None, end) == -1 and b"null" in L.sp_last_error()
    for bad in (8, -16, end, end - 16):  # misaligned, negative, no room for a header
        items[1].table_off = bad
        assert L.sp_draw_batch_plan(items, 3, host, end) == -1 and b"image 1" in L.sp_last_error(), bad


def test_numpy_stand_in_over_a_batch_buffer_draws_pillows_pixels():
    """The layout flush_many uploads, for the seven SIZES: tables at multiples of 16, back to back, the rows behind
    them; draw_helpers.execute on each table of the buffer gives Pillow's pixels."""
    from spotter_amd.jpeg import DeviceRGBImage, _DrawStage

    rng = np.random.default_rng(28)
    refs, ims, arrs = [], [], []
    for i, (w, h) in enumerate(SIZES):
        arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref, im = Image.fromarray(arr), DeviceRGBImage(torch.from_numpy(arr.copy()))
        dr = ImageDraw.Draw(ref)
        boxes, texts = _labels(rng, w, h, 5, i)
        boxes.append([0.0, 0.0, float(w), float(h)])  # (every image keeps at least one touched tile)
        texts.append("TV")
        D.record_labels(im, boxes, texts)
        for box, text in zip(boxes, texts):
            _label((dr,), box, text)
        refs.append(ref), ims.append(im), arrs.append(arr)

    # the staging code itself (what run_many uploads), with pageable host memory where it pins and allocates
    class HostStage(_DrawStage):
        def __init__(self):
            self._stage = self._table = self._copied = self._done = None

        def _alloc(self, n):
            return torch.zeros(n, dtype=torch.uint8), None  # (zeroed: sp_draw_pack leaves its padding unwritten)

    stage = HostStage()
    pairs = [(im._draw_list, im._dev) for im in ims]
    items, buf, end = stage.pack_batch(pairs)
    n = len(pairs)
    rows = C.sizeof(SpDrawBatchItem) * n
    assert len(buf) == end + rows and end % 16 == 0
    off = wg = 0
    for it, (lst, t), ref, arr in zip(items, pairs, refs, arrs):
        table = lst.packed()
        assert it.table_off == off and it.table_off % 16 == 0 and it.table_bytes == len(table)  # back to back
        assert bytes(buf[off:off + len(table)]) == table
        hd = SpDrawTable.from_buffer_copy(table)
        assert (it.n_tiles, it.first_wg) == (hd.n_tiles, wg) and hd.n_tiles > 0
        assert (it.rgb, it.height, it.width, it.row_stride) == (t.data_ptr(), t.shape[0], t.shape[1], t.stride(0))
        off, wg = off + len(table), wg + hd.n_tiles
        out = arr.copy()
        execute(bytes(buf[it.table_off:it.table_off + it.table_bytes]), out)
        assert np.array_equal(out, np.asarray(ref)) and not np.array_equal(out, arr)
    assert off == end and bytes(buf[end:]) == bytes(items)  # the rows after the tables


# ------------------------------------------------------------------------ bulk control flow, stage C on its thread
COMBOS = [("pillow", False), ("pillow", True), ("batched", False), ("batched", True)]
ITEMS = [_raw(9, h=40, w=60), _png(50, h=30, w=50), b"neither", _raw(4, h=32, w=48), _raw(11, h=24, w=64),
         _raw(30, h=20, w=30), _raw(7, h=21, w=33)]


def _bulk_threads():
    return [t for t in threading.enumerate() if t.name.startswith("spotter-bulk")]


def test_bulk_results_are_equal_between_the_four_option_combinations():
    outs = {}
    for draw, overlap in COMBOS:
        det, enc = _detector(batch=3, labelled=True, id2label=ID2LABEL, label_draw=draw, label_overlap=overlap)
        out = list(det.detect(iter(ITEMS)))
        assert enc.calls == [2, 3, 1]  # one encode_many per chunk, in chunk order
        assert len(det.stage_seconds["a"]) == len(det.stage_seconds["b"]) == len(det.stage_seconds["c"]) == 3
        assert [("error" in r) for r in out] == [False, False, True, False, False, False, False]
        assert [r["size"] for r in out if "size" in r] == [(60, 40), (50, 30), (48, 32), (64, 24), (30, 20), (33, 21)]
        outs[draw, overlap] = [r.get("jpeg") for r in out]
        assert not _bulk_threads()
    assert all(v == outs["pillow", False] for v in outs.values()) and outs["pillow", False][0].startswith(b"JPG 60x40 ")
    from spotter_amd.bulk import BulkDetector

    with pytest.raises(ValueError, match="label_draw"):
        BulkDetector(None, None, label_draw="gpu")


@pytest.mark.parametrize("overlap", [False, True])
def test_an_exception_in_stage_c_arrives_at_its_chunks_yield(overlap):
    det, enc = _detector(batch=2, labelled=True, id2label=ID2LABEL, label_overlap=overlap)
    real = enc.encode_many

    def failing(srcs, **kw):
        if len(enc.calls) == 1:  # the second chunk's call
            enc.calls.append(len(srcs))
            raise RuntimeError("stage C of chunk 1")
        return real(srcs, **kw)

    enc.encode_many = failing
    items = [_raw(10 + i, h=20, w=30) for i in range(8)]
    got = []
    with pytest.raises(RuntimeError, match="stage C of chunk 1"):
        for r in det.detect(items):
            got.append(r)
    assert len(got) == 2 and all("jpeg" in r for r in got)  # chunk 0 whole, nothing of chunk 1 or later
    assert not _bulk_threads()


@pytest.mark.parametrize("overlap", [False, True])
def test_closing_the_generator_early_joins_the_threads(overlap):
    det, enc = _detector(batch=2, labelled=True, id2label=ID2LABEL, label_overlap=overlap)
    gen = det.detect([_raw(10 + i, h=20, w=30) for i in range(10)])
    first = next(gen)
    assert "jpeg" in first and round(float(first["scores"][0]) * 255) == 10
    gen.close()
    assert not _bulk_threads()
    assert len(enc.calls) <= 3  # nothing went on after the close
