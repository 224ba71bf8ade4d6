"""Shared by tests/test_draw_device.py (CPU) and tests/test_gpu_draw.py (GPU): the image sizes and label mixes both
draw, and the numpy executor of the packed draw table (what sp_draw_rgb's kernel reads), which is the CPU test's
stand-in for the device and the GPU test's reference for the entry point on its own."""
import os
import sys

import numpy as np
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
from test_draw import AMENITY_TEXTS  # noqa: E402,F401  (the amenity strings of serve.py:31-59)

SIZES = [(1, 1), (2, 3), (7, 5), (33, 17), (64, 8), (65, 9), (90, 70)]  # (width, height)

OP_DT = np.dtype([("kind", "<i4"), ("x0", "<i4"), ("y0", "<i4"), ("x1", "<i4"), ("y1", "<i4"), ("ink", "<u4"),
                  ("mask_off", "<i8"), ("mask_stride", "<i4"), ("sx", "<i4"), ("sy", "<i4"), ("reserved", "<i4")])
TILE_DT = np.dtype([("tx", "<i4"), ("ty", "<i4"), ("first", "<i4"), ("count", "<i4")])


def _div255(a):
    t = a + 128
    return ((t >> 8) + t) >> 8


def execute(table: bytes, img: np.ndarray):
    """The packed draw table applied to img (uint8 [H, W, 3]) in place, as the kernel walks it: one tile at a time,
    the tile's operations in list order, each clipped to the tile. Also checks the table's own invariants."""
    from spotter_amd._lib import SP_DRAW_TILE_H, SP_DRAW_TILE_W, SpDrawTable

    hd = SpDrawTable.from_buffer_copy(table)
    H, W, _ = img.shape
    assert (hd.height, hd.width) == (H, W) and hd.total_bytes == len(table)
    ops = np.frombuffer(table, OP_DT, hd.n_ops, hd.ops_off)
    tiles = np.frombuffer(table, TILE_DT, hd.n_tiles, hd.tiles_off)
    refs = np.frombuffer(table, "<i4", hd.n_refs, hd.refs_off)
    masks = np.frombuffer(table, np.uint8, hd.mask_bytes, hd.masks_off)
    keys = [(int(t["ty"]), int(t["tx"])) for t in tiles]
    assert keys == sorted(set(keys)), "tiles ascend by (ty, tx), none twice"
    nxt, seen = 0, set()
    for t in tiles:
        assert t["first"] == nxt and t["count"] > 0
        nxt += int(t["count"])
        X0, Y0 = int(t["tx"]) * SP_DRAW_TILE_W, int(t["ty"]) * SP_DRAW_TILE_H
        X1, Y1 = min(X0 + SP_DRAW_TILE_W, W) - 1, min(Y0 + SP_DRAW_TILE_H, H) - 1
        mine = refs[t["first"]:t["first"] + t["count"]]
        assert np.all(np.diff(mine) > 0), "a tile's operations keep list order"
        for r in mine:
            op = ops[r]
            xa, xb = max(X0, int(op["x0"])), min(X1, int(op["x1"]))
            ya, yb = max(Y0, int(op["y0"])), min(Y1, int(op["y1"]))
            assert xa <= xb and ya <= yb, "an operation is listed only in tiles it touches"
            seen.add(int(r))
            ink = np.array([(int(op["ink"]) >> s) & 255 for s in (0, 8, 16)], np.int64)
            if op["kind"] == 0:
                img[ya:yb + 1, xa:xb + 1] = ink
                continue
            assert op["kind"] == 1
            rows = int(op["sy"]) + np.arange(ya, yb + 1) - int(op["y0"])
            cols = int(op["sx"]) + np.arange(xa, xb + 1) - int(op["x0"])
            m = masks[int(op["mask_off"]) + rows[:, None] * int(op["mask_stride"]) + cols[None, :]].astype(np.int64)
            out = img[ya:yb + 1, xa:xb + 1].astype(np.int64)
            img[ya:yb + 1, xa:xb + 1] = _div255(out * (255 - m[..., None]) + ink[None, None, :] * m[..., None])
    assert nxt == hd.n_refs and seen == set(range(hd.n_ops))


def random_box(rng, w, h, narrow=False):
    x0, y0 = rng.uniform(-0.6 * w - 3, 1.2 * w), rng.uniform(-0.6 * h - 3, 1.2 * h)
    bw = rng.uniform(0, 6) if narrow and rng.random() < 0.7 else rng.uniform(0, 1.2 * w + 4)
    bh = rng.uniform(0, 6) if narrow and rng.random() < 0.7 else rng.uniform(0, 1.2 * h + 4)
    return [x0, y0, x0 + bw, y0 + bh]


def label(draws, box, text):
    """serve.py:128-136."""
    for d in draws:
        d.rectangle(box, outline="red", width=3)
        d.text(xy=(box[0] + 5, box[1] + 5), text=text, fill="white", stroke_width=1, stroke_fill="black")


def coloured(draws, h):
    """Inks whose channels are neither 0 nor 255, over every mask value and random backgrounds: where the single
    rounding of Pillow's BLEND8 differs from rounding the two products apart."""
    ramp = Image.fromarray(np.arange(256, dtype=np.uint8).reshape(16, 16), "L")
    for d in draws:
        d.text((3.3, 2.6), "dining area", fill=(200, 30, 120), stroke_width=1, stroke_fill=(10, 90, 250))
        for i, ink in enumerate([(1, 127, 254), (200, 100, 50), (128, 129, 77)]):
            d.bitmap((5 + 20 * i, 20 + 9 * i), ramp, fill=ink)
        d.bitmap((-7, h - 9), ramp, fill=(33, 66, 99))
