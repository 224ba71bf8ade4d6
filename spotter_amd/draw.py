"""The label drawing of serve.py:119-137 (`ImageDraw.Draw(image)`, `draw.rectangle`, `draw.text`): Pillow's own
Python code, with two changes. The default font's glyph masks are memoised (below), and on a GPU-decoded image
that has no host pixels the C core object behind `ImageDraw.draw` is a recorder whose fills and blends run on the
GPU (second half of this file: DeviceDraw, DrawList).

Measured on the MI355X box's EPYC host (tools/detect_path.py, profiles/r5/jpeg/): drawing the 16 labels of a
/detect response takes 6.3 ms, nearly all of it FreeType rendering the same few strings (the amenity names of
serve.py:31-59) again and again: `ImageDraw.text` with `stroke_width=1` renders each label twice through
`FreeTypeFont.getmask2` (stroke, then fill), ~0.2 ms each, and the result depends on the string, the stroke,
the ink and — through the hinted 26.6 fixed-point origin — only on which of three classes each fractional
start coordinate falls in: exactly 0, (0, u), [u, 1) with u = 31.5/64 for x and 32.5/64 for y. `Draw(im)`
here is Pillow's ImageDraw with its default font replaced by the same font whose getmask2 keeps the masks per
(string, options, start class).

Exactness: a key is served from the memo only after two renders at *different* start fractions of its class
gave identical masks (a key whose masks differ is never memoised again); fractions within 1e-5 of a class
boundary, negative fractions and every non-default option are rendered by Pillow as before. A render at
exactly the same start (string, options and both start coordinates equal) is also served again from a bounded
cache (`EXACT_CAP` entries, least recently used out): the same inputs, so the same mask. The masks are pure
functions of those inputs, and draw_bitmap then composites them exactly as Pillow does, so the drawn pixels
are Pillow's (tests/test_draw.py: all amenity strings over dense start grids; the whole serve.py tail
byte-identical on the GPU box).
"""
from __future__ import annotations

import ctypes as C
import struct
import threading
import types
from collections import OrderedDict

from PIL import Image as _PILImage
from PIL import ImageColor as _PILColor
from PIL import ImageDraw as _PILDraw
from PIL import ImageFont as _PILFont
from PIL import ImagePath as _PILPath

# the hinted origin moves to the next pixel from these fractions on (26.6 fixed point; y points down in the
# image and up in FreeType, hence the different half-way point)
_UPPER_X = 31.5 / 64
_UPPER_Y = 32.5 / 64
_EPS = 1e-5


def start_class(f: float, upper: float):
    """The start-offset class of a fractional coordinate, or None where the memo is not used."""
    if f == 0.0:
        return 0
    if f < _EPS or f >= 1.0 or abs(f - upper) < _EPS:
        return None
    return 1 if f < upper else 2


class _MemoFont(_PILFont.FreeTypeFont):
    """Pillow's default FreeType font (ImageFont.load_default()) with memoised getmask2."""

    EXACT_CAP = 4096  # renders kept for an exact repeat of (string, options, start)

    def _memo_init(self):
        self._memo_lock = threading.Lock()
        self._memo: dict = {}        # key -> (mask, offset) once verified
        self._pending: dict = {}     # key -> (start pair, mask signature) of its first render
        self._no_memo: set = set()
        self._exact: OrderedDict = OrderedDict()  # (string, options, exact start) -> (mask, offset)
        self.memo_stats = {"hits": 0, "exact_hits": 0, "renders": 0, "bypass": 0}
        # id(mask) -> its bytes (None until DeviceDraw first asks) for exactly the masks _exact and _memo hold:
        # entries leave with their mask, so an id in here always names a live mask of this font
        self._held: dict = {}
        self._memo_ids: set = set()

    def _release(self, val):
        if val is not None and id(val[0]) not in self._memo_ids:
            self._held.pop(id(val[0]), None)

    def _exact_put(self, ekey, val):
        with self._memo_lock:
            old = self._exact.get(ekey)
            self._exact[ekey] = val
            if old is not None and old[0] is not val[0]:
                self._release(old)
            self._held.setdefault(id(val[0]), None)
            if len(self._exact) > self.EXACT_CAP:
                self._release(self._exact.popitem(last=False)[1])

    def mask_bytes(self, mask):
        """The bytes of a mask this font holds in its caches (shared objects nothing writes to), kept with it for
        the device draw's blends; None for any other object."""
        b = self._held.get(id(mask), self)
        if b is self:
            return None
        if b is None:
            b = _tobytes(mask)
            with self._memo_lock:
                if id(mask) in self._held:
                    self._held[id(mask)] = b
        return b

    def getmask2(self, text, mode="", *args, start=None, **kwargs):
        out = self._getmask2(text, mode, *args, start=start, **kwargs)
        log = getattr(_capturing, "calls", None)
        if log is not None:  # record_labels is learning a stamp on this thread
            log.append((text, mode, args, start, kwargs, out))
        return out

    def lookup(self, text, mode, sx, sy, cx, cy, opts):
        """What getmask2(text, mode, start=(sx, sy), **kwargs) returns when it needs no render, else None: the same
        two lookups in the same order with the same bookkeeping, for a caller that already holds the key's parts
        (opts = _opts(kwargs), (cx, cy) the start classes, neither None; mode "", "L" or "1")."""
        ekey = (text, mode, sx, sy, opts)
        with self._memo_lock:
            hit = self._exact.get(ekey)
            if hit is not None:
                self._exact.move_to_end(ekey)
        if hit is not None:
            self.memo_stats["exact_hits"] += 1
            return hit
        key = (text, mode, cx, cy, opts)
        if key in self._no_memo:
            return None
        hit = self._memo.get(key)
        if hit is not None:
            self.memo_stats["hits"] += 1
        return hit

    def _getmask2(self, text, mode="", *args, start=None, **kwargs):
        if mode not in ("", "L", "1"):
            # "RGBA" (ImageDraw.text(embedded_color=True)): Pillow fills the returned mask's alpha band in place
            # (color.fillband), so a shared cached mask would be overwritten; these renders are never cached
            self.memo_stats["bypass"] += 1
            return super().getmask2(text, mode, *args, start=start, **kwargs)
        key = ekey = None
        if not args and isinstance(text, str) and start is not None:
            try:
                opts = _opts(kwargs)
                sx, sy = float(start[0]), float(start[1])
                ekey = (text, mode, sx, sy, opts)
                hash(ekey)
            except (TypeError, ValueError, IndexError):
                ekey = None
            if ekey is not None:
                cx, cy = start_class(sx, _UPPER_X), start_class(sy, _UPPER_Y)
                if cx is not None and cy is not None:
                    key = (text, mode, cx, cy, opts)
        if ekey is not None:
            with self._memo_lock:
                hit = self._exact.get(ekey)
                if hit is not None:
                    self._exact.move_to_end(ekey)
            if hit is not None:
                self.memo_stats["exact_hits"] += 1
                return hit
        if key is None or key in self._no_memo:
            self.memo_stats["bypass"] += 1
            out = super().getmask2(text, mode, *args, start=start, **kwargs)
            if ekey is not None:
                self._exact_put(ekey, out)
            return out
        hit = self._memo.get(key)
        if hit is not None:
            self.memo_stats["hits"] += 1
            return hit
        mask, offset = super().getmask2(text, mode, start=start, **kwargs)
        self._exact_put(ekey, (mask, offset))
        self.memo_stats["renders"] += 1
        sig = (bytes(mask), mask.size, tuple(offset))
        with self._memo_lock:
            first = self._pending.get(key)
            if first is None:
                self._pending[key] = (tuple(start), sig)
            elif first[0] != tuple(start):  # a second fraction of the class: verify before memoising
                if first[1] == sig:
                    self._memo[key] = (mask, offset)
                    self._memo_ids.add(id(mask))
                    self._held.setdefault(id(mask), None)
                else:
                    self._no_memo.add(key)
                del self._pending[key]
        return mask, offset


def _opts(kwargs) -> tuple:
    return tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kwargs.items()))


_capturing = threading.local()  # .calls: the getmask2 calls of this thread's running stamp capture, else absent


def _tobytes(mask) -> bytes:
    im = _PILImage.Image()
    im._im, im._mode, im._size = mask, mask.mode, mask.size
    return im.tobytes()


_font = None
_font_lock = threading.Lock()


def memo_default_font() -> _MemoFont:
    global _font
    with _font_lock:
        if _font is None:
            f = _PILFont.load_default()
            if not isinstance(f, _PILFont.FreeTypeFont):  # Pillow without FreeType: its bitmap font, as is
                return f
            f.__class__ = _MemoFont
            f._memo_init()
            _font = f
        return _font


# ---------------------------------------------------------------------------------------------------------------
# Drawing on a device image. Pillow's ImageDraw does its colour parsing, text layout, anchors
# and stroke-then-fill order in Python and reaches the pixels, for everything serve.py draws, through two methods
# of its C core object `self.draw`: draw_rectangle and draw_bitmap (plus draw_ink). DeviceDraw is that same
# Python class with `self.draw` replaced by a recorder, which turns the two calls into the fill / blend operations
# of sp_draw_rgb (include/spotter_hip.h) on the image's draw list; the image applies the list on the GPU before
# anything reads its pixels (spotter_amd/jpeg.py DeviceRGBImage.flush). Anything else hands over to Pillow.

_OP = struct.Struct("<5iIq4i")  # sp_draw_op (tests/test_draw_device.py checks the layout against the header)
_pack = _OP.pack
_FILL, _BLEND = 0, 1
_COORD_MAX = 1 << 30  # coordinates beyond this (or NaN / inf) are left to Pillow's own int casts


class DrawList:
    """The recorded operations of one image, in call order: packed sp_draw_op records and the bytes of the "L"
    masks they blend. Rectangles are clipped to the image here; an operation that misses it is dropped."""

    def __init__(self, width: int, height: int):
        self.width, self.height = int(width), int(height)
        self.clear()

    def clear(self):
        self.ops: list = []
        self.masks: list = []
        self.mask_bytes = 0
        self._mask_at: dict = {}  # id(mask bytes) -> offset: a mask drawn twice is stored once

    def __len__(self):
        return len(self.ops)

    def fill(self, x0, y0, x1, y1, ink):
        """Every pixel of [x0, x1] x [y0, y1] (inclusive), clipped to the image, becomes the ink."""
        if x0 < 0:
            x0 = 0
        if y0 < 0:
            y0 = 0
        if x1 >= self.width:
            x1 = self.width - 1
        if y1 >= self.height:
            y1 = self.height - 1
        if x0 <= x1 and y0 <= y1:
            self.ops.append(_pack(_FILL, x0, y0, x1, y1, ink & 0xFFFFFF, 0, 0, 0, 0, 0))

    def blend(self, x, y, mask: bytes, mw, mh, ink):
        """An "L" mask of mw x mh bytes placed at (x, y), clipped to the image (Paste.c ImagingFill2)."""
        x0, y0, x1, y1 = (x if x > 0 else 0), (y if y > 0 else 0), x + mw - 1, y + mh - 1
        if x1 >= self.width:
            x1 = self.width - 1
        if y1 >= self.height:
            y1 = self.height - 1
        if x0 > x1 or y0 > y1:
            return
        off = self._mask_at.get(id(mask))
        if off is None:
            off = self._mask_at[id(mask)] = self.mask_bytes
            self.masks.append(mask)  # kept alive here, so its id stays its own until clear()
            self.mask_bytes += len(mask)
        self.ops.append(_pack(_BLEND, x0, y0, x1, y1, ink & 0xFFFFFF, off, mw, x0 - x, y0 - y, 0))

    def pack(self, out=None, cap=0) -> int:
        """sp_draw_pack: bin the operations into tiles and write the packed table (header, operations, tile bins,
        mask bytes) to the host address `out` when it fits in `cap` bytes. Returns the bytes the table needs."""
        from ._lib import lib

        need = C.c_int64()
        L = lib()
        if L.sp_draw_pack(b"".join(self.ops), len(self.ops), b"".join(self.masks), self.mask_bytes, self.height,
                          self.width, out, cap, C.byref(need)):
            raise RuntimeError(f"sp_draw_pack: {L.sp_last_error().decode(errors='replace')}")
        return need.value

    def packed(self) -> bytes:
        """The packed table as bytes (tests; the image packs straight into its pinned staging buffer)."""
        n = self.pack()
        buf = C.create_string_buffer(n)
        self.pack(C.addressof(buf), n)
        return buf.raw


# Pillow's core draw object on a 1x1 RGB image: draw_ink and the argument checks of draw_rectangle are its own
# (same values, same exceptions and messages); whatever it draws lands in the scratch pixel.
_SCRATCH = _PILImage.core.draw(_PILImage.core.fill("RGB", (1, 1)), 0)


def _bytes_of(mask) -> bytes:
    """The bytes of an "L" core image: kept with the mask when it is one the memoising default font holds (the
    same object comes back for a repeated label), read afresh for any other font's render or a caller's bitmap."""
    f = _font
    b = f.mask_bytes(mask) if f is not None else None
    return _tobytes(mask) if b is None else b


def _ints(xy, n):
    """The n doubles Pillow's PyPath_Flatten reads from xy, cast to int as its C code does (toward zero); None
    where the cast is not defined in Python (NaN, inf) or the value is beyond any image."""
    plain = type(xy) in (list, tuple) and len(xy) == n
    if plain:
        for v in xy:
            if type(v) is not float and type(v) is not int:
                plain = False
                break
    if not plain:
        xy = _PILPath.Path(xy).tolist(True)
        if len(xy) != n:
            return None
    try:
        out = [int(v) for v in xy]
    except (ValueError, OverflowError):
        return None
    if min(out) <= -_COORD_MAX or max(out) >= _COORD_MAX:
        return None
    return out


def _outline(lst, x0, y0, x1, y1, ink, w):
    """ImagingDrawRectangle, outline of width w > 0, as four fills: for i < w the rows y0 + i and y1 - i over x0..x1,
    then the columns x1 - i and x0 + i from row y0 + w towards row y1 - w + 1, half-open in the direction of travel
    (Draw.c line32 draws |dy| points from the start). One ink, so the order among the four pieces does not matter."""
    lst.fill(x0, y0, x1, y0 + w - 1, ink)
    lst.fill(x0, y1 - w + 1, x1, y1, ink)
    ys, ye = y0 + w, y1 - w + 1
    if ye != ys:
        ra, rb = (ys, ye - 1) if ye > ys else (ye + 1, ys)
        lst.fill(x1 - w + 1, ra, x1, rb, ink)
        lst.fill(x0, ra, x0 + w - 1, rb, ink)


class _Recorder:
    """Stands where ImageDraw keeps its C core draw object. draw_rectangle and draw_bitmap append to the image's
    draw list by Pillow's rules (Draw.c ImagingDrawRectangle, Paste.c ImagingFill2); every other method hands the
    image over to Pillow."""

    def __init__(self, owner):
        self._owner = owner
        self._image = owner._image
        self.draw_ink = _SCRATCH.draw_ink

    def draw_rectangle(self, xy, ink, fill, width=0):
        _SCRATCH.draw_rectangle(xy, ink, fill, width)  # Pillow's own argument errors, at the call
        c = _ints(xy, 4)
        # (an image that has host pixels by now — somebody loaded it meanwhile — is Pillow's to draw on)
        if c is None or self._image._im is not None:
            return self._owner._hand_over().draw_rectangle(xy, ink, fill, width)
        lst = self._image._draw_list
        x0, y0, x1, y1 = c
        if fill:
            lst.fill(x0, y0, x1, y1, ink)
            return
        w = width or 1
        if w < 0:
            return
        _outline(lst, x0, y0, x1, y1, ink, w)

    def draw_bitmap(self, xy, mask, ink):
        if type(xy) is tuple and len(xy) == 2 and type(xy[0]) is int and type(xy[1]) is int:
            c = xy if -_COORD_MAX < xy[0] < _COORD_MAX and -_COORD_MAX < xy[1] < _COORD_MAX else None
        else:
            c = _ints(xy, 2)
        if (c is None or self._image._im is not None or getattr(mask, "mode", None) != "L"
                or type(ink) is not int):
            return self._owner._hand_over().draw_bitmap(xy, mask, ink)
        mw, mh = mask.size
        self._image._draw_list.blend(c[0], c[1], _bytes_of(mask), mw, mh, ink)

    def __getattr__(self, name):  # draw_lines, draw_polygon, draw_ellipse, ...: Pillow's, on the host image
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self._owner._hand_over(), name)


class DeviceDraw(_PILDraw.ImageDraw):
    """Pillow's ImageDraw on a device image that has no host pixels: the same attributes and all of Pillow's
    Python-level logic, with the C core draw object replaced by a recorder. The image is not loaded."""

    def __init__(self, im):
        # ImageDraw.__init__ for mode "RGB" without im._ensure_mutable() / im.im
        self.palette = None
        self._image = im
        self.mode = "RGB"
        self.draw = _Recorder(self)
        self.ink = self.draw.draw_ink(-1)
        self.fontmode = "L"
        self.fill = False
        if self.font is None:
            self.font = memo_default_font()

    @property
    def im(self):
        """Pillow's text(embedded_color=True) pastes into draw.im: reading it hands the image over to Pillow."""
        self._hand_over()
        return self._image.im

    @im.setter
    def im(self, value):
        raise AttributeError("DeviceDraw.im is the image's own core object")

    def _hand_over(self):
        """Flush what was recorded, materialise the host image as before this class existed, and draw on it with
        Pillow's real core object from here on."""
        if isinstance(self.draw, _Recorder):
            self._image.load()
            self.draw = _PILImage.core.draw(self._image.im, 0)
        return self.draw


# ---------------------------------------------------------------------------------------------------------------
# record_labels: the labels of serve.py:128-136 recorded without Pillow's Python half where that is
# known to give the same list. ImageDraw.text spends its time between the call and the two things that matter here:
# what it asks the font for (getmask2) and what it hands the core object (draw_bitmap). A *stamp* is that pair as
# observed on a real DeviceDraw.text call for one (string, start class pair): per blend the font call (string, mode,
# options; its start is the fractional start) and the offset it returned, the bitmap's position relative to
# (int(x), int(y)) and the ink. Nothing about how ImageDraw.text is written is assumed: a capture whose calls do not
# have exactly that shape is not a stamp, a key is stamped only after two captures at different fractions of its
# class gave the same stamp, and a key whose captures differ is never stamped. A stamp is replayed by asking the font
# again (a memo lookup: the very mask object, so also the very bytes object, that Pillow's path would have blended,
# which keeps the list's one-copy-per-mask rule) and calling DrawList.blend as _Recorder.draw_bitmap does.


class _Capture(_Recorder):
    """The recorder of record_labels' DeviceDraw: during a capture it also notes what draw_bitmap received."""

    seen = None

    def draw_bitmap(self, xy, mask, ink):
        if self.seen is not None:
            self.seen.append((xy, mask, ink))
        return super().draw_bitmap(xy, mask, ink)


_stamps: dict = {}       # (text, cx, cy) -> trusted stamp
_stamp_first: dict = {}  # key -> ((fx, fy), stamp) of its first capture
_stamp_never: set = set()
_stamp_lock = threading.Lock()
stamp_stats = {"hits": 0, "captures": 0, "fallbacks": 0}
_TEXT = {"fill": "white", "stroke_width": 1, "stroke_fill": "black"}  # serve.py:131-136


def _capture_text(draw, x, y, fx, fy, text):
    """DeviceDraw.text for one label, for real (draw.draw is record_labels' _Capture), and the stamp it amounts to
    (None where the image was handed over to Pillow or the calls made are not of the shape a stamp replays)."""
    rec = draw.draw
    calls, seen = [], []
    rec.seen, _capturing.calls = seen, calls
    try:
        draw.text(xy=(x, y), text=text, **_TEXT)
    finally:
        rec.seen = _capturing.calls = None
    if draw._image._im is not None or len(calls) != len(seen) or not seen:
        return None
    ix, iy = int(x), int(y)
    stamp = []
    for (t, mode, args, start, kw, out), (xy, mask, ink) in zip(calls, seen):
        if (args or type(start) is not tuple or start != (fx, fy) or type(out) is not tuple or len(out) != 2
                or out[0] is not mask or getattr(mask, "mode", None) != "L" or type(ink) is not int
                or type(xy) is not tuple or len(xy) != 2 or type(xy[0]) is not int or type(xy[1]) is not int
                or abs(xy[0] - ix) >= 1 << 20 or abs(xy[1] - iy) >= 1 << 20):
            return None
        try:
            opts = _opts(kw)
            hash(opts)
        except TypeError:
            return None
        if type(t) is not str or mode not in ("", "L", "1"):
            return None
        stamp.append((t, mode, dict(kw), tuple(out[1]), xy[0] - ix, xy[1] - iy, ink, opts))
    return tuple(stamp)


def _replay(lst, font, stamp, ix, iy, start, cx, cy) -> bool:
    """Append a stamp's blends at (ix, iy). False, with nothing appended, where the font's answer is not the stamp's."""
    got = []
    for t, mode, kw, offset, _, _, _, opts in stamp:
        hit = font.lookup(t, mode, start[0], start[1], cx, cy, opts)
        mask, off = font.getmask2(t, mode, start=start, **kw) if hit is None else hit
        if tuple(off) != offset or mask.mode != "L":
            return False
        got.append(mask)
    for mask, (_, _, _, _, dx, dy, ink, _) in zip(got, stamp):
        mw, mh = mask.size
        lst.blend(ix + dx, iy + dy, _bytes_of(mask), mw, mh, ink)
    return True


def record_labels(image, boxes, texts) -> None:
    """serve.py:128-136 for one image: per detection `rectangle(box, outline="red", width=3)` then
    `text((box[0] + 5, box[1] + 5), text, fill="white", stroke_width=1, stroke_fill="black")`. On a device image
    without host pixels, `image._draw_list` afterwards holds byte for byte the operations, and the same mask bytes at
    the same offsets, that those calls through draw_module().Draw(image) would have appended: each detection takes
    either a fast path (the rectangle's four fills straight from the box; the text from a trusted stamp) or the
    DeviceDraw calls themselves, and which one is never visible in the list. Any other image is drawn on through
    draw_module().Draw(image). `stamp_stats` counts the texts replayed from a stamp ("hits"), recorded through
    Pillow while their key was being learned ("captures") and recorded through Pillow for good ("fallbacks")."""
    import math

    draw = draw_module().Draw(image)
    if type(draw) is not DeviceDraw:
        for box, text in zip(boxes, texts):
            draw.rectangle(box, outline="red", width=3)
            draw.text(xy=(box[0] + 5, box[1] + 5), text=text, **_TEXT)
        return
    draw.draw = _Capture(draw)
    lst = image._draw_list
    font = draw.font
    stampable = type(font) is _MemoFont and font is _font  # the memoising default font, not ImageDraw.font's
    red = draw.draw.draw_ink(_PILColor.getcolor("red", "RGB"))
    for box, text in zip(boxes, texts):
        # the rectangle: Pillow's argument checks pass for four plain numbers in order, and then the recorder's
        # outline is all that happens
        c = None
        if (image._im is None and type(box) in (list, tuple) and len(box) == 4
                and all(type(v) is float or type(v) is int for v in box) and box[0] <= box[2] and box[1] <= box[3]):
            c = _ints(box, 4)
        if c is None:
            draw.rectangle(box, outline="red", width=3)
        else:
            _outline(lst, c[0], c[1], c[2], c[3], red, 3)
        x, y = box[0] + 5, box[1] + 5
        key = None
        if (stampable and image._im is None and type(text) is str and type(x) is float and type(y) is float
                and 0 <= x < _COORD_MAX and 0 <= y < _COORD_MAX):  # (a NaN fails the comparisons)
            fx, fy = math.modf(x)[0], math.modf(y)[0]
            cx, cy = start_class(fx, _UPPER_X), start_class(fy, _UPPER_Y)
            if cx is not None and cy is not None:
                key = (text, cx, cy)
        if key is None or key in _stamp_never:
            stamp_stats["fallbacks"] += 1
            draw.text(xy=(x, y), text=text, **_TEXT)
            continue
        stamp = _stamps.get(key)
        if stamp is not None and _replay(lst, font, stamp, int(x), int(y), (fx, fy), cx, cy):
            stamp_stats["hits"] += 1
            continue
        got = _capture_text(draw, x, y, fx, fy, text)
        stamp_stats["captures"] += 1
        with _stamp_lock:
            first = _stamp_first.get(key)
            if got is None or stamp is not None or (first is not None and first[1] != got):
                # not a stamp, a trusted stamp the font no longer agrees with, or two captures that differ
                _stamp_never.add(key)
                _stamps.pop(key, None)
                _stamp_first.pop(key, None)
            elif first is None:
                _stamp_first[key] = ((fx, fy), got)
            elif first[0] != (fx, fy):  # a second fraction of the class gave the same stamp
                _stamps[key] = got
                del _stamp_first[key]


_lib_ok = None


def _library_loadable() -> bool:
    global _lib_ok
    if _lib_ok is None:
        try:
            from ._lib import lib

            lib()
            _lib_ok = True
        except (RuntimeError, OSError):
            _lib_ok = False
    return _lib_ok


class _DrawModule(types.ModuleType):
    """`PIL.ImageDraw` as serve.py sees it after the drop-in (module scope): every attribute is
    Pillow's; `Draw(im)` is Pillow's ImageDraw on `im` whose default font memoises its glyph masks. For a device
    image that has not been loaded to the host it is a DeviceDraw: the same class, recording for the GPU."""

    def __init__(self):
        super().__init__("PIL.ImageDraw", _PILDraw.__doc__)

    def __getattr__(self, name):
        return getattr(_PILDraw, name)

    def Draw(self, im, mode=None):  # noqa: N802 - Pillow's name
        if (mode in (None, "RGB") and getattr(im, "_draw_list", None) is not None and im._im is None
                and im.mode == "RGB" and not im.readonly and _library_loadable()):
            return DeviceDraw(im)
        d = _PILDraw.Draw(im, mode)
        if d.font is None:
            d.font = memo_default_font()
        return d


def draw_module() -> types.ModuleType:
    """The `ImageDraw` global the drop-in binds in serve.py (spotter_amd/dropin.py)."""
    return _DrawModule()
