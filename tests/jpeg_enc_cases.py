"""Inputs of the JPEG encoder's stage tests (tests/test_jpeg_enc_cases.py on the CPU: the premises;
tests/test_gpu_jpeg_enc_stages.py: the four kernels of csrc/jpeg_enc.hip stage by stage). numpy only.

A case is (id, rgb uint8 [H, W, 3], quality, subsampling), subsampling in Pillow's codes 0 / 1 / 2 (4:4:4, 4:2:2,
4:2:0). Images stay at a few MCUs unless the MCU count is the point.

geometry    H, W from {1, 7, 8, 9, 15, 16, 17, 24, 25} x the three subsamplings, noise at quality 50: every
            combination of no / right / bottom / both luma dummy blocks and of the chroma row and column clamps, in
            images of at most 2x2 MCUs at 4:2:0 (4x4 at 4:4:4).
runs        steered coefficients. Gray (R = G = B, so Y = v and Cb = Cr = 128 exactly) images built block by block
            as 128 + IDCT(target * qtable) at quality 50: a lone AC coefficient at zig-zag k for k in RUN_K (the
            8-zero fast path from every entry point, 1 / 2 / 3 ZRL codes, a block ending at coefficient 63: no
            EOB), the same plus a coefficient 16 places earlier (run 15 without ZRL), "ladders" whose gaps give
            every run 0..15, and the lone coefficients again with magnitude 2 and the other sign. The colour
            analogue puts the same targets into Cb, then Cr, under Y = 128. Both at 4:4:4 and 4:2:0 (the colour
            image's pixels doubled, so the 2x2 average returns them).
saturation  full-amplitude blocks at quality 100 and 1 in white / black, blue / yellow and red / cyan: solid
            blocks alternating (DC differences of size 11), pixel column / row stripes and the pixel checker
            (coefficient 63 at full amplitude), the sign patterns of a few DCT bases (AC size 10); at block scale
            and doubled (so 4:2:2 / 4:2:0 chroma saturates as well); uniform noise at quality 100 and 1.
flat        one value per image, 40 MCUs in a row: after the first every 4:4:4 MCU is 14 bits, so two or three
            MCUs share each 32-bit word of the emit kernel's atomic ORs.
mcu counts  4:4:4 images of exactly n MCUs, n in MCU_COUNTS: the fdct kernel's 4 MCUs per workgroup, the bits and
            emit kernels' 256, the scan kernel's 1024 threads with chunk = ceil(n / 1024) (1 -> 2 at 1025, threads
            past n idle; 2049: chunk 3). One MCU row, and the same count over several rows (two where n is even,
            else its smallest divisor 3 or 5, down to one MCU per row; 1 and the prime 257 have no such form) so the DC prediction crosses a
            row end; one 4:2:0 image of 1025 MCUs. Flat content with one noise MCU (seeded choice) in every eight,
            so 14-bit and several-hundred-bit MCUs alternate across workgroup and chunk borders.
"""
from __future__ import annotations

import functools
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import jpeg_enc_np as J  # noqa: E402

GEOMETRY_SIZES = (1, 7, 8, 9, 15, 16, 17, 24, 25)
RUN_K = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62, 63)
# zig-zag positions whose gaps are the runs 0..4 / 5..7 / 8..10 / 11..13 / 14, 15
LADDERS = ((1, 3, 6, 10, 15), (6, 13, 21), (9, 19, 30), (12, 25, 39), (15, 31))
MCU_COUNTS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049)
FLAT_VALUES = (0, 77, 128, 255)
SUBS = (0, 1, 2)

_u = np.arange(8)
# orthonormal DCT-II matrix: F = D f D^T, f = D^T F D
_D = np.sqrt(2 / 8) * np.cos((2 * _u[None, :] + 1) * _u[:, None] * np.pi / 16)
_D[0] /= np.sqrt(2)


def _idct(F):
    return _D.T @ F @ _D


def _zz_block(entries):
    """{zig-zag position: value} -> int64 [64] natural order."""
    b = np.zeros(64, np.int64)
    for k, val in entries.items():
        b[J.NATURAL[k]] = val
    return b


def run_targets():
    """int64 [4, 12, 64] natural order: the quantised blocks the "runs" images are built to give.
    Row 0: a lone +-1 at zig-zag k, k in RUN_K; row 1: the same and a coefficient 16 places earlier (k > 16);
    row 2: the ladders (runs 0..15), then lone coefficients at 8, 24, 40, 56 (the fast path entered after a
    non-zero coefficient ends a group of eight); row 3: lone -+2 at k. DC values vary (0 on the ladders)."""
    t = np.zeros((4, 12, 64), np.int64)
    for i, k in enumerate(RUN_K):
        s = 1 if i % 2 == 0 else -1
        t[0, i] = _zz_block({0: 3 * i - 16, k: s})
        t[1, i] = _zz_block({0: 14 - 2 * i, k: -s, **({k - 16: s} if k > 16 else {})})
        t[3, i] = _zz_block({0: (-1) ** i * (i + 2), k: -2 * s})
    for i, pos in enumerate(LADDERS):
        t[2, i] = _zz_block({k: 1 if j % 2 == 0 else -1 for j, k in enumerate(pos)})
    for i, k in enumerate((8, 24, 40, 56)):
        t[2, 5 + i] = _zz_block({0: 5 - i, 7: 1, k: -1})
    t[2, 9] = _zz_block({0: -7, 7: -1, 63: 1})
    t[2, 10] = _zz_block({0: 9, 16: 1, 32: -1, 48: 1})
    t[2, 11] = _zz_block({0: 0})
    return t


def _plane_from_targets(targets, qtab):
    """float plane [rows * 8, cols * 8]: 128 + IDCT(target * qtab) per block."""
    rows, cols, _ = targets.shape
    pl = np.empty((rows * 8, cols * 8))
    for r in range(rows):
        for c in range(cols):
            F = (targets[r, c] * qtab).reshape(8, 8).astype(np.float64)
            pl[r * 8:r * 8 + 8, c * 8:c * 8 + 8] = 128 + _idct(F)
    return pl


def _double(img):
    return np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)


def gray_run_image():
    pl = np.rint(_plane_from_targets(run_targets(), J.quant_tables(50)[0]))
    assert pl.min() >= 0 and pl.max() <= 255  # no clipping: the targets come back exactly
    return np.repeat(pl.astype(np.uint8)[..., None], 3, axis=2)


def colour_run_targets():
    """The chroma targets of the colour "runs" image: (Cb [6, 12, 64], Cr [6, 12, 64]); rows 0-2 carry run_targets'
    rows 0-2 in Cb, rows 3-5 carry them negated in Cr."""
    t = run_targets()[:3]
    z = np.zeros_like(t)
    return np.concatenate([t, z]), np.concatenate([z, -t])


def colour_run_image():
    q = J.quant_tables(50)[1]
    tcb, tcr = colour_run_targets()
    cb, cr = _plane_from_targets(tcb, q) - 128, _plane_from_targets(tcr, q) - 128
    rgb = np.stack([128 + 1.402 * cr, 128 - 0.344136 * cb - 0.714136 * cr, 128 + 1.772 * cb], axis=-1)
    assert rgb.min() >= 0 and rgb.max() <= 255
    return np.rint(rgb).astype(np.uint8)


PAIRS = {"wb": ((255, 255, 255), (0, 0, 0)), "by": ((0, 0, 255), (255, 255, 0)), "rc": ((255, 0, 0), (0, 255, 255))}
BASES = ((0, 1), (1, 0), (1, 1), (3, 2), (7, 0), (4, 4), (5, 7))


def saturation_image(pair):
    """uint8 [16, 112, 3] in the two colours of `pair`: a row of 14 blocks (solid a, b, a, b; pixel column
    stripes, row stripes, checker; the sign pattern of each basis of BASES) over the same row with the colours
    swapped."""
    a, b = (np.array(c, np.uint8) for c in PAIRS[pair])
    y, x = np.mgrid[0:8, 0:8]
    masks = [np.ones((8, 8), bool), np.zeros((8, 8), bool), np.ones((8, 8), bool), np.zeros((8, 8), bool),
             x % 2 == 0, y % 2 == 0, (x + y) % 2 == 0]
    masks += [np.outer(_D[v], _D[u]) > 0 for v, u in BASES]
    row = np.concatenate(masks, axis=1)
    m = np.concatenate([row, ~row], axis=0)
    return np.where(m[..., None], a, b).astype(np.uint8)


def mcu_count_image(n, rows, hs, vs, seed):
    """uint8 image of exactly n MCUs of (8 hs) x (8 vs) pixels in `rows` MCU rows: flat 100, one MCU of every eight
    (its place drawn from a seeded generator) uniform noise."""
    assert n % rows == 0
    cols = n // rows
    rng = np.random.default_rng(seed)
    img = np.full((rows * 8 * vs, cols * 8 * hs, 3), 100, np.uint8)
    for g in range(0, n, 8):
        m = g + int(rng.integers(0, 8))
        if m < n:
            my, mx = divmod(m, cols)
            img[my * 8 * vs:(my + 1) * 8 * vs, mx * 8 * hs:(mx + 1) * 8 * hs] = rng.integers(
                0, 256, (8 * vs, 8 * hs, 3), dtype=np.uint8)
    return img


def _rows_for(n):
    if n % 2 == 0:
        return 2
    for r in (3, 5):
        if n % r == 0:
            return r
    return None


@functools.lru_cache(maxsize=None)
def geometry_cases() -> tuple:
    out = []
    for h in GEOMETRY_SIZES:
        for w in GEOMETRY_SIZES:
            img = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
            out += [(f"geo {h}x{w} s{sub}", img, 50, sub) for sub in SUBS]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def run_cases() -> tuple:
    g, c = gray_run_image(), colour_run_image()
    return (("runs gray 444", g, 50, 0), ("runs gray 420", g, 50, 2), ("runs colour 444", c, 50, 0),
            ("runs colour 420", _double(c), 50, 2), ("runs colour 422", c, 50, 1))


@functools.lru_cache(maxsize=None)
def saturation_cases() -> tuple:
    out = []
    for pair in PAIRS:
        img = saturation_image(pair)
        for q in (100, 1):
            out += [(f"sat {pair} q{q} s{sub}", img, q, sub) for sub in SUBS]
            out += [(f"sat {pair} x2 q{q} s{sub}", _double(img), q, sub) for sub in (1, 2)]
    noise = np.random.default_rng(5).integers(0, 256, (24, 40, 3), dtype=np.uint8)
    for q in (100, 1):
        out += [(f"sat noise q{q} s{sub}", noise, q, sub) for sub in (0, 2)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flat_cases() -> tuple:
    out = []
    for val in FLAT_VALUES:
        for sub in SUBS:
            hs, vs = J.SAMPLING[sub]
            out.append((f"flat {val} s{sub}", np.full((8 * vs, 40 * 8 * hs, 3), val, np.uint8), 75, sub))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mcu_count_cases() -> tuple:
    out = []
    for n in MCU_COUNTS:
        out.append((f"mcus {n} x1", mcu_count_image(n, 1, 1, 1, n), 90, 0))
        r = _rows_for(n)
        if r:
            out.append((f"mcus {n} x{r}", mcu_count_image(n, r, 1, 1, n + 7), 90, 0))
    out.append(("mcus 1025 x5 420", mcu_count_image(1025, 5, 2, 2, 11), 90, 2))
    return tuple(out)


FAMILIES = {"geometry": geometry_cases, "runs": run_cases, "saturation": saturation_cases, "flat": flat_cases,
            "mcu_counts": mcu_count_cases}


def all_cases() -> tuple:
    return tuple(c for f in FAMILIES.values() for c in f())


def case_by_id(cid):
    return _BY_ID()[cid]


@functools.lru_cache(maxsize=None)
def _BY_ID():
    d = {c[0]: c for c in all_cases()}
    assert len(d) == len(all_cases())
    return d


def pillow(img, quality, subsampling) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


class Reference:
    """The exact expectation of every stage for one case, from the numpy oracle and Pillow alone."""

    def __init__(self, case):
        self.id, self.rgb, self.quality, self.sub = case
        self.comps, self.qt = J.coefficient_blocks(self.rgb, self.quality, self.sub)
        self.blocks = J.scan_order_blocks(self.comps)            # int16 [nmcu * bpm, 64], zig-zag
        self.mcu_bits = J.mcu_bit_counts(self.comps)             # int64 [nmcu]
        self.offsets = np.cumsum(self.mcu_bits) - self.mcu_bits  # exclusive
        self.raw, self.nbits = J.entropy_bits(self.comps, stuff=False)
        self.pillow = pillow(self.rgb, self.quality, self.sub)
        self.nmcu = len(self.mcu_bits)
        self.bpm = len(self.blocks) // self.nmcu
        for a in (self.blocks, self.mcu_bits, self.offsets):
            a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def reference(cid) -> Reference:
    """Computed once per process and shared (read-only) by every test that needs it."""
    return Reference(case_by_id(cid))
