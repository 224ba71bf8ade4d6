"""Seeded case builders for the stage tests of the JPEG decode kernels (csrc/jpeg.hip: the IDCT and the upsample +
colour pass, one image per call and batched), numpy only, beside tests/jpeg_stream_writer.py whose `write`,
`components` and `Case` they reuse. tests/test_jpeg_idct_cases.py pins every list on the CPU (Pillow, the host
decoder, oracle.jpeg_np); tests/test_gpu_jpeg_stages.py runs the same lists through the kernels.

1. envelope_blocks(): one 8x8 gray file per block, each labelled with the envelope conditions it trips
   (idct_workgroup's status flag: |dequantised| <= 2^14 - 1, |pass 1| <= 2^14 - 1, pass 2 <= 511, pass 2 >= -512),
   found by a seeded search and kept by class: blocks exactly on either side of both pass-2 bounds among them.
2. three_table_frames(): tq = (0, 1, 2) with three different tables, dense blocks, block counts that put the
   component boundaries inside a workgroup of 32 blocks.
3. edge_grid(): 10 sampling layouts x W, H in {1, 2, 3, 4, 5, 8, 9, 16, 17}, full-range pixel noise: every first /
   last row and column rule, the box replication, every rounding bias.
4. colour_frames(): 256x256 4:4:4 frames whose planes hold every (Cb, Cr), (Y, Cb) and (Y, Cr) pair.
"""
from __future__ import annotations

import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import jpeg_stream_writer as jw  # noqa: E402
from oracle.jpeg_enc_np import AC_LUM, DC_LUM  # noqa: E402
from oracle.jpeg_np import CB, P1, _islow_1d  # noqa: E402

ENV16 = (1 << 14) - 1
CONDITIONS = ("dequantised", "pass 1", "pass 2 high", "pass 2 low")

# the orthonormal 8-point DCT-II: JPEG's forward DCT of a level-shifted block s is D @ s @ D.T
_D = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)]
               for u in range(8)])


def fdct_quantise(samples, quant) -> np.ndarray:
    """samples float [..., 8, 8] (level-shifted), quant [64] or [..., 64] natural order → quantised coefficients
    int64 [..., 64], rounded to nearest and clipped to the +-1023 a baseline stream can carry."""
    c = np.einsum("ux,...xy,vy->...uv", _D, np.asarray(samples, np.float64), _D)
    q = np.asarray(quant, np.float64)
    return np.clip(np.rint(c.reshape(c.shape[:-2] + (64,)) / q), -1023, 1023).astype(np.int64)


def envelope_terms(blocks, quant):
    """Per block, from oracle.jpeg_np._islow_1d in int64 (nothing wraps): (labels bool [n, 4] in CONDITIONS' order,
    largest |dequantised|, largest |pass 1|, pass-2 maximum, pass-2 minimum). blocks int [n, 64], quant [64] or
    [n, 64], natural order."""
    b = np.asarray(blocks, np.int64).reshape(-1, 8, 8) * np.asarray(quant, np.int64).reshape(-1, 8, 8)
    ws = _islow_1d(np.swapaxes(b, 1, 2), CB - P1)
    out = _islow_1d(np.swapaxes(ws, 1, 2), CB + P1 + 3)
    deq, p1 = np.abs(b).max((1, 2)), np.abs(ws).max((1, 2))
    hi, lo = out.max((1, 2)), out.min((1, 2))
    return np.stack([deq > ENV16, p1 > ENV16, hi > 511, lo < -512], 1), deq, p1, hi, lo


class EnvBlock(jw.Case):
    """One block as an 8x8 gray file. cls: the class it was kept for; quant: its table; label: the conditions it
    trips, in CONDITIONS' order; flagged: any(label), what the kernel's status word must say."""

    def __init__(self, cls, k, block, quant):
        block = np.asarray(block, np.int64).reshape(64)
        g = [block.reshape(1, 1, 64)]
        comps = jw.components(g, [(1, 1)], tq=(0,), td=(0,), ta=(0,), ids=(1,))
        data = jw.write(8, 8, comps, {0: [int(x) for x in quant]}, {(0, 0): DC_LUM, (1, 0): AC_LUM}, app=(jw.JFIF,))
        super().__init__(f"{cls} #{k}", data, g, color=0)
        self.cls, self.quant = cls, np.asarray(quant, np.int64)
        lab, self.deq, self.p1, self.hi, self.lo = (x[0] for x in envelope_terms(block[None], self.quant))
        self.label = tuple(bool(x) for x in lab)
        self.flagged = any(self.label)


# class → (label, extra condition on (|pass 1| max, pass-2 max, pass-2 min)), label in CONDITIONS' order
_N, _NPLAIN = 16, 256
_CLASSES = {
    "inside, max 511": ((0, 0, 0, 0), lambda p1, hi, lo: hi == 511),
    "high alone, max 512": ((0, 0, 1, 0), lambda p1, hi, lo: hi == 512),
    "inside, min -512": ((0, 0, 0, 0), lambda p1, hi, lo: lo == -512),
    "low alone, min -513": ((0, 0, 0, 1), lambda p1, hi, lo: lo == -513),
    "both pass-2 bounds": ((0, 0, 1, 1), lambda p1, hi, lo: True),
    "pass 1 with pass 2": (None, lambda p1, hi, lo: True),  # label: pass 1 and at least one pass-2 condition
    "inside, pass 1 >= 16000": ((0, 0, 0, 0), lambda p1, hi, lo: p1 >= 16000),
    "inside": ((0, 0, 0, 0), lambda p1, hi, lo: hi - lo >= 768),  # wide blocks: together they fill [-512, 511]
}


def _search_round(rng, n):
    """n candidate blocks with their flat 8-bit tables: sample-domain noise and two-level patterns in [-560, 560],
    forward DCT, quantised by a table of 1 to 32. Half the patterns have a level close to a pass-2 bound, a quarter
    are nearly flat (one large pass-1 value per row and little else)."""
    q = rng.integers(1, 33, n)
    kind = rng.integers(0, 4, n)
    amp = rng.integers(1, 561, n)[:, None, None]
    noise = rng.uniform(-1.0, 1.0, (n, 8, 8)) * amp
    a = rng.integers(-560, 561, n)
    b = np.where(rng.random(n) < 0.5, rng.integers(-560, 561, n), rng.choice([-513, -512, 511, 512], n))
    two = np.where(rng.random((n, 8, 8)) < rng.random(n)[:, None, None], a[:, None, None], b[:, None, None])
    two = two + rng.uniform(-1.0, 1.0, (n, 8, 8)) * rng.integers(0, 9, n)[:, None, None]
    flat = rng.choice([-1, 1], n)[:, None, None] * rng.integers(490, 521, n)[:, None, None] \
        + rng.uniform(-1.0, 1.0, (n, 8, 8)) * rng.integers(0, 13, n)[:, None, None]
    s = np.where((kind == 0)[:, None, None], noise, np.where((kind == 3)[:, None, None], flat, two))
    s = np.clip(s, -560, 560)
    quant = np.repeat(q[:, None], 64, 1)
    return fdct_quantise(s, quant), quant


@functools.lru_cache(maxsize=None)
def envelope_blocks() -> tuple:
    """The labelled blocks, class by class (_N of each, _NPLAIN of "inside"), then the DC-only blocks under a table of
    8 and the blocks under 16-bit tables. Deterministic: a seeded search, the first blocks of each class kept."""
    rng = np.random.default_rng(21)
    want = {c: (_NPLAIN if c == "inside" else _N) for c in _CLASSES}
    kept = {c: [] for c in _CLASSES}
    for _ in range(12):
        blocks, quant = _search_round(rng, 16384)
        lab, _, p1, hi, lo = envelope_terms(blocks, quant)
        taken = np.zeros(len(blocks), bool)
        for c, (label, extra) in _CLASSES.items():
            if label is None:
                ok = lab[:, 1] & (lab[:, 2] | lab[:, 3]) & ~lab[:, 0]
            else:
                ok = (lab == np.asarray(label, bool)).all(1)
            ok &= extra(p1, hi, lo) & ~taken
            idx = np.flatnonzero(ok)[:want[c] - len(kept[c])]
            taken[idx] = True
            kept[c] += [(blocks[i], quant[i]) for i in idx]
        if all(len(kept[c]) == want[c] for c in _CLASSES):
            break
    out = [EnvBlock(c, k, b, q) for c in _CLASSES for k, (b, q) in enumerate(kept[c])]
    for dc in (511, 512, -512, -513):  # table 8: pass 1 is 32 * DC, every sample DC
        b = np.zeros(64, np.int64)
        b[0] = dc
        out.append(EnvBlock(f"DC {dc} under table 8", 0, b, [8] * 64))
    # 16-bit tables: the dequantised bound trips, and (Parseval) pass 2 with it
    for k, (pos, val, qv) in enumerate(((0, 1, 16384), (0, -1, 16384), (9, 3, 6000), (63, -2, 9000), (1, 1, 65535))):
        b, q = np.zeros(64, np.int64), np.ones(64, np.int64)
        b[pos], q[pos] = val, qv
        b[8] = 5
        out.append(EnvBlock("16-bit table", k, b, q))
    return tuple(out)


def interleaved(blocks) -> list:
    """The blocks reordered so that the flagged ones are spread evenly among the inside ones."""
    ins, outs = [b for b in blocks if not b.flagged], [b for b in blocks if b.flagged]
    n, m = len(blocks), len(outs)
    slots = {k * n // m for k in range(m)}
    ins, outs = iter(ins), iter(outs)
    return [next(outs) if i in slots else next(ins) for i in range(n)]


# ------------------------------------------------------------------------------------------------ frames
S422 = [(2, 1), (1, 1), (1, 1)]
Q2 = [2] * 64
Q3 = [3] * 64
QGRADED = [1 + (k >> 3) + (k & 7) for k in range(64)]  # 1 at DC up to 15 at coefficient 63, natural order
MIXED = dict(jw.LAYOUTS)["y2x2 cb2x1 cr1x2"]


def noise_blocks(rng, width, height, samp, quants, lo=0, hi=256) -> list:
    """Dense blocks per component: pixel noise uniform in [lo, hi), level-shifted, forward DCT, quantised by the
    component's table."""
    maxh, maxv = max(h for h, _ in samp), max(v for _, v in samp)
    mcux, mcuy = -(-width // (8 * maxh)), -(-height // (8 * maxv))
    out = []
    for (h, v), q in zip(samp, quants):
        px = rng.integers(lo, hi, (mcuy * v, mcux * h, 8, 8)) - 128.0
        out.append(fdct_quantise(px, q))
    return out


@functools.lru_cache(maxsize=None)
def three_table_frames() -> tuple:
    """Y, Cb and Cr each on a table of its own (flat 1, flat 3, graded), full-range pixel noise. Per frame (blocks of
    Y / Cb / Cr): 4:4:4 37x21 (15 / 15 / 15) and 17x9 (6 / 6 / 6: fewer than 32 in all), 4:2:0 70x41 (60 / 15 / 15)
    and 16x16 (4 / 1 / 1), y2x2 cb2x1 cr1x2 40x40 (36 / 18 / 18) and 9x17 (8 / 4 / 4)."""
    rng = np.random.default_rng(22)
    qt = {0: jw.Q1, 1: Q3, 2: QGRADED}
    out = []
    for lab, samp, sizes in (("444", jw.S444, ((37, 21), (17, 9))), ("420", jw.S420, ((70, 41), (16, 16))),
                             ("y2x2 cb2x1 cr1x2", MIXED, ((40, 40), (9, 17)))):
        for W, H in sizes:
            g = noise_blocks(rng, W, H, samp, [qt[0], qt[1], qt[2]])
            comps = jw.components(g, samp, tq=(0, 1, 2))
            out.append(jw.Case(f"three tables {lab} {W}x{H}", jw.write(W, H, comps, qt, jw.STD, app=(jw.JFIF,)), g))
    return tuple(out)


EDGE_LAYOUTS = (("420", jw.S420), ("422", S422), ("444", jw.S444)) + tuple(jw.LAYOUTS[:7])
EDGE_SIZES = (1, 2, 3, 4, 5, 8, 9, 16, 17)


@functools.lru_cache(maxsize=None)
def edge_grid() -> tuple:
    """EDGE_LAYOUTS x W x H over EDGE_SIZES, full-range pixel noise under a table of 2: neighbouring chroma samples
    differ by up to 255, so the rounding biases and the edge rules decide pixels. Each case carries .layout, the
    label of its sampling."""
    rng = np.random.default_rng(23)
    out = []
    for lab, samp in EDGE_LAYOUTS:
        for W in EDGE_SIZES:
            for H in EDGE_SIZES:
                g = noise_blocks(rng, W, H, samp, [Q2] * 3)
                data = jw.write(W, H, jw.components(g, samp), {0: Q2, 1: Q2}, jw.STD, app=(jw.JFIF,))
                c = jw.Case(f"{lab} {W}x{H}", data, g)
                c.layout = lab
                out.append(c)
    return tuple(out)


COLOUR_PAIRS = (("cb, cr", 1, 2), ("y, cb", 0, 1), ("y, cr", 0, 2))


@functools.lru_cache(maxsize=None)
def colour_frames() -> tuple:
    """Three 256x256 4:4:4 frames under a table of 1: two planes an x-ramp and a y-ramp 0..255 (a ramp inside each
    block, which the integer IDCT returns exactly: tests/test_jpeg_idct_cases.py), the third noise. Each case
    carries .pair = (component of the x-ramp, component of the y-ramp)."""
    rng = np.random.default_rng(24)
    ramp = np.arange(256.0) - 128.0
    xr = np.broadcast_to(ramp[None, :], (256, 256))
    yr = np.broadcast_to(ramp[:, None], (256, 256))

    def blocks_of(plane):
        return fdct_quantise(plane.reshape(32, 8, 32, 8).transpose(0, 2, 1, 3), jw.Q1)

    out = []
    for lab, cx, cy in COLOUR_PAIRS:
        g = [None] * 3
        g[cx], g[cy] = blocks_of(xr), blocks_of(yr)
        g[3 - cx - cy] = blocks_of(rng.integers(0, 256, (256, 256)) - 128.0)
        data = jw.write(256, 256, jw.components(g, jw.S444), {0: jw.Q1, 1: jw.Q1}, jw.STD, app=(jw.JFIF,))
        c = jw.Case(f"colour domain {lab}", data, g)
        c.pair = (cx, cy)
        out.append(c)
    return tuple(out)
