"""Plain numpy fp64 references of the decoder-side kernels, and the seeded edge inputs their tests share.

References (inputs are the kernels' fp32 arrays widened to fp64): the MSDA core (softmax over L·P,
loc = ref_xy + off·(1/P)·ref_wh·offset_scale, grid_sample bilinear / zeros / align_corners=False, weighted sum),
sigmoid and inverse_sigmoid with its 1e-5 clips, a stable descending top-k, and the post-process decode
(flat index → (query, label), cxcywh → xyxy × (w, h, w, h)).

tests/test_decoder_refs.py checks them on the CPU against oracle/rtdetr_np.py and torch float64 on the inputs
built here; tests/test_gpu_decoder_kernels.py compares the HIP kernels with them on the same inputs.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
EPS32 = float(np.float32(1e-5))  # the clip a float32 clamp(min=1e-5) applies (M2:548-552 on fp32 tensors)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def seed(*what) -> int:
    return zlib.crc32(repr(what).encode())


# ----------------------------------------------------------------------------- references
def sigmoid(x):
    x = f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def inverse_sigmoid(x, eps=EPS32):
    x = np.clip(f64(x), 0.0, 1.0)
    return np.log(np.maximum(x, eps) / np.maximum(1.0 - x, eps))


def topk_stable(x, k):
    """Indices of the k largest along the last axis, value descending, equal values (−0.0 == +0.0) by lower index."""
    x = f64(x)
    n = x.shape[-1]
    order = np.lexsort((np.broadcast_to(np.arange(n), x.shape), -x), axis=-1)
    return order[..., :k]


def sigmoid_order(x, k):
    """The order a correct fp32 sigmoid + top-k gives on inputs whose distinct fp32 sigmoids lie far apart:
    stable argsort of −float32(sigmoid_fp64(x))."""
    return topk_stable(sigmoid(x).astype(F32), k)


def postprocess(logits, boxes, target_hw, k, threshold):
    """logits [B, Q, C], boxes [B, Q, 4] cxcywh, target_hw [B, 2] (h, w) → all k entries per image:
    scores (fp64 sigmoid), labels, xyxy boxes in pixels (fp64), counts of float32 scores > float32 threshold."""
    b, q, c = logits.shape
    flat = np.asarray(logits).reshape(b, q * c)
    idx = sigmoid_order(flat, k)
    scores = np.take_along_axis(sigmoid(flat), idx, 1)
    labels = (idx % c).astype(np.int64)
    qi = idx // c
    bx = np.take_along_axis(f64(boxes), qi[..., None], 1)
    cx, cy, w, h = bx[..., 0], bx[..., 1], bx[..., 2], bx[..., 3]
    th, tw = f64(target_hw)[:, 0:1], f64(target_hw)[:, 1:2]
    xyxy = np.stack([(cx - 0.5 * w) * tw, (cy - 0.5 * h) * th, (cx + 0.5 * w) * tw, (cy + 0.5 * h) * th], -1)
    counts = (scores.astype(F32) > F32(threshold)).sum(1).astype(np.int32)
    return {"scores": scores, "labels": labels, "boxes": xyxy, "counts": counts, "idx": idx}


def grid_sample(value, loc):
    """grid_sample(bilinear, zeros, align_corners=False) at loc in [0, 1] coordinates (grid = 2·loc − 1).
    value [N, H, W, D], loc [N, M, 2] (x, y) → [N, M, D], fp64."""
    value, loc = f64(value), f64(loc)
    n, hh, ww, _ = value.shape
    ix = loc[..., 0] * ww - 0.5  # ((2·loc − 1 + 1)·W − 1) / 2
    iy = loc[..., 1] * hh - 0.5
    x0, y0 = np.floor(ix), np.floor(iy)
    fx, fy = ix - x0, iy - y0
    out = np.zeros(loc.shape[:-1] + (value.shape[-1],))
    rows = np.arange(n)[:, None]
    for dy, wy in ((0, 1.0 - fy), (1, fy)):
        for dx, wx in ((0, 1.0 - fx), (1, fx)):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi <= ww - 1) & (yi >= 0) & (yi <= hh - 1)
            xs = np.where(inside, xi, 0).astype(np.int64)
            ys = np.where(inside, yi, 0).astype(np.int64)
            out += np.where(inside, wx * wy, 0.0)[..., None] * value[rows, ys, xs]
    return out


def msda(value, off_aw, ref, B, Q, heads, head_dim, shapes, points, offset_scale):
    """value [B·S, heads·head_dim], off_aw [B·Q, heads·L·P·3] (offsets (h, l, p, xy), then logits (h, l·P + p)),
    ref [B·Q, 4] → [B·Q, heads·head_dim], fp64."""
    L = len(shapes)
    LP = L * points
    S = sum(h * w for h, w in shapes)
    v = f64(value).reshape(B, S, heads, head_dim)
    oa = f64(off_aw)
    off = oa[:, :heads * LP * 2].reshape(B, Q, heads, LP, 2)
    lg = oa[:, heads * LP * 2:heads * LP * 3].reshape(B, Q, heads, LP)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    aw = e / e.sum(-1, keepdims=True)
    r = f64(ref).reshape(B, Q, 4)
    loc = r[:, :, None, None, :2] + off * (1.0 / points) * r[:, :, None, None, 2:] * float(offset_scale)
    out = np.zeros((B, Q, heads, head_dim))
    start = 0
    for l, (h, w) in enumerate(shapes):
        vl = v[:, start:start + h * w].reshape(B, h, w, heads, head_dim).transpose(0, 3, 1, 2, 4)
        lc = loc[:, :, :, l * points:(l + 1) * points].transpose(0, 2, 1, 3, 4)
        sv = grid_sample(vl.reshape(B * heads, h, w, head_dim), lc.reshape(B * heads, Q * points, 2))
        sv = sv.reshape(B, heads, Q, points, head_dim)
        a = aw[:, :, :, l * points:(l + 1) * points].transpose(0, 2, 1, 3)[..., None]
        out += (sv * a).sum(3).transpose(0, 2, 1, 3)
        start += h * w
    return out.reshape(B * Q, heads * head_dim)


def msda_oracle32(value, off_aw, ref, B, Q, heads, head_dim, shapes, points, offset_scale):
    """The fp32 numpy formulation tests/test_gpu_kernels.py::test_msda_matches_oracle compares the kernel with
    (fp32 locations and oracle.rtdetr_np.grid_sample_bilinear; its softmax and level sum are fp64): the yardstick
    for how far an fp32 evaluation of the formula lies from the fp64 reference."""
    from oracle.rtdetr_np import grid_sample_bilinear

    nH, dh, nP, nL = heads, head_dim, points, len(shapes)
    S = sum(h * w for h, w in shapes)
    D = nH * dh
    offaw = np.asarray(off_aw, F32)
    off = offaw[:, :nH * nL * nP * 2].reshape(B, Q, nH, nL * nP, 2)
    aw = offaw[:, nH * nL * nP * 2:nH * nL * nP * 3].reshape(B, Q, nH, nL * nP).astype(np.float64)
    aw = np.exp(aw - aw.max(-1, keepdims=True))
    aw = aw / aw.sum(-1, keepdims=True)
    r = np.asarray(ref, F32).reshape(B, Q, 4)
    loc = r[:, :, None, None, :2] + off * np.float32(1 / nP) * r[:, :, None, None, 2:] * np.float32(offset_scale)
    vv = np.asarray(value, F32).reshape(B, S, nH, dh)
    exp = np.zeros((B, nH, Q, dh))
    start = 0
    for l, (h, w) in enumerate(shapes):
        vl = vv[:, start:start + h * w].reshape(B, h, w, nH, dh).transpose(0, 3, 1, 2, 4).reshape(B * nH, h, w, dh)
        lc = loc[:, :, :, l * nP:(l + 1) * nP].transpose(0, 2, 1, 3, 4).reshape(B * nH, Q, nP, 2)
        sv = grid_sample_bilinear(vl, lc.astype(np.float32)).reshape(B, nH, Q, nP, dh)
        exp += (sv * aw[:, :, :, l * nP:(l + 1) * nP].transpose(0, 2, 1, 3)[..., None]).sum(3)
        start += h * w
    return exp.transpose(0, 2, 1, 3).reshape(B * Q, D)


def bf16_round(a):
    """fp32 → (bf16 bit patterns as int16, their exact fp32 values), round to nearest even."""
    u = np.ascontiguousarray(a, dtype=F32).view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return bits.view(np.int16), (bits.astype(np.uint32) << 16).view(F32)


# ----------------------------------------------------------------------------- MSDA cases and inputs
MAPS = [(8, 6), (4, 3), (2, 2), (1, 1)]  # (h, w): the smallest maps that keep every level distinct
MAPS_POW2 = [(16, 8), (8, 4), (4, 2)]    # pixel centres and cell borders are exact in fp32


class MsdaCase(NamedTuple):
    id: str
    heads: int
    head_dim: int
    levels: int
    points: int
    layout: str = "aligned"  # "aligned": 16-byte rows; "odd_ld": odd value row stride; "aw_pad": ld_off_aw % 4 != 0
    generic: bool = False    # SP_TUNE_MSDA_GENERIC: the per-lane kernel where the point-sharing one applies
    pow2: bool = False
    bf16: bool = True        # also run with bf16 value rows (the vectorised kernels only)
    B: int = 2
    Q: int = 37              # 74 rows: ragged against 1, 2, 4, 8 and 16 queries per workgroup

    @property
    def shapes(self):
        return (MAPS_POW2 if self.pow2 else MAPS)[:self.levels]


MSDA_CASES = [
    # the point-sharing kernel, and its fallback when the offset rows are not 16-byte aligned
    MsdaCase("h8l_8x32_3x4", 8, 32, 3, 4),
    MsdaCase("h8l_8x32_3x4_pow2", 8, 32, 3, 4, pow2=True),
    MsdaCase("vec64_8x32_3x4_awpad", 8, 32, 3, 4, layout="aw_pad"),
    # the per-lane vectorised kernel at 64, 16, 32, 128 and 256 lanes per query
    MsdaCase("vec64_8x32_3x4_generic", 8, 32, 3, 4, generic=True),
    MsdaCase("vec64_8x32_3x4_generic_pow2", 8, 32, 3, 4, generic=True, pow2=True),
    MsdaCase("vec64_8x32_1x4", 8, 32, 1, 4),
    MsdaCase("vec64_8x32_4x2", 8, 32, 4, 2),
    MsdaCase("vec64_8x32_2x8", 8, 32, 2, 8),
    MsdaCase("vec16_2x32_3x4", 2, 32, 3, 4),
    MsdaCase("vec16_4x16_3x4", 4, 16, 3, 4),
    MsdaCase("vec32_4x32_2x2", 4, 32, 2, 2),
    MsdaCase("vec128_8x64_4x1", 8, 64, 4, 1),
    MsdaCase("vec256_16x64_1x8", 16, 64, 1, 8),
    # fewer workgroups than XCDs in the grid remap
    MsdaCase("h8l_8x32_3x4_3rows", 8, 32, 3, 4, B=1, Q=3),
    MsdaCase("vec64_8x32_3x4_generic_3rows", 8, 32, 3, 4, generic=True, B=1, Q=3),
    # the scalar kernel: one thread per channel
    MsdaCase("scalar_8x32_3x4_oddld", 8, 32, 3, 4, layout="odd_ld", bf16=False),
    MsdaCase("scalar_8x32_3x4_oddld_pow2", 8, 32, 3, 4, layout="odd_ld", pow2=True, bf16=False),
    MsdaCase("scalar_6x32_3x4", 6, 32, 3, 4, bf16=False),    # C = 192: C / 4 = 48 lanes does not divide 256
    MsdaCase("scalar_32x6_2x8", 32, 6, 2, 8, bf16=False),    # head_dim % 4 != 0
    MsdaCase("scalar_10x32_4x2", 10, 32, 4, 2, bf16=False),  # C = 320: a workgroup of more than 256 threads
    MsdaCase("scalar_12x64_3x4", 12, 64, 3, 4, bf16=False),  # C = 768
]
MSDA_RUNS = [(c, False) for c in MSDA_CASES] + [(c, True) for c in MSDA_CASES if c.bf16]
OFFSET_SCALE = 0.5


def _axis_specials(n):
    """Normalised coordinates of an axis of n pixels where bilinear code goes wrong: the centres of the first, an
    interior and the last pixel, every cell border i/n (0 and 1 are ix = −0.5 and n − 0.5), and ix = −1 and n."""
    return ([0.5 / n, (n // 2 + 0.5) / n, (n - 0.5) / n] + [i / n for i in range(n + 1)]
            + [-0.5 / n, (n + 0.5) / n])


def _uniq32(vals):
    return sorted(set(float(F32(v)) for v in vals))


def crafted_rows(shapes, heads, points, rng):
    """The crafted block: a list of (ref[4], offsets [heads, L·P, 2], logits [heads, L·P], far) rows. Offsets are
    zero (ref_xy is the sampling location of every head, level and point) unless the row is about offsets."""
    LP = len(shapes) * points
    rows = []

    def add(ref, off=None, logits=None, far=False):
        off = np.zeros((heads, LP, 2)) if off is None else off
        logits = 2.0 * rng.standard_normal((heads, LP)) if logits is None else logits
        rows.append((np.asarray(ref, np.float64), off, logits, far))

    xs = _uniq32(v for _, w in shapes for v in _axis_specials(w))
    ys = _uniq32(v for h, _ in shapes for v in _axis_specials(h))
    for i in range(max(len(xs), len(ys))):  # every special x and every special y at least once
        add([xs[i % len(xs)], ys[(i + 3) % len(ys)], 0.3, 0.2])
    h0, w0 = shapes[0]
    for y in (-0.5 / h0, 0.0, 1.0, (h0 + 0.5) / h0):  # ix, iy ∈ {−1, −0.5, n − 0.5, n}²: includes the 4 map corners
        for x in (-0.5 / w0, 0.0, 1.0, (w0 + 0.5) / w0):
            add([x, y, 0.3, 0.2])
    # far outside the map: every corner of every sample is invalid, the row's output is exactly 0
    add([1e6, 1e6, 0.3, 0.2], far=True)
    add([-1e6, 1e6, 0.3, 0.2], far=True)
    add([0.5, -1e6, 0.3, 0.2], far=True)
    add([0.5, 0.5, 1.0, 1.0], off=np.full((heads, LP, 2), 1e9), far=True)
    add([0.5, 0.5, 1.0, 1.0], off=np.full((heads, LP, 2), -1e9), far=True)
    # ref_wh = 0: large offsets must not move the location
    add([0.37, 0.61, 0.0, 0.0], off=1e6 * rng.standard_normal((heads, LP, 2)))
    # softmax edges, at spread-out locations so that the weights matter
    spread = lambda: 2.0 * points * rng.standard_normal((heads, LP, 2))  # noqa: E731
    add([0.45, 0.55, 0.5, 0.4], off=spread(), logits=np.full((heads, LP), 0.7))
    add([0.55, 0.45, 0.5, 0.4], off=spread(), logits=np.full((heads, LP), -80.0))
    lg = 2.0 * rng.standard_normal((heads, LP))
    for h in range(heads):
        lg[h, h % LP] = lg[h].max() + 100.0
    add([0.5, 0.5, 0.5, 0.4], off=spread(), logits=lg)
    return rows


class MsdaInputs(NamedTuple):
    value: np.ndarray    # [B·S, C] fp32 (the columns of the value view)
    off_aw: np.ndarray   # [B·Q, heads·L·P·3] fp32
    ref: np.ndarray      # [B·Q, 4] fp32
    far_rows: np.ndarray
    crafted: int         # rows [0, crafted) are the crafted block
    starts: tuple
    S: int


@functools.lru_cache(maxsize=None)
def msda_inputs(case: MsdaCase) -> MsdaInputs:
    rng = np.random.default_rng(seed("msda", case.id))
    shapes = case.shapes
    heads, P = case.heads, case.points
    LP = len(shapes) * P
    R = case.B * case.Q
    S = sum(h * w for h, w in shapes)
    starts = tuple(int(s) for s in np.cumsum([0] + [h * w for h, w in shapes])[:-1])
    C = heads * case.head_dim
    value = rng.standard_normal((case.B * S, C)).astype(F32)
    craft = crafted_rows(shapes, heads, P, rng)
    if R >= 74:
        assert len(craft) <= R - 20, (len(craft), R)  # at least 20 random rows
    else:
        craft = craft[:R - 1]
    n = len(craft)
    off = np.empty((R, heads, LP, 2))
    lg = np.empty((R, heads, LP))
    ref = np.empty((R, 4))
    for i, (r, o, g, _) in enumerate(craft):
        ref[i], off[i], lg[i] = r, o, g
    # random block: ref_xy on [0, 1], ref_wh on [0.01, 0.9], offsets scaled so that about a third of the samples
    # fall outside the map (loc = ref_xy + off·(1/P)·ref_wh·0.5), logits 2·N(0, 1)
    ref[n:, :2] = rng.uniform(0.0, 1.0, (R - n, 2))
    ref[n:, 2:] = rng.uniform(0.01, 0.9, (R - n, 2))
    off[n:] = 1.0 * P * rng.standard_normal((R - n, heads, LP, 2))
    lg[n:] = 2.0 * rng.standard_normal((R - n, heads, LP))
    off_aw = np.concatenate([off.reshape(R, -1), lg.reshape(R, -1)], 1).astype(F32)
    far = np.array([i for i, c in enumerate(craft) if c[3]], np.int64)
    return MsdaInputs(value, off_aw, ref.astype(F32), far, n, starts, S)


class MsdaExpected(NamedTuple):
    value: np.ndarray        # the fp32 values the kernel samples (bf16-rounded for bf16 rows)
    bits: np.ndarray | None  # their bf16 bit patterns (int16), bf16 rows only
    ref: np.ndarray          # fp64 reference [B·Q, C]
    oracle_err: float        # max |fp32 oracle − ref|
    acc_bound: float         # (4·L·P + 8)·2⁻²⁴·max|value|
    bar: float               # max(4·oracle_err, acc_bound), absolute


@functools.lru_cache(maxsize=None)
def msda_expected(case: MsdaCase, bf16: bool) -> MsdaExpected:
    inp = msda_inputs(case)
    bits, value = bf16_round(inp.value) if bf16 else (None, inp.value)
    args = (value, inp.off_aw, inp.ref, case.B, case.Q, case.heads, case.head_dim, case.shapes, case.points,
            OFFSET_SCALE)
    ref = msda(*args)
    oracle_err = float(np.abs(msda_oracle32(*args) - ref).max())
    acc = (4 * case.levels * case.points + 8) * 2.0 ** -24 * float(np.abs(value).max())
    for a in (ref, value):
        a.setflags(write=False)
    return MsdaExpected(value, bits, ref, oracle_err, acc, max(4.0 * oracle_err, acc))


def outside_fraction(case: MsdaCase) -> float:
    """Share of the random block's samples whose location lies outside [0, 1]²."""
    inp = msda_inputs(case)
    LP = case.levels * case.points
    n = inp.crafted
    off = f64(inp.off_aw[n:, :case.heads * LP * 2]).reshape(-1, case.heads, LP, 2)
    r = f64(inp.ref[n:])
    loc = r[:, None, None, :2] + off / case.points * r[:, None, None, 2:] * OFFSET_SCALE
    return float(((loc < 0) | (loc > 1)).any(-1).mean())


# ----------------------------------------------------------------------------- top-k / post-process inputs
GRID = np.arange(-512, 257, dtype=np.float64) / 64.0  # logits j/64: adjacent fp32 sigmoids ≥ 4665 ulp apart
SATURATED = np.array([20.0, 25.0, 30.0])              # sigmoid == 1.0f in fp32 and in fp64 rounded to fp32


def grid_logits(rng, shape, saturated=0.01, zeros=0.0):
    """Logits drawn from GRID (many repeats), a share `saturated` of them from SATURATED and a share `zeros`
    set to exactly 0 (sigmoid exactly 0.5)."""
    x = GRID[rng.integers(0, len(GRID), shape)]
    u = rng.uniform(0, 1, shape)
    x = np.where(u < saturated, SATURATED[rng.integers(0, 3, shape)], x)
    x = np.where(u > 1.0 - zeros, 0.0, x)
    return x.astype(F32)


TARGET_SIZES = np.array([[1, 3000], [4320, 7680], [717, 1200], [640, 640]], np.int32)  # (h, w) per image


def postprocess_inputs(q, c, k, rng):
    """4 images of grid logits [4, Q, C] and boxes [4, Q, 4]: image 0's top k straddle sigmoid == 0.5 (k // 3 positive
    logits, k // 3 exactly 0, the rest negative); image 1 is saturated (more than k logits ≥ 20 where Q·C allows:
    the winners are the lowest flat indices); image 2 has no saturated logit; image 3 a few."""
    n = q * c
    lg = np.empty((4, n), F32)
    neg = GRID[GRID < 0]
    lg[0] = neg[rng.integers(0, len(neg), n)]
    pos = rng.permutation(n)[:2 * (k // 3)]
    lg[0, pos[:k // 3]] = GRID[GRID > 0][rng.integers(0, (GRID > 0).sum(), k // 3)]
    lg[0, pos[k // 3:]] = 0.0
    lg[1] = grid_logits(rng, n, saturated=0.0)
    sat = rng.permutation(n)[:min(n, k + 17)]
    lg[1, sat] = SATURATED[rng.integers(0, 3, len(sat))]
    lg[2] = grid_logits(rng, n, saturated=0.0)
    lg[3] = grid_logits(rng, n, saturated=0.01, zeros=0.01)
    boxes = rng.uniform(0.05, 0.95, (4, q, 4)).astype(F32)
    return lg.reshape(4, q, c), boxes


def ulp_gaps32(vals):
    """Distances in fp32 ulps between consecutive positive float32 values."""
    bits = np.asarray(vals, F32).view(np.int32).astype(np.int64)
    return np.diff(bits)


def special_rows(n, reduce_c, rng):
    """3 rows of n·reduce_c values: ±inf, ±FLT_MAX, ±1e-40 denormals and signed zeros among ordinary values (each
    special several times: ties), an all-negative row, and a row of one repeated value."""
    m = n * reduce_c
    x = rng.standard_normal((3, m)).astype(F32)
    sp = np.array([np.inf, -np.inf, FLT_MAX, -FLT_MAX, 1e-40, -1e-40, 0.0, -0.0], F32)
    pos = rng.permutation(m)[:min(m // 2, 48)]
    x[0, pos] = sp[np.arange(len(pos)) % len(sp)]
    x[1] = -np.abs(x[1]) - F32(0.25)
    x[1, rng.permutation(m)[:5]] = [-np.inf, -FLT_MAX, -1e-40, -FLT_MAX, -np.inf]
    x[2] = F32(-1.75)
    return x


def signed_zero_rows(n, k, rng):
    """3 rows whose k-th largest value is a zero inside a run of mixed −0.0 / +0.0: `k // 2` positive values, then
    zeros of both signs across the cut, the rest negative, all shuffled."""
    x = np.empty((3, n), F32)
    for r in range(3):
        npos = k // 2 - r
        nzero = k + 2 * r
        row = np.concatenate([rng.uniform(0.5, 2.0, npos), np.where(rng.uniform(0, 1, nzero) < 0.5, -0.0, 0.0),
                              -rng.uniform(0.5, 2.0, n - npos - nzero)])
        x[r] = row[rng.permutation(n)]
    return x


# ----------------------------------------------------------------------------- box kernels' inputs
ANCHOR_SHAPES = [(2, 64), (3, 3), (1, 1), (1, 1), (1, 1), (1, 1)]  # level 0's border columns and level 5 are invalid


def ref_init_inputs(batch, k, rng):
    """Anchor logits (oracle.rtdetr_np.anchors_for; invalid rows are FLT_MAX), selected indices that include
    invalid rows, the first and the last anchor and repeats, and deltas that include 0, ±20 and ±100."""
    from oracle.rtdetr_np import anchors_for

    with np.errstate(invalid="ignore"):  # log of the invalid rows, which anchors_for then replaces
        anchors, valid = anchors_for(ANCHOR_SHAPES)
    valid = valid.reshape(-1)
    n = len(anchors)
    idx = rng.integers(0, n, (batch, k)).astype(np.int32)
    bad = np.flatnonzero(~valid)
    idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3] = 0, n - 1, bad[len(bad) // 2], idx[:, 4]
    idx[:, 5:5 + min(len(bad), 6)] = bad[:6]
    delta = rng.standard_normal((batch * k, 4)).astype(F32)
    sp = np.array([0.0, 20.0, -20.0, 100.0, -100.0], F32)
    flat = delta.reshape(-1)
    flat[::3] = sp[np.arange(len(flat[::3])) % len(sp)]
    return anchors, valid, idx, delta


def box_refine_inputs(rows, rng):
    """Reference boxes that include exactly 0, 1, 1e-5, 1 − 1e-5, 5e-6 and values just outside [0, 1] among uniform
    interior values; two delta sets (the decoder chains the kernel) that include 0 and ±15."""
    ref = rng.uniform(0.02, 0.98, (rows, 4)).astype(F32)
    sp = np.array([0.0, 1.0, 1e-5, 1.0 - 1e-5, 5e-6, -1e-3, 1.001, -0.0, 1.0 - 5e-6, 2e-5], F32)
    flat = ref.reshape(-1)
    flat[:6 * len(sp)] = np.tile(sp, 6)  # each special meets several deltas
    deltas = []
    for _ in range(2):
        d = (0.5 * rng.standard_normal((rows, 4))).astype(F32)
        df = d.reshape(-1)
        df[:6 * len(sp)] = np.repeat(np.array([0.0, 15.0, -15.0, 0.3, -2.0, 1.0], F32), len(sp))
        df[6 * len(sp)::7] = 0.0
        deltas.append(d)
    return ref, deltas


def sigmoid32(x):
    """oracle.rtdetr_np.sigmoid (the fp32 numpy restatement), with expf's overflow to inf for x < −88 accepted."""
    from oracle.rtdetr_np import sigmoid as s32

    with np.errstate(over="ignore"):
        return s32(np.asarray(x, F32))
