"""References, input families, case lists and bounds of the backbone-front kernels: sp_preprocess_u8's successors up
to ResNet stage 0 (stem.hip, direct_x3.hip, the pools, the upsample and the layout copy of elementwise.hip).

No GPU and no torch: tests/test_front_refs.py checks everything here on the host, tests/test_gpu_front_kernels.py
launches the same cases on the MI355X. DESIGN.md 5.15 states the arguments.

Exact models (bit for bit)
  fmaf32        fp32 fused multiply-add: the fp64 product is exact, the sum is taken with its TwoSum error term and
                rounded to odd in fp64, then rounded to fp32 (53 >= 2·24 + 2 bits: no double rounding).
  stem_model    sp_stem_conv3x3s2_nchw: 27 fmaf in (kh, kw, ci) order from 0, fmaf(s, scale, shift), relu, RNE.
  avgpool_model sp_avgpool2x2_ceil: fp32 adds in (dy, dx) order from 0, divided by the in-map count, RNE.
  maxpool_ref   sp_maxpool3x3s2 by value (±0 ties compare equal; NaN is outside the kernel's contract).

Families
  ints    dense integers in [-4, 4], scale ±{½, 1, 2}, shift and residual multiples of 2^-5: every intermediate is
          exact in fp32 (asserted), so every order of summation gives the reference bit for bit.
  real    (stem, pools) pixels u8 / 255, weights N(0,1) / √27, FrozenBN-like constants; no subnormal intermediate.
  range   (the five MFMA convs) conv_refs' scaled N(0,1) rows and channels, judged per element against `bound`.
  poison  ints or real with NaN (then +inf) at the element the out-of-map loads fall back to.
"""
from __future__ import annotations

import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_refs as cr  # noqa: E402

F32, F64 = np.float32, np.float64
U = cr.U
GUARD, TAIL = cr.GUARD, cr.TAIL
bf16_bits, bf16_val, bf16_round = cr.bf16_bits, cr.bf16_val, cr.bf16_round
POISONS = (np.nan, np.inf)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ------------------------------------------------------------------------------------------------ exact fp32 fma
def fmaf32(a, b, c):
    """fp32 fmaf(a, b, c), element-wise with broadcasting, correctly rounded (NaN / inf propagate as IEEE's do)."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, F32).astype(F64) for v in (a, b, c)))
    with np.errstate(all="ignore"):
        p = a * b  # exact: 48 significant bits, exponent inside fp64's range
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)  # TwoSum: p + c == s + e exactly
        bits = np.array(s, F64).view(np.int64)
        # round to odd: an inexact sum moves to its odd neighbour on the side of the error
        adj = np.isfinite(s) & (e != 0) & ((bits & 1) == 0)
        step = np.where((e > 0) == (s > 0), 1, -1)
        bits = np.where(adj, bits + step, bits)
        return bits.view(F64).astype(F32)


def bits32(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(got, ref, relu=False):
    """Element-wise bit equality of two fp32 arrays. After a relu a zero's sign is not compared: fmaxf(-0, +0) may
    return either (IEEE 754-2008 maxNum), and the kernels' sums can reach -0."""
    eq = bits32(got) == bits32(ref)
    if relu:
        eq |= (np.asarray(got) == 0) & (np.asarray(ref) == 0)
    return eq


# ------------------------------------------------------------------------------------------------ stem conv 1
STEM_SHAPES = [(1, 1, 1), (1, 2, 2), (1, 3, 5), (1, 4, 6), (1, 32, 32), (3, 17, 31), (2, 31, 33)]
STEM_BLOCK = 256


def stem_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def stem_taps(x):
    """NCHW [n, 3, h, w] → [n·ho·wo, 27] in (kh, kw, ci) order, zero outside the map (selected, not multiplied)."""
    n, _, h, w = x.shape
    ho, wo = stem_out(h, w)
    xp = np.zeros((n, 3, h + 2, w + 2), F32)
    xp[:, :, 1:h + 1, 1:w + 1] = x
    cols = [xp[:, ci, kh:kh + 2 * ho - 1:2, kw:kw + 2 * wo - 1:2]
            for kh in range(3) for kw in range(3) for ci in range(3)]
    return np.stack(cols, axis=-1).reshape(n * ho * wo, 27)


def stem_model(x, wt, scale, shift, relu, bf16=False, order=None, track=None):
    """The kernel's chain in fp32: [n·ho·wo, cout] fp32 values (bf16: the values the RNE bits decode to).
    order: a permutation of the 27 taps (the defective emulations); track: a list that receives the smallest
    non-zero magnitude of any intermediate."""
    taps = stem_taps(x)
    s = np.zeros((taps.shape[0], wt.shape[0]), F32)
    lo = np.inf
    for k in (range(27) if order is None else order):
        s = fmaf32(taps[:, k, None], wt[None, :, k], s)
        nz = np.abs(s[(s != 0) & np.isfinite(s)])
        lo = min(lo, nz.min()) if nz.size else lo
    s = fmaf32(s, scale[None, :], shift[None, :])
    nz = np.abs(s[(s != 0) & np.isfinite(s)])
    lo = min(lo, nz.min()) if nz.size else lo
    if track is not None:
        track.append(lo)
    if relu:
        s = np.where(s < 0, F32(0), s)  # fmaxf(s, 0): NaN → 0 as well
        s = np.where(np.isnan(s), F32(0), s)
    return bf16_round(s) if bf16 else s


def build_stem(fam, shape, cout, poison=None):
    """Operands of a stem case: x [n, 3, h, w], wt [cout, 27], scale, shift (fp32)."""
    n, h, w = shape
    rng = _rng("stem", fam, shape, cout)
    if fam == "ints":
        x = rng.integers(-4, 5, (n, 3, h, w)).astype(F32)
        wt = rng.integers(-4, 5, (cout, 27)).astype(F32)
        scale = cr._pick(rng, (1.0, 2.0, 0.5), cout)
        shift = (rng.integers(-64, 65, cout) / 32.0).astype(F32)
        # 27 products of at most 16: every partial sum is an integer below 2^9, the affine a multiple of 2^-5 < 2^11
        pre = stem_taps(x).astype(F64) @ wt.astype(F64).T * scale.astype(F64) + shift.astype(F64)
        cr._exact32(pre, "stem affine", f"stem-{fam}-{shape}-{cout}")
    else:
        x = cr_lut()[rng.integers(0, 256, (n, 3, h, w))]
        wt = (rng.standard_normal((cout, 27)) / np.sqrt(27.0)).astype(F32)
        scale = (rng.uniform(0.5, 1.5, cout) / np.sqrt(rng.uniform(0.25, 4.0, cout) + 1e-5)).astype(F32)
        shift = rng.standard_normal(cout).astype(F32)
    if poison is not None:
        x[:, :, 0, 0] = poison  # where the out-of-map taps of every image and channel plane point
    return x, wt, scale, shift


def cr_lut():
    """f32(f64(v) · (1/255)): the rescale of sp_preprocess_u8."""
    return (np.arange(256, dtype=F64) * (1 / 255)).astype(F32)


# ------------------------------------------------------------------------------------------------ pools
POOL_SHAPES = [(2, 1, 1, 8), (2, 2, 2, 8), (2, 3, 3, 8), (2, 4, 5, 8), (2, 7, 6, 16)]
POOL_RPC4 = (1640, 19, 3, 8)      # n·ho·gx = 16400 >= 16384: rows-per-chunk 4, ho = 10 = 2·4 + 2 (a partial chunk)
POOL_CHUNKS = (33000, 11, 2, 8)   # 2 chunks per image: 66000 > gridDim.y = 65535 while chunked
POOL_ROWS = (33000, 3, 2, 8)      # 66000 output rows > 65535
MP_ROWS, MP_GATE, GRID_Y = 4, 16384, 65535


def maxpool_geom(n, h, w, c, vec):
    """(ho, wo, gx, rpc, chunks) of sp_maxpool3x3s2's launch, as the launcher computes them."""
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gx = (wo * (c // vec) + 255) // 256
    rpc = MP_ROWS if n * ho * gx >= MP_GATE else 1
    return ho, wo, gx, rpc, n * ((ho + rpc - 1) // rpc)


def maxpool_ref(x, prev_bug=False):
    """nn.MaxPool2d(3, 2, 1) on NHWC by value. prev_bug: the walk's carried row maximum taken from row 2·oy instead
    of 2·oy + 1 inside 4-row chunks (the defective emulation)."""
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xp = np.full((n, h + 2, w + 2, c), -np.inf, F32)
    xp[:, 1:h + 1, 1:w + 1] = x
    rowmax = np.maximum(np.maximum(xp[:, :, 0:2 * wo - 1:2], xp[:, :, 1:2 * wo:2]), xp[:, :, 2:2 * wo + 1:2])
    top, mid, bot = rowmax[:, 0:2 * ho - 1:2], rowmax[:, 1:2 * ho:2], rowmax[:, 2:2 * ho + 1:2]
    if prev_bug:
        top = top.copy()
        inner = np.arange(ho) % MP_ROWS != 0
        top[:, inner] = mid[:, np.arange(ho)[inner] - 1]
    return np.maximum(np.maximum(top, mid), bot)


def avgpool_model(x, bf16=False, div4=False):
    """nn.AvgPool2d(2, 2, 0, ceil_mode=True) on NHWC as the kernel computes it. div4: always divide by 4."""
    n, h, w, c = x.shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    xp = np.zeros((n, 2 * ho, 2 * wo, c), F32)
    xp[:, :h, :w] = x
    inside = np.zeros((2 * ho, 2 * wo), bool)
    inside[:h, :w] = True
    s = np.zeros((n, ho, wo, c), F32)
    cnt = np.zeros((ho, wo), F32)
    with np.errstate(over="ignore", invalid="ignore"):
        for dy in range(2):
            for dx in range(2):
                m = inside[dy::2, dx::2]
                s = np.where(m[None, :, :, None], s + xp[:, dy::2, dx::2], s)
                cnt += m
        s = s / (F32(4) if div4 else cnt[None, :, :, None])
    assert s.dtype == F32
    return bf16_round(s) if bf16 else s


def build_pool(fam, shape, bf16, special=None):
    """x [n, h, w, c] fp32 (bf16: bf16-exact). special "inf": ±inf entries and (max) all -inf windows; "big": values
    near the fp32 (bf16) maximum so a 2×2 sum overflows."""
    n, h, w, c = shape
    rng = _rng("pool", fam, shape, bf16, special)
    if fam == "ints":
        x = rng.integers(-4, 5, shape).astype(F32)
    else:
        x = cr_lut()[rng.integers(0, 256, shape)] - F32(0.5)
    if special == "inf":
        x[rng.random(shape) < 0.05] = np.inf
        x[rng.random(shape) < 0.05] = -np.inf
        x[0, :min(h, 3), :min(w, 3)] = -np.inf  # an all -inf 3×3 window around output (0, 0) of image 0
    if special == "big":
        x[rng.random(shape) < 0.5] = 3.0e38
    return bf16_round(x) if bf16 else x


# ------------------------------------------------------------------------------------------------ MFMA 3×3 convs
KINDS = {  # tile rows × columns and the grid cap per CU, as read from the launchers
    "c32": dict(mode="fp32", cin=32, couts=(32, 64), th=8, tw=64, bf16=False, ld=False, file="stem"),
    "c32_bf16": dict(mode="bf16", cin=32, couts=(32, 64), th=4, tw=64, bf16=True, ld=False, file="stem"),
    "c64_bf16": dict(mode="bf16", cin=64, couts=(64,), th=16, tw=32, bf16=True, ld=True, file="stem"),
    "c32_x3": dict(mode="x3", cin=32, couts=(32, 64), th=8, tw=32, bf16=False, ld=False, file="x3"),
    "c64_x3": dict(mode="x3", cin=64, couts=(64,), th=8, tw=32, bf16=False, ld=True, file="x3"),
}
SLICES = [(64, 64), (128, 192), (192, 72)]  # (ldx, ldy) of the c64 kernels' channel-slice cases


def grid_cap(kind, cout, cus):
    return cus * ((3 if cout == 32 else 2) if kind == "c32_bf16" else 1)


def geometry(kind):
    th, tw = KINDS[kind]["th"], KINDS[kind]["tw"]
    return [(2, 1, 1), (2, th - 1, tw + 1), (2, th, tw), (2, th + 1, tw - 1), (2, 2 * th + 1, 2 * tw + 1)]


def walk(kind, cout, cus):
    """Two narrow maps (w = 2, h = k·TH + 1) of cap + 3 and 2·cap + 1 tiles: one workgroup runs two, then three."""
    th, cap = KINDS[kind]["th"], grid_cap(kind, cout, cus)
    return [(1, (cap + 2) * th + 1, 2), (1, 2 * cap * th + 1, 2)]


def tiles(kind, n, h, w):
    th, tw = KINDS[kind]["th"], KINDS[kind]["tw"]
    return n * ((h + th - 1) // th) * ((w + tw - 1) // tw)


def conv3x3_ref(mode, x4, wt, scale, shift, res=None, act=None):
    """fp64 on the mode's operand model: dict(acc, pre, out [M, Cout] fp64, S = Σ|a||w|, knz). fp32: the fp32
    operands' products; bf16: the operands must already be bf16 values; x3: the six kept plane products."""
    acols = cr.im2col(np.ascontiguousarray(x4, F32), 3, 1, 1)
    a, w = acols.astype(F64), wt.astype(F64)
    if mode == "bf16":
        assert np.array_equal(bits32(bf16_round(acols)), bits32(acols)) and np.array_equal(bf16_round(wt), wt)
    with np.errstate(invalid="ignore"):
        if mode == "x3":
            pa = [p.astype(F64) for p in cr.planes_of(acols, "x3")]
            pw = [p.astype(F64) for p in cr.planes_of(wt, "x3")]
            acc = pa[0] @ (pw[0] + pw[1] + pw[2]).T + pa[1] @ (pw[0] + pw[1]).T + pa[2] @ pw[0].T
        else:
            acc = a @ w.T
        pre = acc * scale.astype(F64)[None] + shift.astype(F64)[None]
        if res is not None:
            pre = pre + res.astype(F64)
    fin = np.isfinite(a)
    S = np.abs(np.where(fin, a, 0)) @ np.abs(w).T
    knz = ((a != 0) & fin).astype(F32) @ (w != 0).astype(F32).T
    return dict(acols=acols, acc=acc, pre=pre, out=cr.act64(pre, act), S=S, knz=knz)


def build_conv(kind, fam, shape, cout, act, res=False, poison=None):
    """Operands, reference and bound of a case of one of the five MFMA convs. Returns dict(x [n, h, w, cin], w
    [cout, 9·cin] fp32, w_bits (bf16 kinds), scale, shift, res ([M, cout] bf16-exact fp32 or None), ref [M, cout]
    fp64 (bf16 rows of an exact family: the value of ref_bits), ref_bits, bound)."""
    q = KINDS[kind]
    n, h, w = shape
    cin, mode = q["cin"], q["mode"]
    cid = f"{kind}-{fam}-{n}x{h}x{w}-{cout}-{act}-{res}"
    rng = _rng("conv", kind, fam, shape, cout, act, res)
    m, kk = n * h * w, 9 * cin
    if fam == "ints":
        x = rng.integers(-4, 5, (n, h, w, cin)).astype(F32)
        wt = rng.integers(-4, 5, (cout, kk)).astype(F32)
        scale = cr._pick(rng, (1.0, 2.0, 0.5), cout)
        shift = (rng.integers(-64, 65, cout) / 32.0).astype(F32)
        r = (rng.integers(-128, 129, (m, cout)) / 32.0).astype(F32) if res else None
    else:
        rs = 2.0 ** ((np.arange(m) % 21) - 10.0)
        cs = 2.0 ** ((np.arange(cin) % 9) - 4.0)
        x = (rng.standard_normal((n, h, w, cin)) * (rs[:, None] * cs[None, :]).reshape(n, h, w, cin)).astype(F32)
        wt = rng.standard_normal((cout, kk)).astype(F32)
        scale = (rng.uniform(0.5, 1.5, cout) / np.sqrt(rng.uniform(0.25, 4.0, cout) + 1e-5)).astype(F32)
        shift = rng.standard_normal(cout).astype(F32)
        idx = np.arange(0, cout, 3)
        shift[idx] = np.resize(F32([-100.0, 20.0, -20.0, -90.0]), len(idx))
        if q["bf16"]:
            x, wt = bf16_round(x), bf16_round(wt)
        r = bf16_round((rng.standard_normal((m, cout)) * 4.0).astype(F32)) if res else None
    if poison is not None:
        x[0, 0, 0, :] = poison  # x[0]: where the out-of-map halo chunks point
    out = dict(x=x, w=wt, w_bits=bf16_bits(wt) if q["bf16"] else None, scale=scale, shift=shift, res=r, id=cid)
    f = conv3x3_ref(mode, x, wt, scale, shift, r, act)
    out.update(ref=f["out"], ref_bits=None, bound=None, S=f["S"], acols=f["acols"])
    if poison is not None:
        return out
    if fam == "ints":
        assert kk * 16 < 2 ** 24
        one = np.broadcast_to
        cr._exact32(f["acc"], "accumulator", cid)
        cr._exact32(one(f["acc"] * scale.astype(F64)[None] + shift.astype(F64)[None], f["acc"].shape), "affine", cid)
        cr._exact32(f["pre"], "+res", cid)
        if q["bf16"]:
            out["ref_bits"] = bf16_bits(f["out"].astype(F32))
            out["ref"] = bf16_val(out["ref_bits"]).astype(F64)
    else:
        sc, sh = np.abs(scale.astype(F64))[None], np.abs(shift.astype(F64))[None]
        rv = np.abs(r.astype(F64)) if res else 0.0
        e_acc = cr.C_MODE[mode] * (f["knz"] + 1) * U * f["S"]               # an n-term fp32 sum in any order
        e_pre = e_acc * sc + 4 * U * (np.abs(f["acc"]) * sc + sh + rv)      # the roundings in front of the activation
        bound = e_pre + 2 * U * np.abs(f["out"]) + 2.0 ** -126              # relu / none: Lipschitz 1, exact
        if q["bf16"]:
            bound = bound + 2.0 ** -8 * (np.abs(f["out"]) + bound)          # the RNE store of bf16 rows
        assert np.isfinite(f["out"]).all() and np.isfinite(bound).all(), cid
        out["bound"] = bound
    return out


def poison_window(n, h, w):
    """[n·h·w] bool: the outputs whose 3×3 window holds pixel (0, 0) of image 0."""
    m = np.zeros((n, h, w), bool)
    m[0, :2, :2] = True
    return m.reshape(-1)


def judge(b, got, got_bits=None, relu=False):
    """(worst err / bound, or the count of differing elements; message) of an output [M, cout] against a built case."""
    if b["bound"] is None:
        if got_bits is not None:
            bad = got_bits != b["ref_bits"]
            if relu:
                bad &= ~((got_bits & 0x7FFF == 0) & (b["ref_bits"] & 0x7FFF == 0))
        else:
            bad = ~same_bits(got, b["ref"].astype(F32), relu)
        nb = int(bad.sum())
        return float(nb), f"{b['id']}: {nb} of {bad.size} elements differ from the exact reference"
    err = np.abs(got.astype(F64) - b["ref"])
    ratio = np.where(np.isfinite(err), err / b["bound"], np.inf)
    return float(ratio.max()), f"{b['id']}: worst err / bound {ratio.max():.3f} at " \
                               f"{np.unravel_index(ratio.argmax(), ratio.shape)}"


# ------------------------------------------------------------------------------------------------ upsample, layout
def upsample_ref(x):
    """F.interpolate(scale_factor=2, mode="nearest") on NHWC."""
    return np.repeat(np.repeat(x, 2, axis=1), 2, axis=2)


UPSAMPLE_CASES = [(2, 3, 33, 32), (65600, 1, 1, 4)]  # w·c/4 = 264: a second, partial x-block; n·h = 65600 > 65535
NCHW_CASES = [(1, 3, 1, 1), (2, 3, 37, 41), (3, 1, 5, 7), (2, 4, 9, 6), (2, 3, 420, 420)]
NCHW_GRID_CAP = 256 * 16 * 256  # grid_for's cap in threads: the last case has 1 058 400 > 1 048 576 elements


# ------------------------------------------------------------------------------------------------ preprocess
K_MAX_IMGS, K_LDS_BYTES, K_COL_TILE = 32, 48 * 1024, 256


def band_rows_needed(in_h, out_h):
    """The widest span of source rows a single output row of the vertical pass needs (Pillow's bounds)."""
    sys.path.insert(0, cr.ROOT)
    from oracle.pil_resize import precompute_coeffs

    bounds = precompute_coeffs(in_h, out_h)[0]
    return max(int(b[1]) for b in bounds)
