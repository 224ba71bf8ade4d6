"""Plain numpy fp64 references of the encoder-side small kernels (sp_attention, sp_attention_bf16, sp_layernorm,
sp_layernorm_bf16, sp_add_rows), the fp32 error bounds their GPU tests assert, float32 emulations of the kernels'
documented algorithms, and the seeded edge inputs the tests share.

tests/test_encoder_refs.py checks the references against torch float64, the inputs' preconditions and that the
emulations stay inside the bounds, without a GPU; tests/test_gpu_encoder_kernels.py compares the HIP kernels with
the references on the same inputs, elementwise against the bounds.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np

F32 = np.float32
U = 2.0 ** -24                    # fp32 unit roundoff
LN_EPS = float(np.float32(1e-5))  # the eps the fp32 kernels add: the float32 nearest 1e-5
LN_C = 24                         # add-chain allowance of the LayerNorm bound (see layernorm_bound)
LOG2E = 1.4426950408889634


def f64(a):
    return np.asarray(a, dtype=np.float64)


def seed(*what) -> int:
    return zlib.crc32(repr(what).encode())


# ----------------------------------------------------------------------------- bf16
def bf16_bits(a) -> np.ndarray:
    """float32 → bf16 bit patterns (uint16), round to nearest even; finite values past bf16's largest round to
    ±inf, NaN stays NaN (quiet, payload dropped)."""
    a = np.ascontiguousarray(a, dtype=F32)
    b = a.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(a)
    if nan.any():
        r = np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)
    return r


def bf16_float(bits) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_round(a) -> np.ndarray:
    """float32 rounded RNE to bf16, as float32."""
    return bf16_float(bf16_bits(a)).reshape(np.shape(a))


def bf16_trunc(a) -> np.ndarray:
    """float32 with the low 16 bits dropped (round toward zero): the wrong rounding the bias statistic detects."""
    a = np.ascontiguousarray(a, dtype=F32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32).reshape(a.shape)


# ----------------------------------------------------------------------------- attention: reference and bound
def attention(q, k, v, scale):
    """softmax(q kᵀ · scale) v per (batch, head) in fp64. q, k, v [B, H, n, dh] (fp32, widened here) →
    (o [B, H, n, dh], scores s [B, H, n, n], weights a [B, H, n, n])."""
    q, k, v = f64(q), f64(k), f64(v)
    s = np.einsum("bhic,bhjc->bhij", q, k) * float(scale)
    e = np.exp(s - s.max(-1, keepdims=True))
    a = e / e.sum(-1, keepdims=True)
    return a @ v, s, a


def attention_bound(q, k, v, scale, bf16=False):
    """Per-output bound on |kernel − attention(q, k, v, scale)| for a flash-style fp32 kernel (16-key blocks,
    online softmax in base 2, fp32 accumulation), from the operands alone. Returns (tol, o) with o the fp64
    reference. With u = 2⁻²⁴, s_j the fp64 scores of one query, a_j its weights and S_j = scale·Σ_c |q_c||k_jc|:

        δ_j = ((dh + 2)·S_j + 3·|s_j − max s| + 2)·u
        tol = Σ_j a_j δ_j |v_j| + (Σ_j a_j δ_j)·|o| + (n/16 + dh/4 + 8)·u·Σ_j a_j |v_j|

    δ_j bounds, to first order, the relative error of key j's unnormalised weight p_j = exp(s_j − m) as it ends up
    in the numerator and in l:
      * the score is a chain of dh fp32 fmas (error ≤ dh·u·Σ_c |q_c||k_jc|), then one multiply by the fp32 product
        scale·log2 e (itself rounded once): (dh + 2)·u·S_j in the exponent, which is a relative error of p_j. The
        same error in the running maximum m multiplies every p_j and l alike and cancels in acc / l.
      * p_j is first taken relative to the running maximum of its block (one fp32 subtraction) and then carried
        to the final maximum by one corr = exp2(m_old − m_new) per later block (one subtraction each). The maxima
        rise monotonically, so the subtracted magnitudes telescope to |s_j − max s|, each rounded with u; doubled
        because the kernel subtracts in base-2 units (|s|·log2 e, ≤ 1.45·|s|), and once more for l's own copy of
        the corr chain: 3·|s_j − max s|·u.
      * v_exp_f32 is good to one ulp (2u): the + 2.
    The first term of tol is that error through the numerator, the second through the denominator l (first order
    in δ: the largest δ the inputs here reach is a few 1e-3).

    The last term is the accumulation: per 16-key block the accumulator and l take one rescale multiply (n/16),
    the score chain is issued as dh/4 MFMA steps, and 8 covers the tail (two cross-group adds of l, 1/l, the
    multiply by it, the block's pairwise sum of four p). The 16 in-block MFMA additions per block are charged no
    worst case of their own (that would be n·u): each of those roundings is relative to the running partial sum
    and of either sign, and tests/test_encoder_refs.py measures a float32 emulation of the whole algorithm at a few
    percent of tol on every input family. A kernel near 1.0 of tol is therefore already a finding.

    bf16 (sp_attention_bf16): q, k, v are the operands rounded RNE to bf16 (the caller rounds them; the products of
    bf16 values are exact in fp32, so the terms above only get smaller), and P is rounded RNE to bf16 for the
    numerator only while l sums the unrounded values: + 2⁻⁸·Σ_j a_j |v_j|. bf16 carries 8 significant bits, so
    round-to-nearest is off by up to half an ulp = 2⁻⁸ of the value (just above a power of two); 2⁻⁹ is only its
    typical size, and a query whose weight sits on one or two keys (the ascending family) reaches the full 2⁻⁸: the
    float32 emulation with a correct RNE exceeds a 2⁻⁹ term there (1.13 of it at n = 129, dh = 32). Truncation (up
    to 2⁻⁷, always downward) is what the bias statistic below is for."""
    q, k, v = f64(q), f64(k), f64(v)
    n, dh = q.shape[-2], q.shape[-1]
    o, s, a = attention(q, k, v, scale)
    S = np.einsum("bhic,bhjc->bhij", np.abs(q), np.abs(k)) * float(scale)
    delta = ((dh + 2) * S + 3.0 * np.abs(s - s.max(-1, keepdims=True)) + 2.0) * U
    ad = a * delta
    av = a @ np.abs(v)
    tol = ad @ np.abs(v) + ad.sum(-1, keepdims=True) * np.abs(o) + (n / 16.0 + dh / 4.0 + 8.0) * U * av
    if bf16:
        tol = tol + 2.0 ** -8 * av
    return tol, o


def emulate_attention(q, k, v, scale, bf16=False, p_round=bf16_round):
    """The kernels' documented algorithm in float32 numpy: keys in blocks of 16, scores by fp32 accumulation times
    the fp32 constant scale·log2 e, a running maximum, corr = exp2(m − m_new), l = l·corr + Σ p,
    acc = acc·corr + P V, o = acc·(1/l). bf16: q, k, v rounded RNE to bf16 first and P rounded by p_round
    (bf16_round = the kernel, bf16_trunc = the wrong rounding) for the numerator only. → float32 [B, H, n, dh]."""
    q, k, v = (np.asarray(t, dtype=F32) for t in (q, k, v))
    if bf16:
        q, k, v = bf16_round(q), bf16_round(k), bf16_round(v)
    B, H, n, dh = q.shape
    sc = F32(F32(scale) * F32(LOG2E))
    m = np.full((B, H, n), -np.inf, F32)
    l = np.zeros((B, H, n), F32)
    acc = np.zeros((B, H, n, dh), F32)
    with np.errstate(invalid="ignore", under="ignore"):
        for j0 in range(0, n, 16):
            kb, vb = k[:, :, j0:j0 + 16], v[:, :, j0:j0 + 16]
            st = (np.einsum("bhic,bhjc->bhij", q, kb, dtype=F32) * sc).astype(F32)
            mn = np.maximum(m, st.max(-1))
            corr = np.where(np.isneginf(m), F32(0), np.exp2(m - mn)).astype(F32)
            m = mn
            pr = np.exp2(st - mn[..., None]).astype(F32)
            l = (l * corr + pr.sum(-1, dtype=F32)).astype(F32)
            pv = pr if not bf16 else p_round(pr)
            acc = (acc * corr[..., None] + np.einsum("bhij,bhjc->bhic", pv, vb, dtype=F32)).astype(F32)
    return (acc * (F32(1) / l)[..., None]).astype(F32)


# ----------------------------------------------------------------------------- attention: inputs
ATTN_FAMILIES = ("normal", "sharp4", "sharp8", "ascending", "descending", "uniform", "onehot", "bigv")
ONEHOT_GAP = 300.0


class AttnInputs(NamedTuple):
    q: np.ndarray       # [B, H, n, dh] float32, as handed to the kernel
    k: np.ndarray
    v: np.ndarray
    scale: float


def attn_inputs(family, B, H, n, dh) -> AttnInputs:
    """Seeded q, k, v [B, H, n, dh] (fp32) of one family, scale = dh^-0.5:
    normal      N(0, 1).
    sharp4/8    q and k times 4 / 8: scores 16× / 64× wider (|s| up to a few hundred).
    ascending   k_j = (j/n)·30·û + 0.1·noise, q = U(5, 15)·û + 0.1·noise (û a unit vector per head): every
                query's maximum rises in every 16-key block, so corr < 1 each time.
    descending  the same keys reversed: the first block holds the maximum, everything later is rescaled by 1.
    uniform     q = 0: all weights 1/n.
    onehot      k_j = 100·w_j (w_j random unit vectors), q_i = k_t(i) for a random key t(i): one key per query
                scores at least ONEHOT_GAP above the rest, every other exp2 underflows to 0, |s| > 1000.
    bigv        normal q, k; V = ±U(0.5, 1.5)·1e4."""
    rng = np.random.default_rng(seed("enc_attn", family, B, H, n, dh))
    shape = (B, H, n, dh)
    q, k, v = (rng.standard_normal(shape) for _ in range(3))
    if family in ("sharp4", "sharp8"):
        f = 4.0 if family == "sharp4" else 8.0
        q, k = q * f, k * f
    elif family in ("ascending", "descending"):
        uh = rng.standard_normal((B, H, 1, dh))
        uh /= np.linalg.norm(uh, axis=-1, keepdims=True)
        ramp = (np.arange(n, dtype=np.float64) / n)[None, None, :, None]
        if family == "descending":
            ramp = ramp[:, :, ::-1]
        k = ramp * 30.0 * uh + 0.1 * k
        q = rng.uniform(5.0, 15.0, (B, H, n, 1)) * uh + 0.1 * q
    elif family == "uniform":
        q = np.zeros(shape)
    elif family == "onehot":
        w = k / np.linalg.norm(k, axis=-1, keepdims=True)
        k = 100.0 * w
        t = rng.integers(0, n, (B, H, n))
        t[..., 0], t[..., -1] = 0, n - 1  # a winner in the first block and one in the last
        q = np.take_along_axis(k, t[..., None], 2)
    elif family == "bigv":
        v = np.where(rng.random(shape) < 0.5, -1.0, 1.0) * rng.uniform(0.5, 1.5, shape) * 1e4
    elif family != "normal":
        raise ValueError(family)
    return AttnInputs(q.astype(F32), k.astype(F32), v.astype(F32), float(dh) ** -0.5)


class AttnCase(NamedTuple):
    inp: AttnInputs
    ref: np.ndarray     # fp64 [B, H, n, dh] (of the bf16-rounded operands when bf16)
    tol: np.ndarray     # the bound, same shape


@functools.lru_cache(maxsize=None)
def attn_case(family, B, H, n, dh, bf16) -> AttnCase:
    inp = attn_inputs(family, B, H, n, dh)
    ops = (bf16_round(inp.q), bf16_round(inp.k), bf16_round(inp.v)) if bf16 else (inp.q, inp.k, inp.v)
    tol, ref = attention_bound(*ops, inp.scale, bf16=bf16)
    for a in (*inp[:3], ref, tol):
        a.setflags(write=False)
    return AttnCase(inp, ref, tol)


BIAS_SHAPES = ((400, 8, 32), (77, 2, 64))  # (n, heads, dh) of the bf16 bias statistic
BIAS_BAR = 2.0 ** -12


def bias_inputs(n, H, dh, B=2) -> AttnInputs:
    """Normal q, k and V = |N(0, 1)| + 0.5 (every output positive and ≥ 0.5, so (got − ref)/ref is well scaled):
    rounding P to nearest leaves mean((got − ref)/ref) near 0, truncating it leaves about −2⁻⁹."""
    rng = np.random.default_rng(seed("enc_attn_bias", n, H, dh, B))
    q, k, v = (rng.standard_normal((B, H, n, dh)) for _ in range(3))
    return AttnInputs(q.astype(F32), k.astype(F32), (np.abs(v) + 0.5).astype(F32), float(dh) ** -0.5)


def bias_statistic(got, ref) -> tuple[float, float]:
    """(mean, max |·|) of (got − ref)/ref."""
    rel = (f64(got) - ref) / ref
    return float(rel.mean()), float(np.abs(rel).max())


def to_rows(x):
    """[B, H, n, dh] → the kernels' row layout [B·n, H·dh] (head h at columns h·dh)."""
    B, H, n, dh = x.shape
    return np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3)).reshape(B * n, H * dh))


# ----------------------------------------------------------------------------- layernorm
def layernorm(x, g, b, eps=LN_EPS):
    """LayerNorm over the last axis in fp64 (biased variance) → (y, mean [rows, 1], var [rows, 1])."""
    x = f64(x)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * f64(g) + f64(b), mu, var


def layernorm_bound(x, g, b, eps=LN_EPS):
    """Per-output bound on |kernel − layernorm(x, g, b)| for a two-pass fp32 LayerNorm → (tol, y). With
    u = 2⁻²⁴, c = LN_C = 24, δμ = c·u·max|x|, t = |x − μ|, σ' = √(var + eps):

        tol = |g|·(δμ + 2(c + 8)·u·t)/σ' + 2u·(|y| + |b|)

    c is no shorter than the longest add chain of any kernel's reductions (spotter_amd/csrc/elementwise.hip):
    layernorm_kernel adds 16 strided elements per lane and then 6 butterfly steps of wave_sum (22);
    layernorm4_kernel adds 4 float4, each a depth-2 pairwise sum plus the add into the lane's total, and 6 butterfly
    steps (18); layernorm256_kernel the same 12 plus 4 steps of group16_sum (16).
      * The mean is a sum of d terms along chains of ≤ c adds and one divide: off by ≤ (c + 1)·u·max|x|, taken as
        δμ. It shifts every x − μ̂ by δμ (the first term), and its effect on the variance is second order.
      * The variance sums d squares along the same chains: relative error ≤ (c + 3)·u (square, chain, divide), so
        σ' is off by half of that; rstd adds the sqrt and the reciprocal (2u), the subtraction x − μ̂ one u and the
        multiply by rstd one more: below (c + 8)·u relative to t/σ', doubled for the terms first order leaves out
        and the part of δμ the variance sees.
      * The multiply by g and the add of b round once each: u·|y − b| + u·|y| ≤ 2u·(|y| + |b|)."""
    x, g, b = f64(x), f64(g), f64(b)
    y, mu, var = layernorm(x, g, b, eps)
    dmu = LN_C * U * np.abs(x).max(-1, keepdims=True)
    sig = np.sqrt(var + eps)
    tol = np.abs(g) * (dmu + 2 * (LN_C + 8) * U * np.abs(x - mu)) / sig + 2 * U * (np.abs(y) + np.abs(b))
    return tol, y


def _butterfly(s, width):
    """The xor-shuffle reduction over the last axis (64 lanes): width 64 = wave_sum, 16 = group16_sum."""
    o = width // 2
    lanes = np.arange(s.shape[-1])
    while o:
        s = (s + s[..., lanes ^ o]).astype(F32)
        o >>= 1
    return s


def emulate_layernorm(x, g, b, eps=LN_EPS):
    """layernorm_kernel's arithmetic in float32 numpy: lane l sums elements l, l + 64, ... in order, the wave
    reduces by xor butterflies, mean = sum / d, the same again for the squares of x − mean, then
    (x − mean)·rstd·g + b. → float32 [rows, d]."""
    x = np.asarray(x, dtype=F32)
    rows, d = x.shape
    g, b = np.asarray(g, dtype=F32), np.asarray(b, dtype=F32)
    pad = np.zeros((rows, 1024), F32)
    pad[:, :d] = x
    valid = (np.arange(1024) < d).reshape(16, 64)
    v = pad.reshape(rows, 16, 64)

    def reduce(t):
        s = np.zeros((rows, 64), F32)
        for i in range(16):
            s = (s + t[:, i]).astype(F32)
        return _butterfly(s, 64)[:, :1]

    with np.errstate(over="ignore"):
        mean = (reduce(v) / F32(d)).astype(F32)
        t = np.where(valid, (v - mean[:, :, None]).astype(F32), F32(0))
        var = (reduce((t * t).astype(F32)) / F32(d)).astype(F32)
        rstd = (F32(1) / np.sqrt((var + F32(eps)).astype(F32))).astype(F32)
        y = (((x - mean).astype(F32) * rstd).astype(F32) * g).astype(F32) + b
    return y.astype(F32)


LN_FAMILIES = ("plain", "offset4", "offset3", "tiny", "const", "outlier")
LN_CONST = 7.25  # 5 significant bits: every partial sum of up to 1024 of them is exact in fp32


def ln_rows(family, rows, d) -> np.ndarray:
    """Seeded x [rows, d] (fp32):
    plain    N(1, 3²).
    offset4  μ = 1e4, σ = 1;  offset3: μ = 1e3, σ = 0.1 (the mean dwarfs the spread: cancellation in x − mean).
    tiny     μ = 1, σ = 1e-4: variance 1e-8, far below eps.
    const    every element LN_CONST: x − mean is exactly 0 and the output is beta, bit for bit.
    outlier  N(0, 1) with one element per row 1e6."""
    rng = np.random.default_rng(seed("enc_ln", family, rows, d))
    z = rng.standard_normal((rows, d))
    if family == "plain":
        x = z * 3.0 + 1.0
    elif family == "offset4":
        x = 1e4 + z
    elif family == "offset3":
        x = 1e3 + 0.1 * z
    elif family == "tiny":
        x = 1.0 + 1e-4 * z
    elif family == "const":
        x = np.full((rows, d), LN_CONST)
    elif family == "outlier":
        x = z
        x[np.arange(rows), rng.integers(0, d, rows)] = 1e6
    else:
        raise ValueError(family)
    return x.astype(F32)


def ln_params(d):
    """gamma U(0.5, 1.5), beta N(0, 1) (no zeros: a −0.0 in beta would not survive 0 + beta)."""
    rng = np.random.default_rng(seed("enc_ln_params", d))
    return rng.uniform(0.5, 1.5, d).astype(F32), rng.standard_normal(d).astype(F32)


class LnCase(NamedTuple):
    x: np.ndarray
    g: np.ndarray
    b: np.ndarray
    ref: np.ndarray
    tol: np.ndarray


@functools.lru_cache(maxsize=None)
def ln_case(family, rows, d) -> LnCase:
    x = ln_rows(family, rows, d)
    g, b = ln_params(d)
    tol, ref = layernorm_bound(x, g, b)
    for a in (x, g, b, ref, tol):
        a.setflags(write=False)
    return LnCase(x, g, b, ref, tol)


LN_DS = (1, 3, 4, 255, 256, 257, 260, 1020, 1023, 1024)
LN_ROWS = (1, 3, 4, 5, 15, 16, 17, 1001)
# every d at 17 rows; every row count at d = 256 (16 rows per block), 260 (float4, 4 rows per block), 257 (scalar)
LN_SHAPES = tuple(sorted({(d, 17) for d in LN_DS} | {(d, r) for d in (256, 260, 257) for r in LN_ROWS}))


# ----------------------------------------------------------------------------- add_rows
BF16_MAX = float(np.array([0x7F7F0000], np.uint32).view(F32)[0])


def add_rows_special(rows=64, cols=64):
    """a, b [rows, cols] fp32 with, in the first columns of every row: +inf + x, −inf + x, inf − inf (NaN), NaN + x,
    −0.0 + −0.0, +0.0 + −0.0, finite sums past bf16's largest finite value (fp32 keeps them, bf16 rounds them to
    ±inf), sums past fp32's largest (inf in both) and the value midway between BF16_MAX and inf (to inf by the even
    rule); N(0, 1) elsewhere. → (a, b, number of special columns)."""
    rng = np.random.default_rng(seed("enc_add_special", rows, cols))
    a = rng.standard_normal((rows, cols)).astype(F32)
    b = rng.standard_normal((rows, cols)).astype(F32)
    inf, nan = F32(np.inf), F32(np.nan)
    half = np.array([0x7F7F8000], np.uint32).view(F32)[0]  # midway between bf16's largest finite value and inf
    special = [(inf, 1.5), (-inf, 1.5), (inf, -inf), (nan, 2.0), (-0.0, -0.0), (0.0, -0.0), (3.4e38, 0.0),
               (-3.4e38, 0.0), (1.7e38, 1.7e38), (3e38, 3e38), (-3e38, -3e38), (half, 0.0), (1.0, nan)]
    for c, (x, y) in enumerate(special):
        a[:, c], b[:, c] = x, y
    return a, b, len(special)
