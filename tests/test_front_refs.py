"""tests/front_refs.py checked on the host, before any GPU sees it: the fmaf emulation against rational arithmetic,
float32 emulations of each documented algorithm against the exact families and the range bound, five defective
emulations against the cases aimed at them, the geometric conditions of every case list. No GPU.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as cr  # noqa: E402
import front_refs as R  # noqa: E402
from test_conv_refs import ORDERS  # noqa: E402  (sequential, blocks of 8, pairwise: fp32 sums of exact fp64 terms)

F32, F64 = np.float32, np.float64
CUS = 256  # the case lists are relative to the device's CU count; the host checks them at the MI355X's


@pytest.fixture(scope="module", autouse=True)
def _lib_built():
    from spotter_amd import _lib

    _lib.load()


# ---------------------------------------------------------------------------------------------- fmaf
def _round_f32(q: Fraction) -> float:
    """A rational rounded to the nearest fp32 (ties to even), subnormals included, by integer arithmetic."""
    if q == 0:
        return 0.0
    e = -149
    while abs(q) / Fraction(2) ** e >= 2 ** 24:
        e += 1
    n = round(q / Fraction(2) ** e)  # Python rounds a Fraction half to even
    v = float(n) * 2.0 ** e          # n <= 2^24 and the power are exact in fp64
    return float(F32(v))             # overflow → inf


def test_fmaf32_equals_rational_arithmetic():
    rng = np.random.default_rng(11)
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)
    # cancellation: c close to -a·b
    c[:600] = -(a[:600].astype(F64) * b[:600].astype(F64)).astype(F32)
    # constructed ties: a·b = odd · odd / 2 < 2^21 ends in one half, c = 2^23 or -2^24 puts the sum where fp32's
    # spacing is 1: exactly between two neighbours
    k = 1000
    ma = rng.integers(2 ** 9, 2 ** 10, k) * 2 + 1
    mb = rng.integers(2 ** 9, 2 ** 10, k) * 2 + 1
    ta, tb = ma.astype(F32), (mb * 2.0 ** -1).astype(F32)
    tc = rng.choice([2.0 ** 23, -2.0 ** 24], k).astype(F32)
    a, b, c = np.concatenate([a, ta]), np.concatenate([b, tb]), np.concatenate([c, tc])
    got = R.fmaf32(a, b, c)
    ties = 0
    for i in range(len(a)):
        q = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        want = _round_f32(q)
        assert float(got[i]) == want and np.signbit(got[i]) == np.signbit(F32(want)) or q == 0, (i, a[i], b[i], c[i])
        if q != 0 and i >= n:
            lo = F32(want)
            ulp = abs(float(np.nextafter(lo, F32(np.inf))) - float(lo))
            ties += abs(q - Fraction(float(lo))) * 2 == Fraction(ulp)
    assert ties == k, ties  # every constructed triple is an exact tie
    # a separate fp32 multiply and add is another function: the cancellation triples tell them apart
    assert (a * b + c != got).sum() > 500


def test_fmaf32_specials():
    assert np.isnan(R.fmaf32(np.nan, 1.0, 0.0)) and np.isnan(R.fmaf32(np.inf, 0.0, 1.0))
    assert R.fmaf32(np.inf, 2.0, 1.0) == np.inf and R.fmaf32(3e38, 3e38, 0.0) == np.inf
    assert np.signbit(R.fmaf32(-1.0, 0.0, 0.0)) == 0  # -0 + +0 = +0
    assert R.fmaf32(2.0 ** -75, 2.0 ** -75, 0.0) == 0.0 and R.fmaf32(2.0 ** -75, 2.0 ** -74, 0.0) == F32(2.0 ** -149)


# ---------------------------------------------------------------------------------------------- stem
def _stem_emulation(x, wt, scale, shift, relu, zero_halo=True, order=None):
    """fp32 emulation of the kernel with its own addressing: per pixel the 27 taps gathered with `ok ? v : 0`
    (zero_halo False: multiplied by the mask instead, which lets a NaN at x[0] through)."""
    n, _, h, w = x.shape
    ho, wo = R.stem_out(h, w)
    out = np.zeros((n * ho * wo, wt.shape[0]), F32)
    taps = np.zeros((n * ho * wo, 27), F32)
    for p in range(n * ho * wo):
        ox, oy, b = p % wo, (p // wo) % ho, p // (wo * ho)
        for kh in range(3):
            for kw in range(3):
                iy, ix = 2 * oy - 1 + kh, 2 * ox - 1 + kw
                ok = 0 <= iy < h and 0 <= ix < w
                for ci in range(3):
                    v = x[b, ci, iy if ok else 0, ix if ok else 0]
                    with np.errstate(invalid="ignore"):
                        taps[p, (kh * 3 + kw) * 3 + ci] = (v if ok else F32(0)) if zero_halo else v * F32(ok)
    s = np.zeros_like(out)
    for k in (order or range(27)):
        s = R.fmaf32(taps[:, k, None], wt[None, :, k], s)
    s = R.fmaf32(s, scale[None], shift[None])
    return np.where(s > 0, s, F32(0)) if relu else s


@pytest.mark.parametrize("shape", R.STEM_SHAPES[:6])
@pytest.mark.parametrize("fam", ["ints", "real"])
def test_stem_model_equals_the_pixelwise_emulation(shape, fam):
    x, wt, sc, sh = R.build_stem(fam, shape, 32)
    track = []
    ref = R.stem_model(x, wt, sc, sh, relu=False, track=track)
    assert track[0] >= 2.0 ** -126, track  # no subnormal intermediate: flush-to-zero could not change the result
    emu = _stem_emulation(x, wt, sc, sh, False)
    assert R.same_bits(emu, ref).all()
    if fam == "ints":  # exact in any order: the fp64 sum is the reference as well
        pre = R.stem_taps(x).astype(F64) @ wt.astype(F64).T * sc.astype(F64) + sh.astype(F64)
        assert np.array_equal(ref.astype(F64), pre)
    # a swapped pair of taps gives other values
    swapped = list(range(27))
    swapped[12], swapped[13] = swapped[13], swapped[12]  # the centre tap's channels 0 and 1: always inside the map
    wrong = R.stem_model(x, wt[:, swapped], sc, sh, relu=False)
    assert (~R.same_bits(wrong, ref)).any(), "a swapped tap goes unnoticed"


def test_stem_real_is_order_sensitive():
    """The real family tells summation orders apart, which a 2e-4 tolerance does not: the reversed chain differs in
    bits but by less than 2e-4."""
    x, wt, sc, sh = R.build_stem("real", (1, 32, 32), 32)
    ref = R.stem_model(x, wt, sc, sh, relu=False)
    rev = R.stem_model(x, wt, sc, sh, relu=False, order=list(range(26, -1, -1)))
    assert (~R.same_bits(rev, ref)).any() and np.abs(rev - ref).max() < 2e-4


@pytest.mark.parametrize("poison", R.POISONS)
def test_stem_poison_marks_only_output_00_and_catches_a_multiplied_mask(poison):
    shape = (3, 4, 6)
    clean = R.stem_model(*R.build_stem("real", shape, 32), relu=False)
    x, wt, sc, sh = R.build_stem("real", shape, 32, poison=poison)
    ref = R.stem_model(x, wt, sc, sh, relu=False).reshape(3, 2, 3, 32)
    first = np.zeros((3, 2, 3), bool)
    first[:, 0, 0] = True
    assert np.isfinite(ref[~first]).all() and not np.isfinite(ref[first]).any()
    assert R.same_bits(ref[~first], clean.reshape(3, 2, 3, 32)[~first]).all()
    masked = _stem_emulation(x, wt, sc, sh, False, zero_halo=False).reshape(3, 2, 3, 32)
    assert not np.isfinite(masked[~first]).all(), "a halo multiplied by its mask goes unnoticed"


# ---------------------------------------------------------------------------------------------- MFMA convs
def _conv_emulation(kind, b, act, order, res_after_relu=False, zero_halo=True, poison_x=None):
    """fp32 emulation of a direct 3×3 kernel: the mode's exact products summed in fp32 in `order`, fmaf(acc, scale,
    shift), + res, relu, RNE for bf16 rows."""
    q = R.KINDS[kind]
    a = b["acols"]
    if q["mode"] == "x3":
        pa, pw = cr.planes_of(a, "x3"), cr.planes_of(b["w"], "x3")
        t = np.stack([pa[i].astype(F64)[:, None, :] * pw[j].astype(F64)[None, :, :] for i, j in cr.KEPT["x3"]], -1)
        t = t.reshape(t.shape[0], t.shape[1], -1)
    else:
        t = a.astype(F64)[:, None, :] * b["w"].astype(F64)[None, :, :]
    acc = ORDERS[order](t)
    v = R.fmaf32(acc, b["scale"][None], b["shift"][None])
    relu = lambda z: np.maximum(z, F32(0))
    if b["res"] is not None and not res_after_relu:
        v = v + b["res"]
    if act == "relu":
        v = relu(v)
    if b["res"] is not None and res_after_relu:
        v = v + b["res"]
    assert v.dtype == F32
    bits = R.bf16_bits(v) if q["bf16"] else None
    return (R.bf16_val(bits) if q["bf16"] else v), bits


SMALL = [(kind, cout) for kind, q in R.KINDS.items() for cout in q["couts"]]


@pytest.mark.parametrize("kind,cout", SMALL)
@pytest.mark.parametrize("order", list(ORDERS))
def test_conv_emulations_equal_ints_and_stay_inside_the_range_bound(kind, cout, order):
    shape = (2, 3, 5)
    for act in (None, "relu"):
        res = kind == "c64_bf16" and act == "relu"
        b = R.build_conv(kind, "ints", shape, cout, act, res=res)
        got, bits = _conv_emulation(kind, b, act, order)
        nb, msg = R.judge(b, got, bits, relu=act == "relu")
        assert nb == 0, msg
        b = R.build_conv(kind, "range", shape, cout, act, res=res)
        got, bits = _conv_emulation(kind, b, act, order)
        worst, msg = R.judge(b, got)
        assert worst <= 1.0, msg


def test_residual_after_relu_differs_on_ints():
    b = R.build_conv("c64_bf16", "ints", (2, 3, 5), 64, "relu", res=True)
    got, bits = _conv_emulation("c64_bf16", b, "relu", "sequential", res_after_relu=True)
    assert R.judge(b, got, bits, relu=True)[0] > 0
    b = R.build_conv("c64_bf16", "range", (2, 3, 5), 64, "relu", res=True)
    got, bits = _conv_emulation("c64_bf16", b, "relu", "sequential", res_after_relu=True)
    assert R.judge(b, got)[0] > 1.0


@pytest.mark.parametrize("kind", list(R.KINDS))
@pytest.mark.parametrize("poison", R.POISONS)
def test_conv_poison_reference_is_finite_outside_the_windows(kind, poison):
    """The reference of a poison case is non-finite exactly in the four outputs whose window holds x[0], and a halo
    that is loaded from x[0] without being zeroed (the value multiplied by its mask) reaches other outputs."""
    cout = R.KINDS[kind]["couts"][0]
    n, h, w = R.geometry(kind)[1]
    b = R.build_conv(kind, "ints", (n, h, w), cout, None, poison=poison)
    win = R.poison_window(n, h, w)
    assert not np.isfinite(b["ref"][win]).any() and np.isfinite(b["ref"][~win]).all()
    # the unzeroed halo: every out-of-map tap carries x[0]'s channels
    x = b["x"]
    xp = np.empty((n, h + 2, w + 2, x.shape[3]), F32)
    xp[:] = x[0, 0, 0]
    xp[:, 1:-1, 1:-1] = x
    cols = [xp[:, i:i + h, j:j + w] for i in range(3) for j in range(3)]
    a = np.stack(cols, 3).reshape(n * h * w, -1).astype(F64)
    with np.errstate(invalid="ignore"):
        bad = a @ b["w"].astype(F64).T
    border = np.ones((n, h, w), bool)
    border[:, 1:-1, 1:-1] = False
    assert not np.isfinite(bad[border.reshape(-1) & ~win]).any(), "an unzeroed halo goes unnoticed"


# ---------------------------------------------------------------------------------------------- pools
def _maxpool_walk(x, rpc, prev_bug=False):
    """The kernels' row walk: chunks of rpc output rows, the 3-tap maximum of input row 2·oy + 1 carried."""
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = np.empty((n, ho, wo, c), F32)

    def hmax(b, iy, ox):
        m = np.full(c, -np.inf, F32)
        if 0 <= iy < h:
            for dx in range(3):
                ix = 2 * ox - 1 + dx
                if 0 <= ix < w:
                    m = np.maximum(m, x[b, iy, ix])
        return m

    for b in range(n):
        for oy0 in range(0, ho, rpc):
            for ox in range(wo):
                prev = hmax(b, 2 * oy0 - 1, ox)
                for oy in range(oy0, min(oy0 + rpc, ho)):
                    r0, r1 = hmax(b, 2 * oy, ox), hmax(b, 2 * oy + 1, ox)
                    out[b, oy, ox] = np.maximum(np.maximum(prev, r0), r1)
                    prev = r0 if prev_bug else r1
    return out


@pytest.mark.parametrize("shape", R.POOL_SHAPES + [(2, 19, 3, 8)])
@pytest.mark.parametrize("special", [None, "inf"])
def test_maxpool_walk_equals_the_reference(shape, special):
    x = R.build_pool("real", shape, False, special)
    ref = R.maxpool_ref(x)
    for rpc in (1, 4):
        assert np.array_equal(_maxpool_walk(x, rpc), ref)
    if special == "inf" and shape[1] >= 3:
        assert np.isneginf(ref[0, 0, 0]).all()  # an all -inf window
    assert np.array_equal(R.maxpool_ref(x, prev_bug=True), _maxpool_walk(x, 4, prev_bug=True))


def test_prev_r0_differs_on_the_rpc4_case():
    n, h, w, c = R.POOL_RPC4
    ho, wo, gx, rpc, chunks = R.maxpool_geom(n, h, w, c, 4)
    assert rpc == 4 and ho % 4 != 0 and n * ho * gx == 16400 >= R.MP_GATE
    for bf16 in (False, True):
        x = R.build_pool("real", (4, h, w, c), bf16)
        assert not np.array_equal(R.maxpool_ref(x, prev_bug=True), R.maxpool_ref(x))
    # with one row per chunk the defect is invisible: the older bf16 case (n = 2, 13 × 10) cannot see it
    x = R.build_pool("real", (2, 13, 10, 8), True)
    assert np.array_equal(_maxpool_walk(x, 1, prev_bug=True), R.maxpool_ref(x))


@pytest.mark.parametrize("shape", R.POOL_SHAPES)
@pytest.mark.parametrize("bf16", [False, True])
def test_avgpool_model_and_divisor_4(shape, bf16):
    for fam in ("ints", "real"):
        x = R.build_pool(fam, shape, bf16)
        ref = R.avgpool_model(x, bf16)
        n, h, w, c = shape
        if fam == "ints":  # exact: equals the fp64 mean
            ho, wo = (h + 1) // 2, (w + 1) // 2
            xp = np.zeros((n, 2 * ho, 2 * wo, c))
            cnt = np.zeros((2 * ho, 2 * wo))
            xp[:, :h, :w], cnt[:h, :w] = x, 1
            s = sum(xp[:, dy::2, dx::2] for dy in range(2) for dx in range(2))
            k = sum(cnt[dy::2, dx::2] for dy in range(2) for dx in range(2))
            mean = s / k[None, :, :, None]
            want = cr.bf16_round(mean.astype(F32)) if bf16 else mean.astype(F32)
            assert np.array_equal(ref, want)
        wrong = R.avgpool_model(x, bf16, div4=True)
        if h % 2 or w % 2:
            assert (~R.same_bits(wrong, ref)).any(), "divisor 4 at a ragged edge goes unnoticed"
        else:
            assert R.same_bits(wrong, ref).all()


def test_avgpool_overflow():
    x = R.build_pool("real", (2, 4, 5, 8), False, "big")
    assert np.isinf(R.avgpool_model(x)).any() and not np.isnan(R.avgpool_model(x)).any()


# ---------------------------------------------------------------------------------------------- case lists
def test_stem_shapes_reach_what_they_claim():
    px = [n * np.prod(R.stem_out(h, w)) for n, h, w in R.STEM_SHAPES]
    assert px[4] == R.STEM_BLOCK and px[5] == 432 and px[6] == 544
    n, h, w = R.STEM_SHAPES[5]
    per = np.prod(R.stem_out(h, w))
    assert per < R.STEM_BLOCK < 2 * per  # the second workgroup starts inside image 1 and ends in image 2
    assert {(h % 2, w % 2) for _, h, w in R.STEM_SHAPES[:4]} >= {(1, 1), (0, 0)}


@pytest.mark.parametrize("kind,cout", SMALL)
def test_conv_case_lists(kind, cout):
    q = R.KINDS[kind]
    th, tw = q["th"], q["tw"]
    g = R.geometry(kind)
    assert [R.tiles(kind, *s) for s in g] == [2, 4, 2, 4, 18]
    cap = R.grid_cap(kind, cout, CUS)
    w1, w2 = R.walk(kind, cout, CUS)
    assert R.tiles(kind, *w1) == cap + 3 and R.tiles(kind, *w2) == 2 * cap + 1
    for n, h, w in (w1, w2):
        assert w == 2 and h % th == 1 and R.tiles(kind, n, h, w) > cap and n * h * w * q["cin"] < 2 ** 22
    if q["ld"]:
        assert all(ldx >= 64 and ldy >= 64 and ldx % 8 == 0 and ldy % 8 == 0 for ldx, ldy in R.SLICES)


def test_launcher_constants_match_the_sources():
    """The tile sizes, caps and gates above are read from the launchers: hold them to the source text."""
    src = lambda f: open(os.path.join(cr.ROOT, "spotter_amd", "csrc", f)).read()
    stem, x3, el, pre = src("stem.hip"), src("direct_x3.hip"), src("elementwise.hip"), src("preprocess.hip")
    shared = src("direct3x3.h")
    assert "constexpr int C3_TW = 64;" in stem and "constexpr int C3_TH = 4;" in stem
    assert "constexpr int F3_TH = 8," in stem and "constexpr int B6_TH = 16, B6_TW = 32," in stem
    assert "g_num_cus * (cout == 32 ? 3 : 2)" in stem and "constexpr int STEM_BLOCK = 256;" in stem
    assert "direct_grid<C3_TH, C3_TW>(n, h, w, cap)" in stem and "direct_grid<F3_TH, C3_TW>(n, h, w, g_num_cus)" in stem
    assert "direct_grid<B6_TH, B6_TW>(n, h, w, g_num_cus)" in stem
    assert "constexpr int DX_TH = 8, DX_TW = 32," in x3 and "direct_grid<DX_TH, DX_TW>(n, h, w, g_num_cus)" in x3
    assert "tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;" in shared and "tiles < cap ? tiles : cap" in shared
    assert "constexpr int MP_ROWS = 4;" in el and ">= 16384 ? MP_ROWS : 1" in el and "if (g > 256 * 16) g = 256 * 16;" in el
    assert "constexpr int kMaxImgs = 32;" in pre and "constexpr int kLdsBytes = 48 * 1024;" in pre
    assert "constexpr int kColTile = 256;" in pre


def test_pool_and_copy_case_lists():
    for vec in (4, 8):
        ho, wo, gx, rpc, chunks = R.maxpool_geom(*R.POOL_RPC4, vec)
        assert (ho, rpc) == (10, 4) and ho % rpc
        ho, wo, gx, rpc, chunks = R.maxpool_geom(*R.POOL_CHUNKS, vec)
        assert rpc == 4 and chunks > R.GRID_Y
    n, h, w, c = R.POOL_ROWS
    assert n * ((h + 1) // 2) > R.GRID_Y
    (n, h, w, c), (n2, h2, w2, c2) = R.UPSAMPLE_CASES
    assert w * c // 4 == 264 and n2 * h2 == 65600 > R.GRID_Y
    assert np.prod(R.NCHW_CASES[-1]) > R.NCHW_GRID_CAP and {c for _, c, _, _ in R.NCHW_CASES} >= {1, 3, 4}


def test_preprocess_lds_cases():
    cap = R.K_LDS_BYTES // (R.K_COL_TILE * 3)
    assert cap == 64
    assert cap - 4 <= R.band_rows_needed(120, 4) <= cap < R.band_rows_needed(200, 4)
