"""tests/encoder_refs.py without a GPU: the fp64 references against torch float64, the preconditions the seeded
input families promise, and the error bounds as valid bars: a float32 numpy emulation of each kernel's documented
algorithm must stay inside them on every family, and the bf16 bias statistic must separate round-to-nearest from
truncation on both sides of its bar."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_refs as refs  # noqa: E402

torch = pytest.importorskip("torch")

F32 = np.float32
ATTN_SHAPES = ((2, 2, 129, 32), (1, 2, 129, 48), (1, 2, 129, 64), (1, 8, 300, 32))  # B, H, n, dh


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


# ----------------------------------------------------------------------------- bf16 helpers
def test_bf16_rounding_matches_torch():
    rng = np.random.default_rng(refs.seed("bf16"))
    a = np.concatenate([rng.standard_normal(4096) * 10.0 ** rng.integers(-30, 30, 4096),
                        [0.0, -0.0, np.inf, -np.inf, 3.4e38, -3.4e38, refs.BF16_MAX, 1.0 + 2.0 ** -8,
                         1.0 + 3 * 2.0 ** -8]]).astype(F32)
    want = torch.from_numpy(a).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(refs.bf16_bits(a), want)
    assert np.array_equal(refs.bf16_round(a), refs.bf16_float(want))
    assert np.isnan(refs.bf16_float(refs.bf16_bits(np.array([np.nan], F32)))).all()
    assert np.isinf(refs.bf16_round(np.array([3.4e38], F32))).all()
    tr = refs.bf16_trunc(a)
    assert np.all(np.abs(tr) <= np.abs(a)) and np.all((tr.view(np.uint32) & 0xFFFF) == 0)


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize("family", refs.ATTN_FAMILIES)
def test_attention_reference_matches_torch_float64(family):
    for B, H, n, dh in ATTN_SHAPES[:1] + ATTN_SHAPES[3:]:
        inp = refs.attn_inputs(family, B, H, n, dh)
        o, s, a = refs.attention(inp.q, inp.k, inp.v, inp.scale)
        want = torch.nn.functional.scaled_dot_product_attention(t64(inp.q), t64(inp.k), t64(inp.v),
                                                                scale=inp.scale).numpy()
        assert np.abs(o - want).max() <= 1e-12 * np.abs(want).max()
        assert np.allclose(a.sum(-1), 1.0, rtol=0, atol=1e-13)
        assert s.shape == a.shape == (B, H, n, n)


def _block_max(s):
    """Running maximum after each 16-key block, [.., n, blocks]."""
    n = s.shape[-1]
    bm = np.stack([s[..., j0:j0 + 16].max(-1) for j0 in range(0, n, 16)], -1)
    return np.maximum.accumulate(bm, -1), bm


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_attention_families_keep_their_promises(bf16):
    """What each family is for holds on the operands the kernel actually multiplies (bf16-rounded for the bf16
    kernel): sharp scores in the hundreds, a maximum that rises in every block / sits in the first, a one-hot winner
    ONEHOT_GAP clear of the rest in first and last block, uniform weights, big mixed-sign V."""
    rnd = refs.bf16_round if bf16 else (lambda a: a)
    for B, H, n, dh in ATTN_SHAPES:
        def scores(family):
            inp = refs.attn_inputs(family, B, H, n, dh)
            return inp, refs.attention(rnd(inp.q), rnd(inp.k), rnd(inp.v), inp.scale)

        _, (_, s, _) = scores("normal")
        assert np.abs(s).max() < 10
        _, (_, s8, _) = scores("sharp8")
        assert np.abs(s8).max() > 200
        _, (_, s, _) = scores("ascending")
        run, bm = _block_max(s)
        step = np.diff(bm, axis=-1)
        full = step if n % 16 == 0 else step[..., :-1]  # a one-key tail block rises by one key's step only
        assert np.all(full > 0.5), "the block maximum must rise in every full block, for every query"
        assert (step[..., -1] > 0).mean() > 0.5
        _, (_, s, _) = scores("descending")
        run, bm = _block_max(s)
        assert np.all(np.diff(bm, axis=-1) < -0.5) and np.all(run == run[..., :1])
        _, (_, s, a) = scores("uniform")
        assert np.all(s == 0) and np.allclose(a, 1.0 / n, rtol=1e-15)
        _, (_, s, a) = scores("onehot")
        top2 = np.sort(s, -1)[..., -2:]
        assert np.all(top2[..., 1] - top2[..., 0] >= refs.ONEHOT_GAP) and top2[..., 1].min() > 1000
        win = s.argmax(-1)
        assert (win < 16).any() and (win >= n - n % 16 - (16 if n % 16 == 0 else 0)).any()
        assert np.all(np.exp2((top2[..., 0] - top2[..., 1]) * refs.LOG2E).astype(F32) == 0)  # underflows in fp32
        inp, _ = scores("bigv")
        assert np.abs(inp.v).min() >= 4e3 and (inp.v > 0).any() and (inp.v < 0).any()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("family", refs.ATTN_FAMILIES)
def test_attention_bound_holds_for_the_float32_emulation(family, bf16):
    """The documented algorithm in float32 numpy stays inside attention_bound on every family and head size (the
    printed fraction is how much of the bar it uses: a few percent)."""
    worst = 0.0
    for B, H, n, dh in ATTN_SHAPES:
        case = refs.attn_case(family, B, H, n, dh, bf16)
        got = refs.emulate_attention(*case.inp[:3], case.inp.scale, bf16=bf16)
        assert np.isfinite(got).all()
        assert np.all(case.tol > 0)
        frac = float((np.abs(got - case.ref) / case.tol).max())
        worst = max(worst, frac)
        assert frac <= 1.0, (family, bf16, (B, H, n, dh), frac)
    print(f"attention emulation {family} {'bf16' if bf16 else 'f32'}: worst err/tol {worst:.3f}")
    if not bf16:  # (a bf16 P on one dominant key may use its whole half ulp)
        assert worst <= 0.5, "the bound is meant to leave a correct fp32 implementation ample room"


def test_attention_bound_rejects_a_dropped_rescale():
    """The bar is tight enough to matter: the same emulation with corr replaced by 1 in the accumulator fails it on
    the ascending family."""
    B, H, n, dh = ATTN_SHAPES[0]
    case = refs.attn_case("ascending", B, H, n, dh, False)
    q, k, v = (np.asarray(t, F32) for t in case.inp[:3])
    sc = F32(F32(case.inp.scale) * F32(refs.LOG2E))
    m = np.full((B, H, n), -np.inf, F32)
    l = np.zeros((B, H, n), F32)
    acc = np.zeros((B, H, n, dh), F32)
    for j0 in range(0, n, 16):
        st = (np.einsum("bhic,bhjc->bhij", q, k[:, :, j0:j0 + 16], dtype=F32) * sc).astype(F32)
        mn = np.maximum(m, st.max(-1))
        corr = np.where(np.isneginf(m), F32(0), np.exp2(m - mn)).astype(F32)
        m = mn
        pr = np.exp2(st - mn[..., None]).astype(F32)
        l = l * corr + pr.sum(-1, dtype=F32)
        acc = acc + np.einsum("bhij,bhjc->bhic", pr, v[:, :, j0:j0 + 16], dtype=F32)  # no rescale
    got = acc / l[..., None]
    assert (np.abs(got - case.ref) / case.tol).max() > 10


@pytest.mark.parametrize("n,H,dh", refs.BIAS_SHAPES)
def test_bf16_bias_statistic_separates_rne_from_truncation(n, H, dh):
    """mean((got − ref)/ref) on positive V: with P rounded to nearest it stays far below BIAS_BAR = 2⁻¹² (and no
    single output is off by more than 2⁻⁹), with P truncated it is about −2⁻⁹, ten times past the bar."""
    inp = refs.bias_inputs(n, H, dh)
    ref, _, _ = refs.attention(refs.bf16_round(inp.q), refs.bf16_round(inp.k), refs.bf16_round(inp.v), inp.scale)
    assert ref.min() >= 0.5
    rne, rne_max = refs.bias_statistic(refs.emulate_attention(*inp[:3], inp.scale, bf16=True), ref)
    trunc, _ = refs.bias_statistic(
        refs.emulate_attention(*inp[:3], inp.scale, bf16=True, p_round=refs.bf16_trunc), ref)
    print(f"bias ({n}, {dh}): RNE mean {rne:+.2e} max {rne_max:.2e}; truncation mean {trunc:+.2e}")
    assert abs(rne) <= refs.BIAS_BAR / 8 and rne_max < 2.0 ** -9
    assert trunc <= -4 * refs.BIAS_BAR


# ----------------------------------------------------------------------------- layernorm
@pytest.mark.parametrize("family", refs.LN_FAMILIES)
def test_layernorm_reference_matches_torch_float64(family):
    for d, rows in ((1, 3), (3, 5), (257, 17), (1024, 5)):
        c = refs.ln_case(family, rows, d)
        want = torch.nn.functional.layer_norm(t64(c.x), (d,), t64(c.g), t64(c.b), refs.LN_EPS).numpy()
        assert np.abs(c.ref - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)


def test_layernorm_families_keep_their_promises():
    for d in (4, 257, 1024):
        x = refs.ln_rows("tiny", 17, d).astype(np.float64)
        assert x.var(-1).max() < refs.LN_EPS / 100
        x = refs.ln_rows("offset4", 17, d).astype(np.float64)
        assert np.all(np.abs(x.mean(-1)) > 2e3 * x.std(-1))
        x = refs.ln_rows("const", 17, d)
        assert np.all(x == F32(refs.LN_CONST))
        x = refs.ln_rows("outlier", 17, d)
        assert np.all((x == F32(1e6)).sum(-1) == 1)
    g, b = refs.ln_params(1024)
    assert np.all(b != 0)
    # the const rows' sums are exact in fp32 in any order: d·7.25 has at most 15 significant bits
    assert float(F32(refs.LN_CONST) * F32(1024)) == refs.LN_CONST * 1024
    assert refs.LN_C >= 22  # the longest chain, counted in layernorm_bound's docstring


@pytest.mark.parametrize("family", refs.LN_FAMILIES)
def test_layernorm_bound_holds_for_the_float32_emulation(family):
    worst = 0.0
    for d, rows in refs.LN_SHAPES:
        if rows > 17:
            continue
        c = refs.ln_case(family, rows, d)
        got = refs.emulate_layernorm(c.x, c.g, c.b)
        assert np.isfinite(got).all() and np.all(c.tol > 0)
        frac = float((np.abs(got - c.ref) / c.tol).max())
        worst = max(worst, frac)
        assert frac <= 1.0, (family, d, rows, frac)
        if family == "const":
            assert np.array_equal(got.view(np.uint32), np.broadcast_to(c.b, got.shape).view(np.uint32))
    print(f"layernorm emulation {family}: worst err/tol {worst:.3f}")
    assert worst <= 0.5


def test_layernorm_bound_rejects_a_wrong_divisor():
    """1/255 in place of 1/256 (mean and variance) is far outside the bar on plain rows."""
    c = refs.ln_case("plain", 17, 256)
    x = c.x.astype(np.float64)
    mu = x.sum(-1, keepdims=True) / 255
    var = ((x - mu) ** 2).sum(-1, keepdims=True) / 255
    bad = (x - mu) / np.sqrt(var + refs.LN_EPS) * c.g + c.b
    assert (np.abs(bad - c.ref) / c.tol).max() > 100


def test_ln_shapes_cover_the_issue_list():
    assert {d for d, r in refs.LN_SHAPES if r == 17} == set(refs.LN_DS)
    for d in (256, 260, 257):
        assert {r for dd, r in refs.LN_SHAPES if dd == d} == set(refs.LN_ROWS)


# ----------------------------------------------------------------------------- add_rows
def test_add_rows_special_inputs():
    a, b, ns = refs.add_rows_special()
    with np.errstate(invalid="ignore", over="ignore"):
        s = a + b
    bits = refs.bf16_bits(s)
    r = refs.bf16_float(bits)
    assert np.isnan(s[:, :ns]).any() and np.isinf(s[:, :ns]).any()
    over = np.isfinite(s) & (np.abs(s) > refs.BF16_MAX)
    assert over[0].sum() >= 3 and np.all(np.isinf(r[over])) and np.all(np.sign(r[over]) == np.sign(s[over]))
    negz = (s == 0) & np.signbit(s)
    assert negz.any() and np.all(bits[negz] == 0x8000)
    assert np.all(np.isnan(r) == np.isnan(s))
