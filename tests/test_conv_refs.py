"""tests/conv_refs.py checked on the host, before any GPU sees it: float32 emulations of every operand mode against
the references and the bound, three defective emulations against the probe family, and the coverage ledger (every
instance sp_conv2d can launch has a matrix case that sp_conv_plan maps to exactly that instance). No GPU.
"""
import os
import sys
from math import erf

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as R  # noqa: E402

F32, F64 = np.float32, np.float64
EMU_LIMIT = 8_000_000  # M · Cout · (products per output) of the cases the emulations run


@pytest.fixture(scope="module", autouse=True)
def _lib_built():
    from spotter_amd import _lib

    _lib.load()


# ---------------------------------------------------------------------------------------------- emulations
def _terms(c, r, kept=None, round_a=R.bf16_round):
    """The exact products the mode's MFMAs accumulate, [M, Cout, K·c_mode] fp64 (k major, kept pairs minor).
    kept / round_a: the defective variants (a dropped plane pair, a truncating A rounding)."""
    a, mode = r["acols"], c["mode"]
    if mode == "fp32":
        pa, pw, pairs = [a], [r["w"]], [(0, 0)]
    elif mode == "bf16":
        pa, pw, pairs = [a if c["a_rows"] else round_a(a)], [R.bf16_val(r["w_bits"])], [(0, 0)]
    else:
        pa, pw, pairs = R.planes_of(a, mode), R.planes_of(r["w"], mode), (kept or R.KEPT[mode])
    t = np.stack([pa[i].astype(F64)[:, None, :] * pw[j].astype(F64)[None, :, :] for i, j in pairs], axis=-1)
    return t.reshape(t.shape[0], t.shape[1], -1)


def _fma(acc32, t64):
    return (acc32.astype(F64) + t64).astype(F32)


def _seq(t):
    acc = np.zeros(t.shape[:-1], F32)
    for j in range(t.shape[-1]):
        acc = _fma(acc, t[..., j])
    return acc


def _blocks8(t):
    j = t.shape[-1]
    t = np.concatenate([t, np.zeros(t.shape[:-1] + ((-j) % 8,), F64)], axis=-1).reshape(t.shape[:-1] + (-1, 8))
    part = np.zeros(t.shape[:-1], F32)
    for i in range(8):
        part = _fma(part, t[..., i])
    acc = np.zeros(part.shape[:-1], F32)
    for b in range(part.shape[-1]):
        acc = acc + part[..., b]
    return acc


def _pairwise(t):
    j = t.shape[-1]
    n = 1 << max(1, (j - 1).bit_length())
    t = np.concatenate([t, np.zeros(t.shape[:-1] + (n - j,), F64)], axis=-1)
    x = (t[..., 0::2] + t[..., 1::2]).astype(F32)
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


ORDERS = {"sequential": _seq, "blocks of 8": _blocks8, "pairwise": _pairwise}


def _epilogue32(c, r, acc):
    """The kernels' epilogue in float32: ·row_scale, fma(·, scale, shift), + res1, act, + res2, RNE to bf16 rows."""
    m = acc.shape[0]
    v = acc
    if c["row_period"]:
        v = v * r["row_scale"][np.arange(m) % c["row_period"]][:, None]
    if c["affine"]:
        v = (v.astype(F64) * r["scale"].astype(F64)[None] + r["shift"].astype(F64)[None]).astype(F32)
    if r["r1"] is not None:
        v = v + r["r1"]
    if c["act"] == "relu":
        v = np.maximum(v, F32(0))
    elif c["act"] == "silu":
        with np.errstate(over="ignore"):
            v = v / (F32(1) + np.exp(-v))
    elif c["act"] == "gelu":
        v = F32(0.5) * v * (F32(1) + np.vectorize(erf)((v * F32(0.70710678)).astype(F64)).astype(F32))
    if r["r2"] is not None:
        v = v + r["r2"]
    assert v.dtype == F32
    return v


def _small_cases():
    seen, out = set(), []
    for _want, _prod, cases in R.matrix():
        for c in cases:
            L = R.layout(c)
            # one case per (family, mode, kernel size, stride, flags): the first, which is the smallest shape
            key = (c["fam"], c["mode"], c["shape"][5:7]) + tuple(sorted(
                (k, v) for k, v in c.items() if k not in ("want", "id", "ov", "fam", "mode", "shape")))
            if key in seen or L["M"] * c["shape"][4] * L["K"] * R.C_MODE[c["mode"]] > EMU_LIMIT:
                continue
            seen.add(key)
            out.append(c)
    return out


def _emulate(c, r, order, **defect):
    got = _epilogue32(c, r, ORDERS[order](_terms(c, r, **defect)))
    bits = R.bf16_bits(got) if c["c_bf16"] else None
    return (R.bf16_val(bits) if c["c_bf16"] else got), bits


_SMALL = _small_cases()


@pytest.mark.parametrize("mode", R.MODES)
def test_float32_emulations_meet_the_references(mode):
    """float32 emulations of the mode (the kept products accumulated sequentially, in blocks of 8, and pairwise;
    the fp32 epilogue) equal the probe and ints references bit for bit and stay inside the range bound."""
    cases = [c for c in _SMALL if c["mode"] == mode]
    assert {c["fam"] for c in cases} == set(R.FAMILIES), "no small case of a family for this mode"
    worst, n = {}, 0
    for c in cases:
        r = R.build(c, 2 if c["ws"] else 1)
        for order in ORDERS:
            got, bits = _emulate(c, r, order)
            bad, w, msg = R.compare(c, r, got, bits)
            assert not bad, (order, msg)
            if c["fam"] == "range":
                worst[order] = max(worst.get(order, 0.0), w)
            n += 1
    print(f"{mode}: {len(cases)} cases x 3 orders; worst range err / bound " +
          ", ".join(f"{o} {w:.3f}" for o, w in worst.items()))


DEFECTS = {
    "x3 without mid·mid": ("x3", dict(kept=[p for p in R.KEPT["x3"] if p != (1, 1)])),
    "x3 without hi·lo": ("x3", dict(kept=[p for p in R.KEPT["x3"] if p != (0, 2)])),
    "x2 without hi·lo": ("x2", dict(kept=[p for p in R.KEPT["x2"] if p != (0, 1)])),
    "bf16 A truncated": ("bf16", dict(round_a=R.bf16_trunc)),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_defective_emulations_fail_probe(name):
    """An emulation that drops mid·mid, one that drops a hi·lo, one that truncates A: each differs from the probe
    reference on every probe case of its mode that gives it the chance (a truncating A only where A is rounded)."""
    mode, defect = DEFECTS[name]
    cases = [c for c in _SMALL if c["mode"] == mode and c["fam"] == "probe" and not c["a_rows"]]
    assert len(cases) >= 4
    failed = 0
    for c in cases:
        r = R.build(c, 2 if c["ws"] else 1)
        got, bits = _emulate(c, r, "sequential", **defect)
        failed += bool(R.compare(c, r, got, bits)[0])
    print(f"{name}: fails {failed} of {len(cases)} probe cases")
    assert failed == len(cases), (failed, len(cases))


# ---------------------------------------------------------------------------------------------- the ledger
def test_every_instance_has_a_case_that_plans_to_it():
    """Coverage ledger: every tuple tests/golden/conv_plan.jsonl.gz records under default overrides, the 2-way
    split's image of every 3-way-split one, and every other compiled instance (all SP_GLDS_CONFIGS ids × the
    operand modes they fit × general / 1×1 fast path, the register-staged tiles, the eighteen fp32 ids) has
    cases in the matrix, and sp_conv_plan maps EVERY case's descriptor (fake aligned pointers) to its tuple."""
    rec = R.recorded_targets()
    tg = R.targets()
    assert len(rec) >= 65 and rec <= set(tg)
    g = R.glds_configs()
    assert {52, 53, 54, 55, 56} <= set(g) and all(g[i]["fit1a"] for i in (52, 53, 54, 55, 56))
    for i in (52, 53, 54, 55, 56):
        assert (2, i, 1, 0, 1, 1, 3, 0, 0) in tg and (2, i, 1, 0, 1, 0, 1, 0, 0) in tg
    for t in (14, 45, 46, 47, 63, 64):  # the fp32 path's bottleneck expands: the split mode's slab epilogues
        assert any(k[:3] == (2, t, 3) and k[6] in (2, 4) for k in rec), t
    matched, n_cases = 0, 0
    for want, production, cases in R.matrix():
        assert cases, want
        fams = {c["fam"] for c in cases}
        assert fams == set(R.FAMILIES if production else R.FAMILIES[:2]), (want, fams)
        for c in cases:
            with R.overrides(c["ov"]):
                key, _splits = R.plan_of(R.fake_desc(c))
            assert key == want == c["want"], (c["id"], key, want)
            n_cases += 1
        matched += 1
    assert matched == len(tg)
    print(f"ledger: {matched} target tuples ({len(rec)} recorded, {sum(tg.values())} production), {n_cases} cases, "
          "every one planned to its tuple")


def test_bf16_rounding_ties_of_the_probe_family():
    """The three tie operands round as the issue of the family says (RNE), and truncation moves two of them."""
    t = np.array(R.TIES, np.float32)
    assert np.array_equal(R.bf16_round(t), np.float32([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]))
    assert np.array_equal(R.bf16_trunc(t), np.float32([1.0, 1 + 2.0 ** -7, 1.0]))
    hi, mid, lo = R.planes_of(np.float32([R.V918]), "x3")
    assert (hi[0], mid[0], lo[0]) == (1.0, 2.0 ** -9, 2.0 ** -18)
    hi, lo = R.planes_of(np.float32([R.V918]), "x2")
    assert (hi[0], lo[0]) == (1.0, 2.0 ** -9)
