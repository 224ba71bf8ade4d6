"""Host checks of tests/wino_refs.py: the fp64 stage references against the direct conv, float32 emulations of every
stage (two accumulation orders each) against every bound and every exact family, defective emulations against the
matrix (a defect every case tolerates is a hole), and sp_winograd_plan on fake descriptors: the tile rule's
boundaries, the refusals, and the ledger of component-GEMM instances. No GPU.

-s prints the looseness of each bound (worst correct-emulation err / bound per stage) and the number of cases
each defect fails."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as R  # noqa: E402
import wino_refs as W  # noqa: E402

f32 = np.float32
ROOT = R.ROOT


# ------------------------------------------------------------------------------------------------ emulations
def _fma(a, b, c, contract):
    """fp32 a·b + c with one rounding (contract) or two."""
    if contract:
        return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    return ((f32(a) * b).astype(f32) + c).astype(f32)


def _chain(row, vals, contract, reverse):
    idx = [j for j in range(len(row)) if row[j] != 0]
    acc = np.zeros_like(vals[idx[0]])
    for j in (idx[::-1] if reverse else idx):
        acc = _fma(row[j], vals[j], acc, contract)
    return acc


def emu_input(x, wm, contract=True, reverse=False, bt=None, pair_bug=False):
    bt = W.BT[wm] if bt is None else bt
    d = W.patches(x.astype(f32), wm)
    P = wm + 2
    if pair_bug:  # the second tile of a horizontal pair transforms the first tile's columns
        tw = (x.shape[2] + wm - 1) // wm
        odd = (np.arange(d.shape[0]) % tw) % 2 == 1
        d = d.copy()
        d[odd] = d[np.nonzero(odd)[0] - 1]
    q = [[_chain(bt[b], [d[:, i, j] for j in range(P)], contract, reverse) for b in range(P)] for i in range(P)]
    v = [_chain(bt[a], [q[i][b] for i in range(P)], contract, reverse) for a in range(P) for b in range(P)]
    return np.stack(v)


def _act32(y, act):
    if act == "relu":
        return np.maximum(y, f32(0))
    if act == "silu":
        with np.errstate(over="ignore"):
            return (y / (f32(1) + np.exp(-y).astype(f32))).astype(f32)
    if act == "gelu":
        return R.act64(y.astype(np.float64), "gelu").astype(f32)
    return y


def emu_output(m, n, h, w, wm, e, contract=True, reverse=False, transposed=False, res2_first=False):
    P = wm + 2
    m4 = m.astype(f32).reshape(P, P, m.shape[1], m.shape[2])
    if transposed:
        m4 = m4.transpose(1, 0, 2, 3)
    at = W.AT[wm]
    s = [[_chain(at[p], [m4[a, b] for a in range(P)], contract, reverse) for b in range(P)] for p in range(wm)]
    y = np.stack([np.stack([_chain(at[q], s[p], contract, reverse) for q in range(wm)], axis=1) for p in range(wm)],
                 axis=1)  # [T, wm, wm, c]
    y = W.untile(y, n, h, w, wm)
    sc = e["scale"] if e["scale"] is not None else np.ones(y.shape[1], f32)
    sh = e["shift"] if e["shift"] is not None else np.zeros(y.shape[1], f32)
    y = (y.astype(np.float64) * sc[None, :] + sh[None, :]).astype(f32)
    if e["r1"] is not None:
        y = y + e["r1"]
    if res2_first and e["r2"] is not None:
        return _act32(y + e["r2"], e["act"])
    y = _act32(y, e["act"])
    if e["r2"] is not None:
        y = y + e["r2"]
    return y


def emu_gemm(v, u, mode, reverse=False, no_midmid=False, trunc_a=False, bi_shift=False):
    """fp32 accumulation of the kept bf16 × bf16 products (each exact in fp32) in k-blocks of 16 (forward) or 4
    (reverse: the blocks and the kept products in the opposite order)."""
    if bi_shift:
        u = np.roll(u, -1, axis=0)
    if mode == "bf16":
        pa, pw, kept = [(R.bf16_trunc if trunc_a else R.bf16_round)(v)], [u], [(0, 0)]
    else:
        pa, pw, kept = R.planes_of(v, mode), R.planes_of(u, mode), list(R.KEPT[mode])
        if trunc_a:  # the A split cut short: its last plane missing
            pa[-1] = np.zeros_like(pa[-1])
        if no_midmid:
            kept.remove((1, 1))
    kb = 4 if reverse else 16
    blocks = list(range(0, v.shape[2], kb))
    if reverse:
        blocks, kept = blocks[::-1], kept[::-1]
    acc = np.zeros((v.shape[0], v.shape[1], u.shape[1]), f32)
    for k0 in blocks:
        for ia, iw in kept:
            part = np.matmul(pa[ia][:, :, k0:k0 + kb].astype(np.float64),
                             pw[iw][:, :, k0:k0 + kb].astype(np.float64).transpose(0, 2, 1))
            acc = (acc + part.astype(f32)).astype(f32)
    return acc


def emu_path(c, r, alt=False, **defect):
    n, h, w, cin, cout = c["shape"]
    wm = c["wm"]
    din = {k: defect[k] for k in ("bt", "pair_bug") if k in defect}
    dg = {k: defect[k] for k in ("no_midmid", "trunc_a", "bi_shift") if k in defect}
    do = {k: defect[k] for k in ("transposed", "res2_first") if k in defect}
    v = emu_input(r["x"], wm, contract=not alt, reverse=alt, **din)
    m = emu_gemm(v, r["u"], c["mode"], reverse=alt, **dg)
    return emu_output(m, n, h, w, wm, r, contract=not alt, reverse=alt, **do)


def emulate(c, r, alt=False, **defect):
    n, h, w, cin, cout = c["shape"]
    wm = c["wm"]
    if c["stage"] == "in":
        return emu_input(r["x"], wm, contract=not alt, reverse=alt, **defect)
    if c["stage"] == "out":
        return emu_output(r["m"], n, h, w, wm, r, contract=not alt, reverse=alt, **defect)
    if c["stage"] == "gemm":
        return emu_gemm(r["v"], r["u"], c["mode"], reverse=alt, **defect)
    return emu_path(c, r, alt, **defect)


_built = {}


def built(c):
    """One reference per case, shared by every test of this file and left unchanged."""
    if c["id"] not in _built:
        _built[c["id"]] = W.build(c)
    return _built[c["id"]]


def _small(c):
    """The cases the host emulations run: everything but the large GEMM / VW-switch shapes."""
    n, h, w, cin, cout = c["shape"]
    L = W.layout(c)
    return (L["NC"] * L["T"] * max(cin, cout) <= 36 * 257 * 160 and L["NC"] * L["T"] * cin * cout <= 1 << 26
            and not c["in_vw"])


# ------------------------------------------------------------------------------------------------ references
def test_matrices_agree_with_the_library_binding():
    """Bᵀ, Aᵀ and G here are ops.WINO_*, and Bᵀ / Aᵀ of F(4×4) are the kernel's kBT43 / kAT43."""
    import re

    from spotter_amd import ops

    for wm in (2, 4):
        assert np.array_equal(W.BT[wm], ops.WINO_BT[wm]) and np.array_equal(W.AT[wm], ops.WINO_AT[wm])
        assert np.allclose(W.G[wm], ops.WINO_G[wm], rtol=0, atol=1e-16)
    src = open(os.path.join(ROOT, "spotter_amd", "csrc", "winograd.hip")).read()
    for name, mat in (("kBT43", W.BT[4]), ("kAT43", W.AT[4])):
        body = re.search(name + r"\[\d\]\[\d\] = \{(.*?)\};", src, re.S).group(1)
        vals = [float(v.rstrip("f")) for v in re.findall(r"-?\d+\.?\d*f", body)]
        assert np.array_equal(np.array(vals).reshape(mat.shape), mat), name


@pytest.mark.parametrize("wm", [2, 4])
def test_stage_references_compose_to_the_direct_conv(wm):
    """Bᵀ d B → · G g Gᵀ → Aᵀ M A in fp64 equals the direct fp64 cross-correlation on every whole-path shape: to
    1e-12 of the output scale on N(0,1) data, exactly on the impulse family (asserted by build) and on integers
    with the family's tap values."""
    rng = np.random.default_rng(wm)
    for (n, h, w, cin, cout) in W.PATH_SHAPES + tuple((1, hh, ww, 32, 4) for hh, ww in W.HW):
        x = rng.standard_normal((n, h, w, cin))
        wk = rng.standard_normal((cout, 3, 3, cin))
        got = W.output_ref(W.gemm_ref(W.input_ref(x, wm), W.weights_ref(wk, wm)), n, h, w, wm)
        ref = W.direct_ref(x, wk)
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (wm, n, h, w)
        xi = rng.integers(-8, 9, (n, h, w, cin)).astype(np.float64)
        wi = rng.integers(-1, 2, (cout, 3, 3, cin)) * W.TAP[wm]
        ui = W.weights_ref(wi, wm)  # an integer by construction (fp64 thirds / fifteenths are not exact: rounded)
        assert np.abs(ui - np.rint(ui)).max() < 1e-9
        got = W.output_ref(W.gemm_ref(W.input_ref(xi, wm), np.rint(ui)), n, h, w, wm)
        assert np.array_equal(got, W.direct_ref(xi, wi)), (wm, n, h, w)
    for c in W.cases("path"):
        if c["wm"] == wm and c["fam"] == "impulse":
            built(c)  # asserts U exact, V / U bf16-exact, |path| < 2^16 on the 2^-8 grid, composition == direct


def test_matrix_reaches_what_the_issue_lists():
    ins, outs, gem, path = (W.cases(s) for s in ("in", "out", "gemm", "path"))
    for wm in (2, 4):
        for fam in ("ints", "range"):
            got = {(c["shape"][1:3], c["shape"][0], c["shape"][3], c["gap"]) for c in ins
                   if c["wm"] == wm and c["fam"] == fam and not c["in_vw"]}
            assert got == {(hw, n, ci, g) for hw in W.HW for n in (1, 3) for ci in (32, 96) for g in (False, True)}
            got = {(c["shape"][1:3], c["shape"][0], c["shape"][4], c["gap"]) for c in outs
                   if c["wm"] == wm and c["fam"] == fam}
            assert got == {(hw, n, co, g) for hw in W.HW for n in (1, 3) for co in (4, 8, 132) for g in (False, True)}
            assert {c["epi"] for c in outs if c["wm"] == wm and c["fam"] == fam} == set(W.EPIS)
        assert {c["map"] for c in ins if c["wm"] == wm and c["fam"] == "range"} == {"normal", "offset", "relu"}
    for mode in W.MODES:
        g = [c for c in gem if c["mode"] == mode]
        assert {c["shape"][2] // c["wm"] for c in g} >= {1, 63, 65, 130, 257}
        assert {c["shape"][3] for c in g} >= {32, 64, 160} and {c["shape"][4] for c in g} >= {4, 48, 128, 136, 256, 384}
        assert {c["cfg"] for c in g} >= set(W.WINO_CFGS) and {c["wm"] for c in g} == {2, 4}
        assert {c["tile"] for c in g if c["tile"]} == {14, 63, 246, 245}
        for wm in (2, 4):
            p = [c for c in path if c["mode"] == mode and c["wm"] == wm]
            assert {(c["shape"], c["fam"]) for c in p} == {(s, f) for s in W.PATH_SHAPES for f in ("impulse", "range")}
    # the impulse family puts an impulse on every patch position and uses all nine taps
    for wm in (2, 4):
        seen = np.zeros((wm + 2, wm + 2), bool)
        for c in path:
            if c["wm"] == wm and c["fam"] == "impulse" and c["mode"] == "x3":
                r = built(c)
                seen |= (W.patches(r["x"], wm) != 0).any(axis=(0, 3))
                if min(c["shape"][3:]) >= 9:
                    assert (r["wk"].reshape(c["shape"][4], 9, -1) != 0).any(axis=(0, 2)).all()
        assert seen.all(), (wm, seen)


# ------------------------------------------------------------------------------------------------ emulations
LOOSENESS = {}


@pytest.mark.parametrize("stage", ["in", "out", "gemm", "path"])
def test_correct_emulations_stay_in_bounds(stage):
    """Two float32 emulations of the stage (fused multiply-adds in the kernels' order; separate multiply and add in
    the reverse order; the GEMM in k-blocks of 16 forward and of 4 backward) reproduce every exact family bit for
    bit and stay inside every range bound. The worst err / bound states how loose each bound is."""
    worst, fails = {}, []
    for c in W.cases(stage):
        if not _small(c):
            continue
        r = built(c)
        for alt in (False, True):
            bad, w, msg = W.compare(c, r, emulate(c, r, alt))
            if c["fam"] == "range":
                k = (stage, c["wm"], c["mode"] if stage in ("gemm", "path") else "-")
                worst[k] = max(worst.get(k, 0.0), w)
            if bad:
                fails.append((alt, msg))
    LOOSENESS.update(worst)
    print("\n" + "\n".join(f"looseness {k}: worst correct-emulation err / bound {v:.4f}" for k, v in sorted(worst.items())))
    assert not fails, (len(fails), fails[:5])
    assert worst and all(v > 1e-3 for v in worst.values()), worst  # a bound a thousand times too wide sees nothing


DEFECTS = {
    # name: (stage, emulation flags, predicate on the cases that could notice)
    "BT coefficient -2.5 -> -2": ("in", dict(bt="bt"), lambda c: c["wm"] == 4),
    "F(2x2) pair reads first tile's columns": ("in", dict(pair_bug=True), lambda c: c["wm"] == 2),
    "output component order transposed": ("out", dict(transposed=True), lambda c: True),
    "res2 before the activation": ("out", dict(res2_first=True), lambda c: True),
    "x3 without mid*mid": ("gemm", dict(no_midmid=True), lambda c: c["mode"] == "x3"),
    "truncated A split": ("gemm", dict(trunc_a=True), lambda c: True),
    "batch member reads U of bi + 1": ("gemm", dict(bi_shift=True), lambda c: True),
}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_defective_emulations_fail_named_cases(name):
    """Each defect, applied to the stage's emulation and to the whole path's, fails cases of both matrices."""
    stage, flags, pred = DEFECTS[name]
    if "bt" in flags:
        bt = W.BT[4].copy()
        assert bt[1, 2] == -2.5
        bt[1, 2] = -2.0
        flags = dict(bt=bt)
    for st in (stage, "path"):
        failed, exact_failed, tried = [], 0, 0
        for c in W.cases(st):
            if not (_small(c) and pred(c)):
                continue
            tried += 1
            r = built(c)
            bad, w, msg = W.compare(c, r, emulate(c, r, False, **flags))
            if bad:
                failed.append(c["id"])
                exact_failed += c["fam"] != "range"
        print(f"\ndefect '{name}' on {st}: fails {len(failed)} of {tried} cases ({exact_failed} exact), e.g. {failed[:2]}")
        if st == stage:
            assert failed and exact_failed, (name, st)
        elif name in ("x3 without mid*mid", "truncated A split"):
            # the whole-path bound is two orders above the real error (Y_abs >> |out|): it cannot see a dropped
            # low-order product, which is why the GEMM stage is tested on exact operands of its own
            continue
        else:
            assert failed, (name, st)


# ------------------------------------------------------------------------------------------------ the plan
def _desc(wm, T, cin, cout, mode, **kw):
    c = W._case("gemm", "ints", wm, mode, W._gemm_shape(T, cin, cout, wm))
    d = W.fake_desc(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _tile(wm, T, cout, mode="x3", cfg=None):
    with W.forced(cfg):
        key, nc, tiles, _, _ = W.plan_of(_desc(wm, T, 32, cout, mode), wm)
    assert nc == (wm + 2) ** 2 and tiles == T
    return key[1] + (200 if key[6] == 4 else 0)


def test_plan_rule_boundaries():
    """The component GEMM's tile rule at ±1 around every threshold (rows = NC·T), and the input transform's VW
    switch at 2^18 items, through sp_winograd_plan on fake descriptors."""
    for wm, nc in ((2, 16), (4, 36)):
        up = lambda rows: -(-rows // nc)  # noqa: E731  (the smallest T with NC·T >= rows)
        t12, t20, t400 = up(12000), up(20000), up(400000)
        for mode in ("x3", "x2"):
            assert _tile(wm, t12 - 1, 128, mode) == 14 and _tile(wm, t12 - 1, 256, mode) == 14
            assert _tile(wm, t12, 128, mode) == 14 and _tile(wm, t12, 256, mode) == 63
            assert _tile(wm, t12, 384, mode) == 63 and _tile(wm, t12, 252, mode) == 14
            assert _tile(wm, t20 - 1, 256, mode) == 63 and _tile(wm, t20 - 1, 128, mode) == 14
            assert _tile(wm, t20, 128, mode) == 246 and _tile(wm, t20, 256, mode) == 246
            assert _tile(wm, t20, 260, mode) == 14 and _tile(wm, t20, 384, mode) == 245
            assert _tile(wm, t400 - 1, 384, mode) == 245 and _tile(wm, t400, 384, mode) == 247
            assert _tile(wm, t400, 256, mode) == 246 and _tile(wm, t400, 512, mode) == 247
        assert _tile(wm, t20, 128, "bf16") == 46  # one plane: the direct-store form is a split-operand instance
    # every matrix case plans to the tuple it was built for (and names its rule tile where it carries one)
    for c in W.cases("gemm"):
        with W.forced(c["cfg"]):
            key, nc, tiles, _, _ = W.plan_of(W.fake_desc(c), c["wm"])
        assert key == W.expected_plan(c) and (c["tile"] is None or key[1] == c["tile"] % 100), (c["id"], key)
    # tile 247 runs under the forced id at a small shape: the forced tuple is the rule's tuple at the large one
    q = W.RULE_247_SHAPE
    for mode in W.MODES:
        with W.forced(None):
            big = W.plan_of(_desc(q["wm"], q["T"], q["cin"], q["cout"], mode), q["wm"])[0]
        small = [W.expected_plan(c) for c in W.cases("gemm") if c["cfg"] == 247 and c["mode"] == mode]
        assert small and all(s == big for s in small), (mode, big, small)
    # in_vw: 1 below 2^18 tile × channel items, 2 from there; F(2×2) is float4 throughout; out_vw is 1
    for c in W.cases("in"):
        if c["in_vw"]:
            assert W.plan_of(W.fake_desc(c), 4)[3:] == (c["in_vw"], 1), c["id"]
    assert W.plan_of(_desc(4, 8191, 32, 4, "x3"), 4)[3] == 1 and W.plan_of(_desc(4, 8192, 32, 4, "x3"), 4)[3] == 2
    assert W.plan_of(_desc(2, 8192, 32, 4, "x3"), 2)[3:] == (4, 4)


def production_launches():
    with open(os.path.join(ROOT, "tests", "golden", "wino_launches.json")) as f:
        return [tuple(x) for x in json.load(f)["launches"]]


def test_ledger_every_component_gemm_instance_has_a_case():
    """Every (tile, planes, epilogue variant, fast_1x1) the rule or a forced WINO_CFGS id can produce, and every
    tuple the engine's recorded Winograd launches plan to (production), is reached by a GEMM case of the matrix."""
    have = {W.expected_plan(c) for c in W.cases("gemm")}
    want = {}
    for mode in W.MODES:
        for wm in (2, 4):
            for cfg in W.WINO_CFGS + (W.X2_FALLBACK_CFGS if mode == "x2" else ()):
                for T, cout in ((1, 4), (334, 256), (556, 128), (556, 384), (11112, 384)):
                    with W.forced(cfg):
                        want.setdefault(W.plan_of(_desc(wm, T, 32, cout, mode), wm)[0], False)
    launches = production_launches()
    assert launches
    for wm, n, h, w, cin, cout, mode in launches:
        c = W._case("path", "range", wm, mode, (n, h, w, cin, cout))
        key, nc, tiles, in_vw, out_vw = W.plan_of(W.fake_desc(c), wm)
        want[key] = True
    missing = {k: p for k, p in want.items() if k not in have}
    print(f"\nwinograd ledger: {len(want)} tuples ({sum(want.values())} production), {len(have)} in the matrix")
    assert not missing, missing
    assert all(k[0] == 2 and k[5] == 1 for k in want)  # LDS-DMA, always on the 1×1 fast path


REFUSALS = [
    (dict(lda=31), "lda"), (dict(ldc=3), "ldc"), (dict(res1=R.PTR["res1"], ldr1=0), "ldr1"),
    (dict(res2=R.PTR["res2"], ldr2=0), "ldr2"), (dict(A_bf16=R.PTR["A"]), "bf16 rows"),
    (dict(C_bf16=R.PTR["C"]), "bf16 rows"), (dict(res1_bf16=R.PTR["res1"]), "bf16 rows"),
    (dict(res2_bf16=R.PTR["res2"]), "bf16 rows"), (dict(Ho=5), "3x3 stride-1"), (dict(Cin=48, lda=48), "Cin % 32"),
    (dict(Cout=6, ldc=8), "Cout % 4"), (dict(A=R.PTR["A"] + 4), "16-byte aligned"),
    (dict(A2=R.PTR["A2"]), "A2"), (dict(row_scale=R.PTR["row_scale"], row_period=3), "row_scale"),
    (dict(out_rows_per_group=2), "grouped rows"), (dict(ln_gamma=R.PTR["scale"]), "LayerNorm"),
]


def refusal_desc(kw):
    """A valid 1×4×6, 32 → 4 descriptor with the fields of one refusal changed."""
    c = W._case("path", "range", 4, "x3", (1, 4, 6, 32, 4))
    d = W.fake_desc(c)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("wm", [2, 4])
def test_plan_refusals_name_the_argument(wm):
    from spotter_amd import ops

    assert ops.wino_plan(refusal_desc({}), wm)["tiles"] == (6 if wm == 2 else 2)
    for kw, word in REFUSALS:
        with pytest.raises(RuntimeError, match=word.replace("%", "%")):
            ops.wino_plan(refusal_desc(kw), wm)
    d = refusal_desc({})
    nc, T = (wm + 2) ** 2, (6 if wm == 2 else 2)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.wino_plan(d, wm, work_elems=nc * T * 36 - 1)
    with pytest.raises(RuntimeError, match="wino_plane_stride"):
        ops.wino_plan(d, wm, plane_stride=nc * 4 * 32 - 8)
    with pytest.raises(RuntimeError, match="aligned"):
        ops.wino_plan(d, wm, plane_stride=nc * 4 * 32 + 4)
    d.precision = 1  # one plane: the stride is not read
    assert ops.wino_plan(d, wm, plane_stride=0)["gemm"]["planes"] == 1
    d.precision = 0
    with pytest.raises(RuntimeError, match="precision 0"):
        ops.wino_plan(d, wm)
