"""fp64 references, input families and the case matrix of the Winograd path (csrc/winograd.hip), stage by stage.

No GPU and no torch: tests/test_wino_refs.py checks everything here on the host (the references against the direct
fp64 conv, float32 emulations of each stage against every bound, defective emulations against the matrix, the
coverage ledger of the component GEMM), tests/test_gpu_winograd.py launches the same matrix on the MI355X.
DESIGN.md ("Winograd stages against fp64") states the arguments. Built on tests/conv_refs.py: its bf16 helpers,
planes_of, KEPT, C_MODE, act64, U, the guard conventions (GUARD, TAIL) and compare are used as they are.

Workspace layout (include/spotter_hip.h): V [NC][T][Cin] then M [NC][T][Cout], fp32, component-major,
NC = (wm + 2)², component ab = (wm + 2)·a + b, tiles (b, ty, tx) row-major, T = N·⌈H/wm⌉·⌈W/wm⌉.

A case is a plain dict (see `_case`): stage "in" | "out" | "gemm" | "path", family, wm, mode, shape
(n, h, w, cin, cout) (gemm: n = 1, h = 1, w·wm = T·wm, so T tiles) and the flags below.

Families
  ints     in: map values integers in [-8, 8]. Bᵀ holds multiples of 1/2 (F(4×4)) or ±1 (F(2×2)), so V is a
           multiple of 1/4 below 2^9 and every partial sum in any order is exact in fp32.
           out: M values integers in [-R, R]. Aᵀ holds multiples of 1/8, so Y is a multiple of 1/64 and
           |Y| <= 124·R (Σ|Aᵀ| of the last row is 11.125, squared 123.8). R = 1024 without an affine / residual
           (2^17·2^6 < 2^24); with the dyadic epilogue of conv_refs (scale 1, 2, 1/2; shift and residuals
           multiples of 2^-10) R = 32, so that y·scale + shift + res stays a multiple of 2^-10 below 2^14.
           gemm: dense integers in [-4, 4] for V and U.
  probe    gemm only: V sparse from conv_refs' operand sets (at most 56 products per output, one non-zero in every
           16-deep k-step), U dense and different for every component, bf16-exact in bf16 mode. Expected: the
           mode's kept-product model (x3 six products, x2 three, bf16 one) bit for bit.
  impulse  whole path: the map is zero except for one ±1 impulse in every fifth pixel, each in a channel of its
           own; every (cout, cin) pair has one non-zero tap, ±225 (F(4×4): G holds thirds and fifteenths, so
           U = G g Gᵀ is an integer of magnitude <= 256, bf16-exact) or ±4 (F(2×2): G holds halves). V is then a
           single product of two Bᵀ entries (bf16-exact), every product and partial sum a multiple of 2^-8, and
           `build` asserts that the path evaluated on absolute values stays below 2^16. Expected: the direct 3×3
           cross-correlation through the dyadic epilogue, bit for bit.
  range    judged per element against a derived bound (below); three maps: N(0,1) with the row / channel
           power-of-two scaling of conv_refs ("normal"), 100 + N(0,1) ("offset"), max(N(0,1) + 1, 0)·2^((c mod 9) - 4)
           ("relu"); real BN constants, silu / gelu, residuals.

Bounds of the range family (u = 2^-24, γ(n) = n·u / (1 - n·u); no term comes from a kernel's output)
  in    The kernels form q = Σ_j Bᵀ[b][j] d[i][j] and V = Σ_i Bᵀ[a][i] q[i] as chains of fused multiply-adds with
        exact (dyadic) coefficients: a chain over the n non-zeros of a row carries at most n roundings, so
        |V̂ - V| <= γ(nnz(Bᵀ[a]) + nnz(Bᵀ[b])) · (|Bᵀ| |d| |B|)[a][b]. F(2×2)'s additions are counted the same way
        (two non-zeros per row; the kernel rounds once per row).
  out   The same with Aᵀ: |Ŷ - Y| <= γ(nnz(Aᵀ[p]) + nnz(Aᵀ[q])) · (|Aᵀ| |M| |A|)[p][q], then the epilogue terms of
        conv_refs.build (4u on the affine and res1, the activation's slope and own error, 2u on res2).
  gemm  conv_refs.build's e_acc with S = |V| |U|: C_MODE·(knz + 1)·u·S (+ 3.1·2^-16·S for x2: the dropped lo·lo
        and the second-plane rounding).
  path  the stage bounds propagated: e_V through |U|, the fp32 rounding of U (u·|U|, through |V| + e_V), e_acc
        on S = (|V| + e_V)|U|, in bf16 mode the two operand roundings (2^-9 each, and their product), the sum e_M
        through |Aᵀ|·|A|, the output transform's own γ on |Aᵀ|(S + e_M)|A|, then the epilogue terms. The reference
        is the direct fp64 cross-correlation of the fp32 map and the fp32 3×3 weights.
"""
from __future__ import annotations

import zlib

import numpy as np

import conv_refs as R
from conv_refs import C_MODE, GUARD, PLANES, TAIL, U, act64, bf16_bits, bf16_round, bf16_val, compare, planes_of  # noqa: F401

BT = {2: np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64),
      4: np.array([[4, -6, -8, 6, 4, 0], [0, 4, -10, 2, 4, 0], [0, -4, 2, 10, 4, 0], [0, -8, -4, 8, 4, 0],
                   [0, 2, -4, -2, 4, 0], [0, 4, -6, -8, 6, 4]], np.float64) / 4}
AT = {2: np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64),
      4: np.array([[8, 8, 8, 8, 8, 0], [0, -8, 8, 4, -16, 0], [0, 8, 8, 2, 32, 0], [0, -8, 8, 1, -64, 8]],
                  np.float64) / 8}
G = {2: np.array([[2, 0, 0], [1, 1, 1], [1, -1, 1], [0, 0, 2]], np.float64) / 2,
     4: np.array([[15, 0, 0], [-5, 5, -5], [5, 5, 5], [-16, -8, -4], [1, -2, 4], [0, 0, 15]], np.float64) / 15}
TAP = {2: 4.0, 4: 225.0}  # impulse family: the one non-zero tap of every (cout, cin) pair
MODES = ("x3", "x2", "bf16")
GROWS = 2  # NaN guard rows before and after the map in the A buffer
WINO_CFGS = (None, 63, 33, 14, 45, 44, 246, 247)  # tests/test_gpu_kernels.py WINO_CFGS
X2_FALLBACK_CFGS = (11, 220)  # LDS-DMA tiles outside kGldsX2Ids: the 2-way split falls back to the rule
HW = ((1, 1), (1, 5), (2, 3), (3, 2), (4, 4), (5, 1), (6, 7), (7, 6), (8, 9), (9, 8))
EPIS = ((), ("affine",), ("res1",), ("act",), ("res2",), ("affine", "res1", "act", "res2"))
PATH_SHAPES = ((2, 9, 11, 64, 96), (1, 1, 1, 32, 64), (3, 8, 6, 32, 4), (1, 5, 7, 128, 136))


def nc_of(wm):
    return (wm + 2) ** 2


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def tiles_of(n, h, w, wm):
    th, tw = (h + wm - 1) // wm, (w + wm - 1) // wm
    return th, tw, n * th * tw


# ------------------------------------------------------------------------------------------------ fp64 stages
def patches(x, wm):
    """NHWC [n, h, w, c] → the (wm+2)² input patches [T, wm+2, wm+2, c] (rows / cols wm·t - 1 .., zero padding)."""
    n, h, w, c = x.shape
    th, tw, T = tiles_of(n, h, w, wm)
    P = wm + 2
    xp = np.zeros((n, th * wm + 2, tw * wm + 2, c), x.dtype)
    xp[:, 1:h + 1, 1:w + 1] = x
    d = np.empty((n, th, tw, P, P, c), x.dtype)
    for i in range(P):
        for j in range(P):
            d[:, :, :, i, j] = xp[:, i:i + th * wm:wm, j:j + tw * wm:wm]
    return d.reshape(T, P, P, c)


def input_ref(x, wm, bt=None):
    """V = Bᵀ d B of every tile, fp64 [NC, T, Cin] (bt: another matrix in Bᵀ's place, e.g. |Bᵀ|)."""
    bt = BT[wm] if bt is None else bt
    d = patches(np.asarray(x, np.float64), wm)
    v = np.einsum("ai,tijc,bj->abtc", bt, d, bt, optimize=True)
    return v.reshape(nc_of(wm), d.shape[0], d.shape[3])


def in_counts(wm):
    """Roundings of V's component ab: nnz(Bᵀ[a]) + nnz(Bᵀ[b]), [NC, 1, 1]."""
    nz = (BT[wm] != 0).sum(axis=1)
    return (nz[:, None] + nz[None, :]).reshape(-1, 1, 1).astype(np.float64)


def gemm_ref(v, u):
    """M_ab = V_ab · U_abᵀ: [NC, T, Cin] × [NC, Cout, Cin] → [NC, T, Cout] fp64."""
    return np.matmul(np.asarray(v, np.float64), np.asarray(u, np.float64).transpose(0, 2, 1))


def untile(yt, n, h, w, wm):
    """[T, wm, wm, c] tile outputs → [n·h·w, c] rows (the ragged last tile row / column cropped)."""
    th, tw, T = tiles_of(n, h, w, wm)
    c = yt.shape[-1]
    y = yt.reshape(n, th, tw, wm, wm, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, th * wm, tw * wm, c)
    return np.ascontiguousarray(y[:, :h, :w]).reshape(n * h * w, c)


def output_ref(m, n, h, w, wm, at=None, transposed=False):
    """Y = Aᵀ M A of every tile → [n·h·w, Cout] fp64 (at: another matrix in Aᵀ's place; transposed: the defect
    that reads component (b, a) for (a, b))."""
    at = AT[wm] if at is None else at
    P = wm + 2
    m4 = np.asarray(m, np.float64).reshape(P, P, m.shape[1], m.shape[2])
    if transposed:
        m4 = m4.transpose(1, 0, 2, 3)
    return untile(np.einsum("pa,abtc,qb->tpqc", at, m4, at, optimize=True), n, h, w, wm)


def out_counts(n, h, w, wm, c):
    """Roundings of output pixel (p, q) of a tile: nnz(Aᵀ[p]) + nnz(Aᵀ[q]), as [n·h·w, c] rows."""
    nz = (AT[wm] != 0).sum(axis=1).astype(np.float64)
    _, _, T = tiles_of(n, h, w, wm)
    t = np.broadcast_to((nz[:, None] + nz[None, :])[None, :, :, None], (T, wm, wm, c))
    return untile(np.ascontiguousarray(t), n, h, w, wm)


def direct_ref(x, wk):
    """The 3×3 stride-1 pad-1 cross-correlation in fp64: x NHWC, wk [Cout, 3, 3, Cin] → [n·h·w, Cout]."""
    cols = R.im2col(np.asarray(x, np.float64), 3, 1, 1)
    return cols @ np.asarray(wk, np.float64).reshape(wk.shape[0], -1).T


def weights_ref(wk, wm):
    """U = G g Gᵀ in fp64, [NC, Cout, Cin]."""
    g = np.asarray(wk, np.float64)
    u = np.einsum("ai,oijc,bj->aboc", G[wm], g, G[wm])
    return u.reshape(nc_of(wm), g.shape[0], g.shape[3])


# ------------------------------------------------------------------------------------------------ cases
def _case(stage, fam, wm, mode, shape, **f):
    """Flags: gap (A / C rows inside a wider buffer: lda = Cin + 32 from column 16, ldc = Cout + 24 from column 8),
    epi (the epilogue parts given: affine, res1, act, res2), map (range: normal | offset | relu), cfg (forced tile
    id, gemm), tile (the tile the rule must choose, asserted through sp_winograd_plan), in_vw (asserted likewise)."""
    c = dict(stage=stage, fam=fam, wm=wm, mode=mode, shape=tuple(shape), gap=False, epi=(), map="normal", cfg=None,
             tile=None, in_vw=None, c_bf16=False)
    assert set(f) <= set(c), set(f) - set(c)
    c.update(f)
    tag = ",".join(f"{k}={'+'.join(v) if isinstance(v, tuple) else v}" for k, v in sorted(f.items()) if v)
    c["id"] = f"{stage}{wm}-{fam}-{mode}-{'x'.join(map(str, shape))}" + (f"-{tag}" if tag else "")
    return c


def layout(c):
    """Element layout of a case's buffers."""
    n, h, w, cin, cout = c["shape"]
    wm = c["wm"]
    th, tw, T = tiles_of(n, h, w, wm)
    nc = nc_of(wm)
    lda = cin + (32 if c["gap"] else 0)
    ldc = cout + (24 if c["gap"] else 0)
    m = n * h * w
    return dict(M=m, T=T, th=th, tw=tw, NC=nc, lda=lda, a_off=GROWS * lda + (16 if c["gap"] else 0),
                a_numel=(m + 2 * GROWS) * lda, ldc=ldc, c_off=8 if c["gap"] else 0, c_numel=m * ldc + TAIL,
                ldr1=cout + 4, ldr2=cout + 8, v_el=nc * T * cin, m_el=nc * T * cout,
                work_numel=nc * T * (cin + cout) + TAIL)


def rule_tile(nc, T, cout):
    """The component GEMM's tile rule (winograd.hip wino_plan) → cfg (tile, or 200 + tile: direct-store form)."""
    rows = nc * T
    if cout % 128 == 0 and 12000 <= rows < 20000:
        return 63 if cout >= 256 else 14
    if cout % 128 or rows < 12000:
        return 14
    if rows >= 400000 and cout >= 384:
        return 247
    return 246 if cout <= 256 else 245


def expected_plan(c):
    """The sp_conv_plan_info tuple (conv_refs.plan_key) of the case's component GEMM: the forced id where it
    applies, else the rule; 200 + id runs epilogue 4 on split operands (the 1×1 fast path always holds here)."""
    n, h, w, cin, cout = c["shape"]
    L = layout(c)
    g = R.glds_configs()
    planes = PLANES[c["mode"]]
    cfg = c["cfg"]
    if cfg is not None and planes == 2 and not g[cfg % 100]["fit2"]:
        cfg = None
    if cfg is None:
        cfg = rule_tile(L["NC"], L["T"], cout)
    req = 4 if cfg >= 200 else 2 if cfg >= 100 else 1
    epv = req if planes >= 2 and req > 1 else 1
    return (2, cfg % 100, planes, 0, 0, 1, epv, 0, 0)


def _gemm_shape(T, cin, cout, wm):
    return (1, 1, T * wm, cin, cout)


def gemm_cases():
    """Forced ids × modes over the (T, Cin, Cout) sets (a covering, not the full product: every value of every
    set occurs with every mode), then every branch of the rule at its smallest shape."""
    Ts, cins, couts = (1, 63, 65, 130, 257), (32, 64, 160), (4, 48, 128, 136, 256, 384)
    out, i = [], 0
    for mode in MODES:
        cfgs = WINO_CFGS + (X2_FALLBACK_CFGS if mode == "x2" else ())
        for cfg in cfgs:
            for rep in range(3):
                T, cin, cout = Ts[i % 5], cins[(i // 2) % 3], couts[(i + i // 6) % 6]
                wm = 2 if i % 2 else 4
                fam = ("probe", "ints", "range")[rep] if cfg in (None, 14, 246) else ("probe", "ints")[rep % 2]
                out.append(_case("gemm", fam, wm, mode, _gemm_shape(T, cin, cout, wm), cfg=cfg))
                i += 1
    # the full T × Cin × Cout product per mode under the rule (all short batches: tile 14), F(2×2) and F(4×4)
    # batches alternating
    for mode in MODES:
        for T in Ts:
            for cin in cins:
                for cout in couts:
                    wm = 2 if i % 2 else 4
                    out.append(_case("gemm", ("probe", "ints")[(i // 2) % 2], wm, mode, _gemm_shape(T, cin, cout, wm)))
                    i += 1
    # the rule's branches (wm 4: NC = 36; rows = 36·T): below / inside / above the short-batch band, by Cout
    for mode in MODES:
        for T, cout, tile in ((333, 128, 14), (334, 132, 14), (334, 128, 14), (334, 256, 63), (556, 128, 246),
                              (556, 256, 246), (556, 384, 245), (556, 136, 14)):
            out.append(_case("gemm", "ints" if mode != "bf16" else "probe", 4, mode, _gemm_shape(T, 32, cout, 4),
                             tile=tile))
        # F(2×2): NC = 16, the same thresholds in rows
        out.append(_case("gemm", "probe", 2, mode, _gemm_shape(750, 32, 256, 2), tile=63))
        out.append(_case("gemm", "probe", 2, mode, _gemm_shape(1250, 32, 128, 2), tile=246))
    seen = set()  # (a product case may repeat a case of the covering)
    return [c for c in out if not (c["id"] in seen or seen.add(c["id"]))]


# tile 247 needs 400000 rows × Cout >= 384 (a 600 MB M): the instance runs at a small shape under the forced id
# (gemm_cases: cfg 247), and the host test asserts that the rule's tuple at this shape is that very tuple
RULE_247_SHAPE = dict(wm=4, T=11112, cin=32, cout=384)


def transform_cases(stage):
    out, i = [], 0
    for wm in (2, 4):
        for fam in ("ints", "range"):
            for (h, w) in HW:
                for n in (1, 3):
                    for ch in ((32, 96) if stage == "in" else (4, 8, 132)):
                        for gap in (False, True):
                            shape = (n, h, w, ch, 4) if stage == "in" else (n, h, w, 32, ch)
                            f = dict(gap=gap)
                            if stage == "out":
                                f["epi"] = EPIS[i % 6]
                            if fam == "range":
                                f["map"] = ("normal", "offset", "relu")[i % 3]
                            out.append(_case(stage, fam, wm, "x3", shape, **f))
                            i += 1
    if stage == "in":  # the VW switch of the F(4×4) input transform at 2^18 tile × channel items
        out.append(_case("in", "ints", 4, "x3", (1, 28, 292, 512, 4), in_vw=1))   # T = 7·73 = 511
        out.append(_case("in", "ints", 4, "x3", (1, 64, 128, 512, 4), in_vw=2))   # T = 16·32 = 512
    return out


def path_cases():
    out, i = [], 0
    epis = (("affine", "res1", "act"), ("affine", "act"), ("affine", "act", "res2"))
    for wm in (2, 4):
        for mode in MODES:
            for shape in PATH_SHAPES:
                for fam in ("impulse", "range"):
                    f = dict(epi=epis[i % 3], gap=bool(i % 2))
                    if fam == "range":
                        f["map"] = ("normal", "offset", "relu")[i % 3]
                    out.append(_case("path", fam, wm, mode, shape, **f))
                    i += 1
    return out


_cases = {}


def cases(stage):
    if stage not in _cases:
        _cases[stage] = {"in": lambda: transform_cases("in"), "out": lambda: transform_cases("out"),
                         "gemm": gemm_cases, "path": path_cases}[stage]()
        ids = [c["id"] for c in _cases[stage]]
        assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:3]
    return _cases[stage]


def fake_desc(c):
    """The case's sp_conv_desc on fake aligned pointers (no device), as conv_refs.fake_desc does it."""
    from spotter_amd._lib import SpConvDesc

    n, h, w, cin, cout = c["shape"]
    L = layout(c)
    d = dict(A=R.PTR["A"] + 4 * L["a_off"], lda=L["lda"], N=n, H=h, W=w, Cin=cin, KH=3, KW=3, stride=1, pad=1, Ho=h,
             Wo=w, Wt=R.PTR["Wt"], Cout=cout, C=R.PTR["C"] + 4 * L["c_off"], ldc=L["ldc"],
             precision=R.PRECISION[c["mode"]], act=R.ACTS.index(_act(c)))
    if "affine" in c["epi"]:
        d.update(scale=R.PTR["scale"], shift=R.PTR["shift"])
    if "res1" in c["epi"]:
        d.update(res1=R.PTR["res1"], ldr1=L["ldr1"])
    if "res2" in c["epi"]:
        d.update(res2=R.PTR["res2"], ldr2=L["ldr2"])
    return SpConvDesc(**d)


class forced:
    """with forced(cfg): the calling thread's sp_set_conv_config, restored on exit."""

    def __init__(self, cfg):
        self.cfg = cfg

    def __enter__(self):
        from spotter_amd import _lib

        _lib.load().sp_set_conv_config(-1 if self.cfg is None else self.cfg)

    def __exit__(self, *exc):
        from spotter_amd import _lib

        _lib.load().sp_set_conv_config(-1)


def plan_of(desc, wm, **kw):
    """sp_winograd_plan of a descriptor under the current overrides → (gemm key, components, tiles, in_vw, out_vw)."""
    p = R._ops().wino_plan(desc, wm, **kw)
    return R.plan_key(p["gemm"]), p["components"], p["tiles"], p["in_vw"], p["out_vw"]


# ------------------------------------------------------------------------------------------------ operands
def _act(c):
    if "act" not in c["epi"]:
        return None
    if c["fam"] != "range":
        return "relu"
    return ("relu", "silu", "gelu")[zlib.crc32(c["id"].encode()) % 3]


def _map(rng, c):
    n, h, w, cin, _ = c["shape"]
    z = rng.standard_normal((n, h, w, cin))
    if c["map"] == "offset":
        return (100.0 + z).astype(np.float32)
    if c["map"] == "relu":
        return (np.maximum(z + 1.0, 0.0) * 2.0 ** ((np.arange(cin) % 9) - 4.0)).astype(np.float32)
    rs = 2.0 ** ((np.arange(n * h * w) % 21) - 10.0)
    cs = 2.0 ** ((np.arange(cin) % 9) - 4.0)
    return (z * (rs[:, None] * cs[None, :]).reshape(n, h, w, cin)).astype(np.float32)


def _epilogue_operands(rng, c, m, cout, exact, typ):
    """scale, shift, r1, r2 (fp32 or None) for the parts in c["epi"]; typ: a typical |accumulator|."""
    e = dict(scale=None, shift=None, r1=None, r2=None, act=_act(c))
    if "affine" in c["epi"]:
        if exact:
            e["scale"] = R._pick(rng, (1.0, 2.0, 0.5), cout)
            e["shift"] = (rng.integers(-2048, 2049, cout) / 1024.0).astype(np.float32)
        else:  # FrozenBN constants, a few channels pushed to ±20 and below -88 (conv_refs.build)
            e["scale"] = (rng.uniform(0.5, 1.5, cout) / np.sqrt(rng.uniform(0.25, 4.0, cout) + 1e-5)).astype(np.float32)
            e["shift"] = rng.standard_normal(cout).astype(np.float32)
            idx = np.arange(0, cout, 3)
            e["shift"][idx] = np.resize(np.float32([-100.0, 20.0, -20.0, -90.0]), len(idx))
    for key, part in (("r1", "res1"), ("r2", "res2")):
        if part in c["epi"]:
            if exact:
                e[key] = (rng.integers(-128, 129, (m, cout)) / 1024.0).astype(np.float32)
            else:
                e[key] = (rng.standard_normal((m, cout)) * (1.0 + typ * 0.01)).astype(np.float32)
    return e


def epilogue(acc, e, res2_first=False):
    """The header's formula in fp64 → (acc·scale + shift, + res1, act, + res2). res2_first: the defect that adds
    res2 before the activation."""
    sc = e["scale"].astype(np.float64)[None, :] if e["scale"] is not None else 1.0
    sh = e["shift"].astype(np.float64)[None, :] if e["shift"] is not None else 0.0
    r1 = e["r1"].astype(np.float64) if e["r1"] is not None else 0.0
    r2 = e["r2"].astype(np.float64) if e["r2"] is not None else 0.0
    t2 = acc * sc + sh
    t3 = t2 + r1
    if res2_first:
        return t2, t3, act64(t3 + r2, e["act"]), act64(t3 + r2, e["act"])
    f = act64(t3, e["act"])
    return t2, t3, f, f + r2


def epilogue_bound(acc_true, e_acc, e):
    """conv_refs.build's range bound behind the accumulator (no row_scale)."""
    sc = np.abs(e["scale"].astype(np.float64))[None, :] if e["scale"] is not None else 1.0
    sh = np.abs(e["shift"].astype(np.float64))[None, :] if e["shift"] is not None else 0.0
    r1 = np.abs(e["r1"].astype(np.float64)) if e["r1"] is not None else 0.0
    r2 = np.abs(e["r2"].astype(np.float64)) if e["r2"] is not None else 0.0
    t2, t3, f, out = epilogue(acc_true, e)
    e_pre = e_acc * sc + 4 * U * (np.abs(acc_true * sc) + sh + r1)
    slope, e_act = {None: (1.0, 0.0), "relu": (1.0, 0.0), "silu": (1.1, 8 * U * np.abs(f)),
                    "gelu": (1.13, 8 * U * np.abs(t3))}[e["act"]]
    return slope * e_pre + e_act + 2 * U * (np.abs(f) + r2) + 2.0 ** -126


def _exact_epilogue(acc, e, cid):
    steps = epilogue(acc, e)
    R._exact32(acc, "transform output", cid)
    for name, v in zip(("·scale+shift", "+res1", "act", "+res2"), steps):
        R._exact32(np.broadcast_to(v, acc.shape), name, cid)
    return steps[-1]


def gemm_model(v, u, mode):
    """The mode's operand model of M = V·Uᵀ per component in fp64: (kept-product accumulator, S = |V||U|, knz).
    v [NC, T, Cin] fp32; u [NC, Cout, Cin] fp32 (bf16 mode: the values its bits decode to)."""
    ut = lambda a: a.astype(np.float64).transpose(0, 2, 1)  # noqa: E731
    if mode == "bf16":
        aop = bf16_round(v).astype(np.float64)
        acc = np.matmul(aop, ut(u))
        s_a = aop
    else:
        pa = [p.astype(np.float64) for p in planes_of(v, mode)]
        pw = [ut(p) for p in planes_of(u, mode)]
        if mode == "x3":
            acc = np.matmul(pa[0], pw[0] + pw[1] + pw[2]) + np.matmul(pa[1], pw[0] + pw[1]) + np.matmul(pa[2], pw[0])
        else:
            acc = np.matmul(pa[0], pw[0] + pw[1]) + np.matmul(pa[1], pw[0])
        s_a = v.astype(np.float64)
    S = np.matmul(np.abs(s_a), np.abs(ut(u)))
    knz = np.matmul((s_a != 0).astype(np.float32), (ut(u) != 0).astype(np.float32)).astype(np.float64)
    return acc, S, knz


def e_acc_of(mode, knz, S):
    return C_MODE[mode] * (knz + 1) * U * S + (3.1 * 2.0 ** -16 * S if mode == "x2" else 0.0)


def weight_planes(u, mode):
    """U [NC, Cout, Cin] fp32 → the int16 planes [1, 2 or 3][NC·Cout·Cin] the GEMM streams."""
    ops = R._ops()
    if mode == "bf16":
        return bf16_bits(u).reshape(1, -1).view(np.int16)
    return (ops.split_bf16x3_host if mode == "x3" else ops.split_bf16x2_host)(u)


def build(c):
    """Operands, the fp64 reference and (range) the per-element bound of a case → dict:
      in:   x (NHWC fp32), ref / bound [NC, T, Cin]
      out:  m (fp32 [NC, T, Cout]), scale, shift, r1, r2, act, ref / bound [n·h·w, Cout]
      gemm: v (fp32 [NC, T, Cin]), u (fp32 [NC, Cout, Cin]), planes (int16), ref / bound [NC, T, Cout]
      path: x, wk (fp32 [Cout, 3, 3, Cin]), u, planes, the epilogue operands, ref / bound [n·h·w, Cout]"""
    n, h, w, cin, cout = c["shape"]
    wm, fam, mode, cid, stage = c["wm"], c["fam"], c["mode"], c["id"], c["stage"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    L = layout(c)
    nc, T, m = L["NC"], L["T"], L["M"]
    exact = fam != "range"
    r = dict(act=_act(c))
    if stage == "in":
        if exact:
            x = rng.integers(-8, 9, (n, h, w, cin)).astype(np.float32)
        else:
            x = _map(rng, c)
        ref = input_ref(x, wm)
        absv = input_ref(np.abs(x), wm, np.abs(BT[wm]))
        if exact:
            R._exact32(ref, "V", cid)
            assert (absv * 4).max() < 2 ** 24 and np.array_equal(ref * 4, np.rint(ref * 4)), cid
            bound = np.zeros_like(ref)
        else:
            bound = gamma(in_counts(wm)) * absv + 2.0 ** -126
        r.update(x=x, ref=ref, bound=bound)
    elif stage == "out":
        if exact:
            rad = 32 if c["epi"] and set(c["epi"]) != {"act"} else 1024
            mm = rng.integers(-rad, rad + 1, (nc, T, cout)).astype(np.float32)
        else:
            rs = 2.0 ** ((np.arange(T) % 21) - 10.0)
            cs = 2.0 ** ((np.arange(cout) % 9) - 4.0)
            mm = (rng.standard_normal((nc, T, cout)) * rs[None, :, None] * cs[None, None, :]).astype(np.float32)
        y = output_ref(mm, n, h, w, wm)
        absy = output_ref(np.abs(mm), n, h, w, wm, np.abs(AT[wm]))
        e = _epilogue_operands(rng, c, m, cout, exact, float(np.abs(y).mean()))
        if exact:
            assert (absy * 64).max() < 2 ** 24 and np.array_equal(y * 64, np.rint(y * 64)), cid
            ref = _exact_epilogue(y, e, cid)
            bound = np.zeros_like(ref)
        else:
            ref = epilogue(y, e)[-1]
            bound = epilogue_bound(y, gamma(out_counts(n, h, w, wm, cout)) * absy, e)
        r.update(m=mm, ref=ref, bound=bound, y=y, **e)
    elif stage == "gemm":
        fc = dict(mode=mode, a_rows=False, shape=(1, 1, nc * T, cin, cout, 1, 1, 0))
        if fam == "probe":
            av, wv = R._probe_sets(fc)
            v = R._probe_a(rng, fc, av).reshape(nc, T, cin)
            u = R._pick(rng, wv, (nc, cout, cin))
        elif fam == "ints":
            v = rng.integers(-4, 5, (nc, T, cin)).astype(np.float32)
            u = rng.integers(-4, 5, (nc, cout, cin)).astype(np.float32)
        else:
            rs = 2.0 ** ((np.arange(nc * T) % 21) - 10.0).reshape(nc, T, 1)
            cs = 2.0 ** ((np.arange(cin) % 9) - 4.0)
            v = (rng.standard_normal((nc, T, cin)) * rs * cs).astype(np.float32)
            u = rng.standard_normal((nc, cout, cin)).astype(np.float32)
        if mode == "bf16":
            u = bf16_round(u)
        acc, S, knz = gemm_model(v, u, mode)
        if exact:
            if fam == "probe":
                assert knz.max() <= 56 and S.max() < 64.0, (cid, knz.max(), S.max())
            R._exact32(acc, "accumulator", cid)
            ref, bound = acc, np.zeros_like(acc)
        else:
            vt = bf16_round(v) if mode == "bf16" else v
            ref = gemm_ref(vt, u)
            bound = e_acc_of(mode, knz, S) + 2.0 ** -126
        r.update(v=v, u=u, planes=weight_planes(u, mode), ref=ref, bound=bound)
    else:
        if fam == "impulse":
            x = np.zeros((n, h, w, cin), np.float32)
            for b in range(n):  # every fifth pixel, the phase moving with the image
                pix = np.arange(b % 5, h * w, 5)
                ch = (np.arange(len(pix)) + 3 * b) % cin
                x[b].reshape(h * w, cin)[pix, ch] = np.where((np.arange(len(pix)) + b) % 2, -1.0, 1.0)
            assert ((x != 0).sum(axis=(1, 2)) <= 1).all(), cid  # one impulse per image and channel at most
            wk = np.zeros((cout, 9, cin), np.float32)
            o, i = np.meshgrid(np.arange(cout), np.arange(cin), indexing="ij")
            wk[o, (o * 4 + i) % 9, i] = np.where((o + i) % 3 == 0, -TAP[wm], TAP[wm])
            wk = wk.reshape(cout, 3, 3, cin)
        else:
            x = _map(rng, c)
            wk = (rng.standard_normal((cout, 3, 3, cin)) / np.sqrt(9.0 * cin)).astype(np.float32)
        u = R._ops().winograd_weights_host(wk, wm)
        if mode == "bf16":
            u = bf16_round(u)
        y = direct_ref(x, wk)
        e = _epilogue_operands(rng, c, m, cout, exact, float(np.abs(y).mean()))
        absv = input_ref(np.abs(x), wm, np.abs(BT[wm]))
        uabs = np.abs(u.astype(np.float64))
        if exact:
            v = input_ref(x, wm)
            assert np.array_equal(weights_ref(wk, wm), u.astype(np.float64)), cid  # integers: U is exact
            assert np.array_equal(u, bf16_round(u)) and np.array_equal(v.astype(np.float32), bf16_round(v.astype(np.float32))), cid
            yabs = output_ref(np.matmul(absv, uabs.transpose(0, 2, 1)), n, h, w, wm, np.abs(AT[wm]))
            assert yabs.max() * 256 < 2 ** 24, (cid, yabs.max())
            assert np.array_equal(output_ref(gemm_ref(v, u), n, h, w, wm), y), cid
            ref = _exact_epilogue(y, e, cid)
            bound = np.zeros_like(ref)
        else:
            e_v = gamma(in_counts(wm)) * absv
            vhat = absv + e_v
            ut = uabs.transpose(0, 2, 1)
            S = np.matmul(vhat, ut)
            e_m = np.matmul(e_v, ut) + U * S + e_acc_of(mode, float(cin), S)
            if mode == "bf16":  # V and U each rounded to 8 significant bits (2^-9 relative), and their product
                e_m = e_m + (2.0 ** -8 + 2.0 ** -18) * S
            e_y = (output_ref(e_m, n, h, w, wm, np.abs(AT[wm]))
                   + gamma(out_counts(n, h, w, wm, cout)) * output_ref(S + e_m, n, h, w, wm, np.abs(AT[wm])))
            ref = epilogue(y, e)[-1]
            bound = epilogue_bound(y, e_y, e)
        r.update(x=x, wk=wk, u=u, planes=weight_planes(u, mode), ref=ref, bound=bound, y=y, **e)
    assert np.isfinite(r["ref"]).all() and np.isfinite(r["bound"]).all(), cid
    return r
