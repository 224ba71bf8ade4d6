"""fp64 references, input families and the case matrix of the whole sp_conv_desc contract (include/spotter_hip.h).

No GPU and no torch: tests/test_conv_refs.py checks everything here on the host (float32 emulations of every
operand mode, the coverage ledger against tests/golden/conv_plan.jsonl.gz), tests/test_gpu_conv_plans.py launches
the same matrix on the MI355X. DESIGN.md ("Conv / GEMM instances against fp64") states the arguments.

A case is a plain dict (see `_case`). `want` is the sp_conv_plan_info tuple the case was built to run:
(family, tile, planes, generic, a_bf16, fast_1x1, epilogue, splits > 1, counters). Both test files assert that
sp_conv_plan names exactly that instance for the case's descriptor before anything is compared.

Families
  probe  operands from {0, ±1, ±(1+2^-9)} (+ ±(1+2^-9+2^-18) for the split modes, + the three bf16 rounding ties
         for bf16 A given as fp32 rows, + bf16-exact ±(1+2^-7), ±(1+2^-6) where an operand is bf16 in memory).
         A sparse (at most 56 non-zero products per output, at least one non-zero channel in every 16-deep
         k-step of every tap of every pixel), W dense: every kept product and every partial sum in any order is
         a multiple of 2^-18 below 2^6, exact in fp32, so the output must equal the fp64 operand model bit for
         bit. `build` asserts the cap, the range and the fp32 representability of every epilogue intermediate.
  ints   dense integers in [-4, 4], K·16 < 2^24: exact in every mode at full K (long pipelines, split-K).
  range  N(0,1) operands, row m scaled by 2^((m mod 21) - 10), channel k by 2^((k mod 9) - 4), real BN constants
         and residuals, silu / gelu; judged per element against `bound` (no term from any kernel's output).
"""
from __future__ import annotations

import gzip
import json
import os
import re
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODES = ("fp32", "bf16", "x3", "x2")
PLANES = {"fp32": 0, "bf16": 1, "x3": 3, "x2": 2}
MODE_OF_PLANES = {v: k for k, v in PLANES.items()}
PRECISION = {"fp32": 0, "bf16": 1, "x3": 2, "x2": 3}  # sp_precision
# accumulator additions per operand product: the products the mode keeps (c_mode of the range bound)
C_MODE = {"fp32": 1, "bf16": 1, "x3": 6, "x2": 3}
ACTS = (None, "relu", "silu", "gelu")
U = 2.0 ** -24  # unit roundoff of fp32
FAMILIES = ("probe", "ints", "range")
GUARD = 8      # guard columns right of every output row
TAIL = 64      # guard elements behind the last output row
FP32_IDS = [110, 111, 120, 121, 210, 211, 220, 221, 1110, 1111, 1120, 1121, 4110, 4111, 4120, 4121, 4210, 4211]
REG_TILE = {1: (128, 128), 2: (256, 128), 3: (64, 128), 4: (64, 64), 5: (128, 256), 6: (128, 64)}  # kRegTile


# ------------------------------------------------------------------------------------------------ bf16 helpers
def _ops():
    import sys

    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from spotter_amd import ops

    return ops


def bf16_bits(a):
    return _ops().bf16_bits(a).reshape(np.shape(a))


def bf16_val(bits):
    return (np.asarray(bits).astype(np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(a):
    """fp32 → the fp32 value of its RNE bf16 rounding."""
    return bf16_val(bf16_bits(a))


def bf16_trunc(a):
    """fp32 → the fp32 value of its bf16 truncation (what a defective loader would do)."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def planes_of(a, mode):
    """The bf16 planes (as fp32 values, same shape as a) of an fp32 operand in a split mode."""
    ops = _ops()
    a = np.ascontiguousarray(a, np.float32)
    p = ops.split_bf16x3_host(a) if mode == "x3" else ops.split_bf16x2_host(a)
    return [bf16_val(q.view(np.uint16)).reshape(a.shape) for q in p]


# plane pairs (A plane, W plane) the kernels keep: 0 hi, 1 mid (x3) or lo (x2), 2 lo (x3)
KEPT = {"x3": [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)], "x2": [(1, 0), (0, 1), (0, 0)]}


# ------------------------------------------------------------------------------------------------ tile data
def glds_configs():
    """SP_GLDS_CONFIGS and the membership sets of csrc/conv_plan.h → {id: dict(BM, BN, BK, NS, AB, fit1, fit3,
    fit1a, fit2, slab, a16_only)}, the LDS fits recomputed here from GldsCfg's formula (160 KB)."""
    src = open(os.path.join(ROOT, "spotter_amd", "csrc", "conv_plan.h")).read()
    sets = {n: [int(v) for v in re.search(n + r"\[\] = \{([^}]*)\}", src).group(1).split(",")]
            for n in ("kGldsSlabIds", "kGldsBf16AOnlyIds", "kGldsX2Ids")}
    out = {}
    for m in re.findall(r"^\s*X\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (true|false), (\d+), (true|false)\)",
                        src, re.M):
        tid, wm, wn, tm, tn, ns, bk = map(int, m[:7])
        ab = m[9] == "true"

        def fits(pl, apl=0):
            bm, bn = 32 * tm * wm, 32 * tn * wn
            ra, rb = (bk // 8 if apl else bk // 4), bk // 8
            stage = bm * ra * (apl or 1) + pl * bn * rb
            nb = tm if wm * wn * tm * 32 * tn * 32 // 4 <= ns * stage else 1
            epi = wm * wn * nb * 32 * tn * 32 // 4
            return max(ns * stage, epi) * 16 <= 163840

        out[tid] = dict(BM=32 * tm * wm, BN=32 * tn * wn, BK=bk, NS=ns, AB=ab, fit1=fits(1), fit3=fits(3),
                        fit1a=ab and fits(1, 1), fit2=tid in sets["kGldsX2Ids"] and fits(2),
                        slab=tid in sets["kGldsSlabIds"], a16_only=tid in sets["kGldsBf16AOnlyIds"])
    assert len(out) >= 36, len(out)
    return out


def tile_dims(family, tile):
    """(BM, BN, BK, NS) of an instance: the tile the shapes of its cases are relative to."""
    if family == 2:
        g = glds_configs()[tile]
        return g["BM"], g["BN"], g["BK"], g["NS"]
    if family == 1:
        return REG_TILE[tile] + (32, 2)
    tm, tn, db = (tile // 100) % 10, (tile // 10) % 10, tile % 10
    bm, bn = (128 * tm, 32 * tn) if tile >= 4000 else (32, 128 * tn) if tile >= 1000 else (64 * tm, 64 * tn)
    return bm, bn, 32, 2 if db else 1


# ------------------------------------------------------------------------------------------------ cases
def _case(want, fam, mode, shape, ov=(-1, -1, 0, 0, -1), **f):
    """One matrix case. shape = (n, h, w, cin, cout, k, stride, pad). Flags (all optional): a_rows (A given as
    bf16 rows), c_bf16, res1 / res2 ("f32" | "bf16"), a2, row_period, affine (scale + shift), act, rpg (rows per
    output group), odd_ld (odd ldc), a_off / lda (A off alignment), slice (output into a channel slice), ws
    (split-K workspace), cnt (arrival counters). ov = (cfg, split-K cfg, max_splits, min_ktiles, epilogue knob)."""
    c = dict(want=tuple(want), fam=fam, mode=mode, shape=tuple(shape), ov=tuple(ov), a_rows=False, c_bf16=False,
             res1=None, res2=None, a2=False, row_period=0, affine=False, act=None, rpg=0, odd_ld=False, a_off=0,
             lda=0, slice=False, ws=False, cnt=False)
    assert set(f) <= set(c), set(f) - set(c)
    c.update(f)
    tag = ",".join(f"{k}={v}" for k, v in sorted(f.items()) if v)
    c["id"] = f"{fam}-{mode}-{'x'.join(map(str, shape))}-cfg{ov[0]}" + (f"-{tag}" if tag else "")
    return c


def layout(c):
    """Element layout of a case's buffers: dict(M, K, Ho, Wo, lda, ldr1, ldr2, a_numel, ldc, c_off, c_numel, rpg,
    gstride)."""
    n, h, w, cin, cout, k, st, pad = c["shape"]
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    m = n * ho * wo
    lda = c["lda"] or cin
    ldc = cout + GUARD + (1 if c["odd_ld"] else 0) + (GUARD if c["slice"] else 0)
    c_off = GUARD if c["slice"] else 0
    rpg = c["rpg"]
    gstride = rpg * ldc + GUARD if rpg else 0
    rows_span = ((m + rpg - 1) // rpg) * gstride if rpg else m * ldc
    ldr = lambda kind: (cout + 7) // 8 * 8 if kind == "bf16" else cout  # the slab epilogue DMAs bf16 res1 rows
    return dict(M=m, K=k * k * cin, Ho=ho, Wo=wo, lda=lda, ldr1=ldr(c["res1"]), ldr2=ldr(c["res2"]),
                a_numel=c["a_off"] + n * h * w * lda, ldc=ldc, c_off=c_off,
                c_numel=rows_span + TAIL, rpg=rpg, gstride=gstride)


PTR = {f: 0x100000 + 0x100000 * i for i, f in enumerate(
    ["A", "A2", "Wt", "scale", "shift", "row_scale", "res1", "res2", "C", "workspace", "Wt_bf16", "counters"])}


def fake_desc(c):
    """The case's sp_conv_desc on fake pointers with the alignment the GPU test's tensors have (no device)."""
    from spotter_amd._lib import SpConvDesc

    n, h, w, cin, cout, k, st, pad = c["shape"]
    L = layout(c)
    esz = lambda b: 2 if b else 4
    d = dict(lda=L["lda"], N=n, H=h, W=w, Cin=cin, KH=k, KW=k, stride=st, pad=pad, Ho=L["Ho"], Wo=L["Wo"], Wt=PTR["Wt"],
             Cout=cout, ldc=L["ldc"], out_rows_per_group=L["rpg"], out_group_stride=L["gstride"],
             precision=PRECISION[c["mode"]], act=ACTS.index(c["act"]))
    d["A_bf16" if c["a_rows"] else "A"] = PTR["A"] + esz(c["a_rows"]) * c["a_off"]
    d["C_bf16" if c["c_bf16"] else "C"] = PTR["C"] + esz(c["c_bf16"]) * L["c_off"]
    if c["a2"]:
        d.update(A2=PTR["A2"], lda2=cin)
    if c["affine"]:
        d.update(scale=PTR["scale"], shift=PTR["shift"])
    if c["row_period"]:
        d.update(row_scale=PTR["row_scale"], row_period=c["row_period"])
    for r, ld in (("res1", "ldr1"), ("res2", "ldr2")):
        if c[r]:
            d[r + ("_bf16" if c[r] == "bf16" else "")] = PTR[r]
            d[ld] = L[ld]
    if c["mode"] != "fp32":
        d.update(Wt_bf16=PTR["Wt_bf16"], wt_plane_stride=cout * L["K"] if c["mode"] in ("x3", "x2") else 0)
    if c["ws"]:
        d.update(workspace=PTR["workspace"], workspace_elems=1 << 20)
    if c["cnt"]:
        d.update(splitk_counters=PTR["counters"], splitk_counters_len=1024)
    return SpConvDesc(**d)


class overrides:
    """with overrides(ov): the calling thread's sp_set_conv_config / sp_set_splitk_config / sp_set_tuning set to
    the case's, restored to the product defaults on exit."""

    def __init__(self, ov):
        self.ov = ov

    def __enter__(self):
        from spotter_amd import _lib

        L = _lib.load()
        L.sp_set_conv_config(self.ov[0])
        L.sp_set_splitk_config(self.ov[1], self.ov[2], self.ov[3])
        L.sp_set_tuning(3, self.ov[4])

    def __exit__(self, *exc):
        from spotter_amd import _lib

        L = _lib.load()
        L.sp_set_conv_config(-1)
        L.sp_set_splitk_config(-1, 0, 0)
        L.sp_set_tuning(3, -1)


PLAN_FIELDS = ("family", "tile", "planes", "generic", "a_bf16", "fast_1x1", "epilogue", "splits", "counters")


def plan_key(plan):
    """sp_conv_plan_info (dict or sequence in field order) → the ledger's tuple (splits as splits > 1)."""
    v = [plan[f] for f in PLAN_FIELDS] if isinstance(plan, dict) else list(plan)
    return tuple(v[:7]) + (int(v[7] > 1), v[8])


def plan_of(desc):
    """sp_conv_plan of a descriptor under the current overrides → (key, splits)."""
    p = _ops().conv_plan(desc)
    return plan_key(p), p["splits"]


# ------------------------------------------------------------------------------------------------ targets
def recorded_targets():
    """Every distinct tuple tests/golden/conv_plan.jsonl.gz records under effectively default overrides."""
    with gzip.open(os.path.join(ROOT, "tests", "golden", "conv_plan.jsonl.gz"), "rt") as f:
        _, *lines = [json.loads(ln) for ln in f]
    dflt, out = [-1, -1, 0, 0, -1], set()
    for _enc, o, res in lines:
        o = o + dflt[len(o):]
        if isinstance(res, str) or o[0] != -1 or o[1] != -1 or o[2] not in (0, 16) or o[3] not in (0, 8) or o[4] != -1:
            continue
        out.add(plan_key(res))
    return out


def targets():
    """{tuple: production?}: the recorded tuples, the planes-2 image of each planes-3 one on a kGldsX2Ids tile
    (production: the 2-way split takes the 3-way split's choice), and one tuple per remaining compiled instance."""
    g = glds_configs()
    t = {k: True for k in recorded_targets()}
    for k in list(t):
        if k[2] == 3 and ((k[0] == 2 and g[k[1]]["fit2"]) or k[0] == 1):
            t.setdefault(k[:2] + (2,) + k[3:], True)
    for tid, q in g.items():
        for mode, ok in (("bf16", q["fit1"] and not q["a16_only"]), ("x3", q["fit3"] and not q["a16_only"]),
                         ("x2", q["fit2"] and not q["a16_only"])):
            for fast in (0, 1):
                if ok:
                    t.setdefault((2, tid, PLANES[mode], 0, 0, fast, 1, 0, 0), False)
        if q["fit1a"]:
            for fast in (0, 1):
                for epv in (1, 3):
                    t.setdefault((2, tid, 1, 0, 1, fast, epv, 0, 0), False)
    for r in REG_TILE:
        for p in (1, 3, 2):
            t.setdefault((1, r, p, 0, 0, 0, 1, 0, 0), False)
    for p in (1, 3, 2):  # the generic gather and both split-K combines of every bf16-MFMA operand mode
        t.setdefault((1, 4, p, 1, 0, 0, 1, 0, 0), False)
        t.setdefault((1, 4, p, 0, 0, 0, 1, 1, 0), False)
        t.setdefault((1, 4, p, 0, 0, 0, 1, 1, 1), False)
    for i in FP32_IDS:
        t.setdefault((0, i, 0, 0, 0, 0, 1, 0, 0), False)
    return t


# ------------------------------------------------------------------------------------------------ the matrix
def _gemm(m, cout, kk, fast=True):
    """A 1×1 conv whose GEMM is m × cout × kk: stride 1 (the LDS-DMA kernels' 1×1 fast path) or, fast=False,
    stride 2 over a one-row map of 2m - 1 pixels (the same GEMM through the general path)."""
    return (1, 1, m, kk, cout, 1, 1, 0) if fast else (1, 1, 2 * m - 1, kk, cout, 1, 2, 0)


def _nks(ns, bk):
    """k-steps of the edge shape: 1, NS - 1, NS, NS + 1 (k16 tiles: rounded up to even, Cin % 32 == 0 is the
    fast operand path's condition)."""
    s = {1, ns - 1, ns, ns + 1} - {0}
    return sorted({v + (v & 1) if bk == 16 else v for v in s})


def cases_for(want, production):
    """The cases of one target tuple (all three families for a production tuple, probe + ints on the first two
    shapes for a compiled-only one)."""
    fam_id, tile, planes, generic, a16, fast, epv, split, cnt = want
    mode = MODE_OF_PLANES[planes]
    bm, bn, bk, ns = tile_dims(fam_id, tile)
    g = glds_configs().get(tile) if fam_id == 2 else None
    cfg = tile
    if fam_id == 2 and epv in (2, 4) and not (epv == 2 and g["slab"]):
        cfg = tile + (200 if epv == 4 else 100)
    ov = (-1, -1, 0, 0, -1) if split else (cfg, -1, 0, 0, -1)
    gemm_fast = bool(fast) or fam_id != 2
    # the flags every case of this tuple carries, and the variants it admits
    base = dict(a_rows=bool(a16))
    if fam_id == 2 and epv in (2, 4):
        base.update(affine=True, res1="f32", act="relu")
        variants = [dict()] + ([dict(res2="f32"), dict(rpg=16)] if epv == 2 else [])
    elif fam_id == 2 and epv == 3:
        base.update(c_bf16=True)
        variants = [dict(), dict(affine=True, res1="bf16", act="relu", slice=True)]
    elif fam_id == 2 and planes >= 2 and fast and g["slab"]:
        # the planner promotes a BN affine / residual to the slab epilogue here: variant 1 only without them,
        # with row_scale, or on the scalar epilogue
        variants = [dict(), dict(row_period=7, affine=True, res1="f32", act="relu"), dict(rpg=16)]
    else:
        variants = [dict(), dict(affine=True, res1="f32", act="relu"), dict(row_period=7, affine=True),
                    dict(affine=True, res1="f32", res2="f32", act="relu"), dict(rpg=16, affine=True)]
        if a16 or (planes == 1 and fam_id == 2):
            variants.append(dict(c_bf16=True, affine=True, res1="bf16", res2="bf16", act="relu", slice=True))
        if fam_id == 1 and not generic:
            variants.append(dict(a2=True))
    if split:
        base.update(ws=True, cnt=bool(cnt))
    if generic:
        shapes = [(1, 9, 9, 24, 40, 3, 1, 1), (1, 9, 9, 3, 32, 3, 2, 1), _gemm(37, 4, 24)]
        extra = [((2, 5, 7, 32, 36, 3, 1, 1), dict(a_off=1, lda=33))]  # A one float off alignment, odd lda
    elif split:
        shapes = [(1, 7, 10, 32 * nk, 68, 1, 1, 0) for nk in (8, 9, 16)]
        extra = []
    else:
        shapes = [_gemm(37, 4, 64, gemm_fast)]
        shapes += [_gemm(2 * bm + 1, 2 * bn + 4, nk * bk, gemm_fast) for nk in _nks(ns, bk)]
        extra = [(_gemm(37, 6, 64, gemm_fast), dict(odd_ld=True))]  # the scalar epilogue
        if fam_id != 2 or not fast:
            shapes += [(2, 5, 7, cin, 68, 3, st, 1) for st in (1, 2) for cin in (32, 64)]
        if (bm, bn) == (64, 64) and production:  # xcd_index: 7, 8 and 17 workgroups
            shapes += [_gemm(445, 60, 64, gemm_fast), _gemm(507, 64, 64, gemm_fast), _gemm(1087, 64, 64, gemm_fast)]
    if fam_id == 2 and epv in (2, 3, 4):
        extra = []  # the slab epilogues need the float4 epilogue
    fams = FAMILIES if production else FAMILIES[:2]
    out = []
    for fam in fams:
        acts = {"range": ("silu", "gelu")}.get(fam)
        if production:
            for i, s in enumerate(shapes):
                f = dict(base, **variants[0])
                if acts and f.get("act"):
                    f["act"] = acts[i % 2]
                out.append(_case(want, fam, mode, s, ov, **f))
            mid = shapes[min(2, len(shapes) - 1)]
            for i, v in enumerate(variants[1:]):
                f = dict(base, **v)
                if acts and f.get("act"):
                    f["act"] = acts[i % 2]
                out.append(_case(want, fam, mode, mid, ov, **f))
            for s, v in extra:
                out.append(_case(want, fam, mode, s, ov, **dict(base, **v)))
        else:
            n2 = 1 + len(_nks(ns, bk))
            for s in shapes[:n2] if not (generic or split) else shapes:
                out.append(_case(want, fam, mode, s, ov, **dict(base, **variants[0])))
            if fam_id == 1 and not (generic or split):  # only the register-staged tiles take the A2 addend
                for s in shapes[:2]:
                    f = dict(base, a2=True, affine=True, res1="f32", act="relu")
                    out.append(_case(want, fam, mode, s, ov, **f))
    return out


_matrix = None


def matrix():
    """[(want, production, [cases])] for every target tuple, in a fixed order."""
    global _matrix
    if _matrix is None:
        t = targets()
        _matrix = [(k, t[k], cases_for(k, t[k])) for k in sorted(t)]
    return _matrix


# ------------------------------------------------------------------------------------------------ operands
def im2col(a4, k, st, pad):
    """NHWC [n, h, w, c] → [M, k·k·c] with k in (tap, channel) order, zero padding."""
    n, h, w, c = a4.shape
    ho, wo = (h + 2 * pad - k) // st + 1, (w + 2 * pad - k) // st + 1
    ap = np.zeros((n, h + 2 * pad, w + 2 * pad, c), a4.dtype)
    ap[:, pad:pad + h, pad:pad + w] = a4
    cols = [ap[:, i:i + (ho - 1) * st + 1:st, j:j + (wo - 1) * st + 1:st] for i in range(k) for j in range(k)]
    return np.stack(cols, axis=3).reshape(n * ho * wo, k * k * c)


def _pick(rng, vals, shape, signed=True):
    v = rng.choice(np.asarray(vals, np.float64), size=shape)
    if signed:
        v = v * rng.choice([-1.0, 1.0], size=shape)
    return v.astype(np.float32)


V9, V918 = 1 + 2.0 ** -9, 1 + 2.0 ** -9 + 2.0 ** -18
TIES = (1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20)  # → 1, 1 + 2^-6, 1 + 2^-7 under RNE
BF_EXACT = (1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6)


def _probe_sets(c):
    """(A values, W values) of the probe family for the case's operand mode (magnitudes; signs are random)."""
    if c["mode"] == "bf16":
        return (BF_EXACT if c["a_rows"] else (1.0, V9) + TIES), BF_EXACT[:2]
    if c["mode"] == "fp32":
        return (1.0, V9), (1.0, V9)
    return (1.0, V9, V918), (1.0, V9, V918)


def _probe_a(rng, c, vals):
    """Sparse A: per pixel 56 // (k·k) non-zero channels at most, one in every 16-channel group (every k-step of
    every tap of every pixel holds a non-zero), the rest at random."""
    n, h, w, cin, cout, k, st, pad = c["shape"]
    budget = min(cin, 56 // (k * k))
    groups = [np.arange(s, min(s + 16, cin)) for s in range(0, cin, 16)]
    assert len(groups) <= budget, (cin, k)
    npix = n * h * w
    score = rng.random((npix, cin))
    for gr in groups:  # the group's chosen channel sorts first
        score[np.arange(npix), gr[0] + rng.integers(0, len(gr), npix)] = -1.0
    ch = np.argsort(score, axis=1)[:, :budget]
    a = np.zeros((npix, cin), np.float32)
    a[np.arange(npix)[:, None], ch] = _pick(rng, vals, ch.shape)
    assert all((a[:, gr] != 0).any(axis=1).all() for gr in groups)
    return a.reshape(n, h, w, cin)


def act64(v, act):
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "silu":
        with np.errstate(over="ignore"):
            return v / (1.0 + np.exp(-v))
    if act == "gelu":
        from math import erf

        return 0.5 * v * (1.0 + np.vectorize(erf)(v * 0.7071067811865476))
    return v


def _exact32(x, what, cid):
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64)), f"{cid}: {what} is not exact in fp32"


def build(c, splits=1):
    """Operands, the fp64 reference and (range) the per-element bound of a case. Returns a dict:
      a1, a2 (NHWC fp32; a1 bf16-exact with a_rows), w (fp32 [Cout, K]), w_bits (bf16 mode: uint16), scale, shift,
      row_scale, r1, r2 ([M, Cout] fp32 or None), acols / wop (the mode's operand model pieces), ref ([M, Cout]
      fp64: the expected output; for c_bf16 the value the RNE bits decode to is ref_bits), S, knz, bound."""
    n, h, w_, cin, cout, k, st, pad = c["shape"]
    fam, mode, cid = c["fam"], c["mode"], c["id"]
    rng = np.random.default_rng(zlib.crc32(cid.encode()))
    L = layout(c)
    m, kk = L["M"], L["K"]
    r = dict(a2=None, scale=None, shift=None, row_scale=None, r1=None, r2=None, w_bits=None)
    # ---- A (and the A2 addend: the loader's fp32 sum is the operand)
    if fam == "probe":
        av, wv = _probe_sets(c)
        t = _probe_a(rng, c, av)
        wt = _pick(rng, wv, (cout, kk))
        if c["a2"]:  # a1 + a2 == t exactly; where t is zero some pairs cancel (a1 = -a2 != 0)
            a2 = np.where(t != 0, np.sign(t), 0).astype(np.float32) * (rng.random(t.shape) < 0.5)
            z = (t == 0) & (rng.random(t.shape) < 0.125)
            a2 = np.where(z, 1.0, a2).astype(np.float32)
            a1 = (t.astype(np.float64) - a2).astype(np.float32)
            assert np.array_equal(a1 + a2, t)
        else:
            a1, a2 = t, None
    elif fam == "ints":
        assert kk * 16 < 2 ** 24
        wt = rng.integers(-4, 5, (cout, kk)).astype(np.float32)
        if c["a2"]:
            a1 = rng.integers(-2, 3, (n, h, w_, cin)).astype(np.float32)
            a2 = rng.integers(-2, 3, (n, h, w_, cin)).astype(np.float32)
        else:
            a1, a2 = rng.integers(-4, 5, (n, h, w_, cin)).astype(np.float32), None
    else:
        rs = 2.0 ** ((np.arange(n * h * w_) % 21) - 10.0)
        cs = 2.0 ** ((np.arange(cin) % 9) - 4.0)
        sc = (rs[:, None] * cs[None, :]).reshape(n, h, w_, cin)
        a1 = (rng.standard_normal((n, h, w_, cin)) * sc).astype(np.float32)
        a2 = (rng.standard_normal((n, h, w_, cin)) * sc).astype(np.float32) if c["a2"] else None
        wt = rng.standard_normal((cout, kk)).astype(np.float32)
        if c["a_rows"]:
            a1 = bf16_round(a1)
    t = a1 if a2 is None else a1 + a2  # fp32 sum, as the loader forms it
    r.update(a1=a1, a2=a2, w=wt)
    # ---- the operand model of the mode, in fp64
    acols = im2col(t, k, st, pad)
    if mode == "bf16":
        r["w_bits"] = bf16_bits(wt)
        wop = bf16_val(r["w_bits"]).astype(np.float64)
        aop = (acols if c["a_rows"] else bf16_round(acols)).astype(np.float64)
        acc = aop @ wop.T
        acc_true, s_a, s_w = acc, aop, wop
    else:
        aop, wop = acols.astype(np.float64), wt.astype(np.float64)
        acc_true, s_a, s_w = aop @ wop.T, aop, wop
        if mode == "fp32":
            acc = acc_true
        else:
            pa = [p.astype(np.float64) for p in planes_of(acols, mode)]
            pw = [p.astype(np.float64) for p in planes_of(wt, mode)]
            if mode == "x3":  # hi·(hi+mid+lo) + mid·(hi+mid) + lo·hi: the six kept products (the sums are exact)
                acc = pa[0] @ (pw[0] + pw[1] + pw[2]).T + pa[1] @ (pw[0] + pw[1]).T + pa[2] @ pw[0].T
            else:
                acc = pa[0] @ (pw[0] + pw[1]).T + pa[1] @ pw[0].T
    S = np.abs(s_a) @ np.abs(s_w).T
    knz = (s_a != 0).astype(np.float32) @ (s_w != 0).astype(np.float32).T
    r.update(acols=acols, S=S, knz=knz, acc=acc)
    # ---- epilogue operands
    exact = fam != "range"
    res_bf16 = lambda v: bf16_round(v.astype(np.float32))
    if c["affine"]:
        if exact:
            r["scale"] = _pick(rng, (1.0, 2.0, 0.5), cout)
            r["shift"] = (rng.integers(-2048, 2049, cout) / 1024.0).astype(np.float32)
        else:  # FrozenBN: gamma / sqrt(var + eps), beta - mean · that; a few channels pushed to ±20 and below -88
            r["scale"] = (rng.uniform(0.5, 1.5, cout) / np.sqrt(rng.uniform(0.25, 4.0, cout) + 1e-5)).astype(np.float32)
            r["shift"] = rng.standard_normal(cout).astype(np.float32)
            idx = np.arange(0, cout, 3)
            r["shift"][idx] = np.resize(np.float32([-100.0, 20.0, -20.0, -90.0]), len(idx))
    if c["row_period"]:
        p = c["row_period"]
        r["row_scale"] = _pick(rng, (0.25, 0.5, 1.0, 2.0), p) if exact else rng.uniform(0.5, 2.0, p).astype(np.float32)
    for key in ("r1", "r2"):
        kind = c["res1" if key == "r1" else "res2"]
        if kind:
            if exact:
                v = rng.integers(-128, 129, (m, cout)) / (32.0 if kind == "bf16" else 1024.0)
                if kind == "bf16":
                    assert np.array_equal(v.astype(np.float32), res_bf16(v))
            else:
                v = rng.standard_normal((m, cout)) * (1.0 + np.abs(acc_true).mean() * 0.01)
                v = res_bf16(v) if kind == "bf16" else v
            r[key] = v.astype(np.float32)
    # ---- the header's formula in fp64, step by step
    one = np.float64(1.0)
    rsv = r["row_scale"].astype(np.float64)[np.arange(m) % c["row_period"]][:, None] if c["row_period"] else one
    scv = r["scale"].astype(np.float64)[None, :] if c["affine"] else one
    shv = r["shift"].astype(np.float64)[None, :] if c["affine"] else 0.0
    r1v = r["r1"].astype(np.float64) if r["r1"] is not None else 0.0
    r2v = r["r2"].astype(np.float64) if r["r2"] is not None else 0.0

    def epilogue(a):
        t1 = a * rsv
        t2 = t1 * scv + shv
        t3 = t2 + r1v
        f = act64(t3, c["act"])
        return t1, t2, t3, f, f + r2v

    steps = epilogue(acc)
    r["ref"] = steps[-1]
    if exact:
        if fam == "probe":  # the conditions of the exactness argument, for this very case
            assert knz.max() <= 56, (cid, knz.max())
            assert S.max() < 64.0, (cid, S.max())
        assert c["act"] in (None, "relu")
        _exact32(acc, "accumulator", cid)
        for name, v in zip(("acc·row_scale", "·scale+shift", "+res1", "act", "+res2"), steps):
            _exact32(np.broadcast_to(v, acc.shape), name, cid)
        r["bound"] = np.zeros_like(acc)
    else:
        # the range reference is fp64 of the operands themselves (bf16: of the rounded operands the mode defines)
        t1, t2, t3, f, out = epilogue(acc_true)
        r["ref"] = out
        e_acc = C_MODE[mode] * (knz + splits) * U * S + (3.1 * 2.0 ** -16 * S if mode == "x2" else 0.0)
        e_pre = e_acc * np.abs(rsv * scv) + 4 * U * (np.abs(acc_true * rsv * scv) + np.abs(shv) + np.abs(r1v))
        slope, e_act = {None: (1.0, 0.0), "relu": (1.0, 0.0), "silu": (1.1, 8 * U * np.abs(f)),
                        "gelu": (1.13, 8 * U * np.abs(t3))}[c["act"]]
        r["bound"] = slope * e_pre + e_act + 2 * U * (np.abs(f) + np.abs(r2v)) + 2.0 ** -126
        assert np.isfinite(out).all() and np.isfinite(r["bound"]).all(), cid
    if c["c_bf16"]:
        if exact:
            r["ref_bits"] = bf16_bits(r["ref"].astype(np.float32))
        else:
            r["bound"] = r["bound"] + 2.0 ** -8 * (np.abs(r["ref"]) + r["bound"])
    return r


def compare(c, r, got, got_bits=None):
    """(failed?, worst err / bound or count of differing elements, message) of a kernel (or emulation) output
    `got` [M, Cout] (fp32 values; got_bits: the raw bf16 bits of a C_bf16 output)."""
    if c["fam"] != "range":
        if c["c_bf16"] and got_bits is not None:
            bad = got_bits != r["ref_bits"]
        else:
            bad = got.astype(np.float64) != r["ref"]  # NaN compares unequal: an unwritten element fails
        nb = int(bad.sum())
        return nb > 0, float(nb), f"{c['id']}: {nb} of {bad.size} elements differ from the exact reference"
    err = np.abs(got.astype(np.float64) - r["ref"])
    ratio = np.where(np.isfinite(err), err / r["bound"], np.inf)
    w = float(ratio.max())
    return not w <= 1.0, w, f"{c['id']}: worst err / bound {w:.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
