"""Host-side checks of the TF32-class tier (SP_PREC_F32X2, precision "fp32-x2"): the two-plane weight split, the
planner's choices for two planes against the 3-way split's, the argument checks and the public precision name.
No GPU."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SP_PREC_BF16, SP_PREC_F32X3, SP_PREC_F32X2 = 1, 2, 3
SP_CONV_GLDS = 2  # sp_conv_family (include/spotter_hip.h), read back below


def _f32(bits):
    return (np.asarray(bits).view(np.uint16).astype(np.uint32) << 16).view(np.float32)


def test_split_bf16x2_host_planes_and_residual():
    """hi = RNE(w), lo = RNE(w - hi) as bf16 bit patterns, over fp32 values from the subnormal range to the
    largest binades. The residual bound |w - hi - lo| <= 2^-16 |w| is derived for bf16 planes with their 8-bit
    significand: it is asserted for every |w| >= 2^-118, where it is at least half the spacing of the bf16
    subnormals (2^-134) and so holds whether lo is normal or not. Below that lo is a bf16 subnormal whose spacing
    no longer shrinks with |w|, and the same RNE statement reads |w - hi - lo| <= 2^-134, asserted instead."""
    from spotter_amd.ops import bf16_bits, split_bf16x2_host

    rng = np.random.default_rng(19)
    parts = [rng.standard_normal(4096).astype(np.float32)]
    # every binade from the smallest subnormal to just under overflow of the bf16 rounding, both signs
    e = rng.integers(-149, 127, size=8192)
    m = rng.uniform(1.0, 2.0, size=8192) * rng.choice([-1.0, 1.0], size=8192)
    parts.append(np.ldexp(m, e).astype(np.float32))
    parts.append(np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 2.0 ** -149, -2.0 ** -140, 1e38, -3e38, 257.0 / 256,
                           1 + 2.0 ** -9, 1 + 2.0 ** -8 + 2.0 ** -17], np.float32))
    w = np.concatenate(parts)
    w = w[np.isfinite(_f32(bf16_bits(w)))]  # RNE of the top half-binade overflows to inf: not a weight
    planes = split_bf16x2_host(w)
    assert planes.dtype == np.int16 and planes.shape == (2, w.size)
    hi, lo = planes.view(np.uint16)
    assert np.array_equal(hi, bf16_bits(w))
    assert np.array_equal(lo, bf16_bits(w - _f32(hi)))
    w64 = w.astype(np.float64)
    resid = np.abs(w64 - _f32(hi).astype(np.float64) - _f32(lo).astype(np.float64))
    big = np.abs(w64) >= 2.0 ** -118
    assert (~big).sum() > 100 and (np.abs(w64) < 2.0 ** -126).any() and (np.abs(w64) > 1e30).any()
    assert (resid[big] <= 2.0 ** -16 * np.abs(w64[big])).all()
    assert (resid[~big] <= 2.0 ** -134).all()
    # the planes keep what one bf16 plane drops: on the unit-scale values the residual is >= 100x smaller
    u = slice(0, 4096)
    one = np.abs(w64[u] - _f32(hi[u]).astype(np.float64))
    assert resid[u].max() * 100 < one.max()


def _desc(prec, *, n=1, h=8, w=8, cin=32, cout=64, k=1, stride=1, pad=0, planes_stride=None, **kw):
    from spotter_amd import _lib

    ho = (h + 2 * pad - k) // stride + 1
    wo = (w + 2 * pad - k) // stride + 1
    f = dict(A=1 << 20, lda=cin, N=n, H=h, W=w, Cin=cin, KH=k, KW=k, stride=stride, pad=pad, Ho=ho, Wo=wo,
             Wt=2 << 20, Cout=cout, C=3 << 20, ldc=cout, precision=prec, Wt_bf16=4 << 20,
             wt_plane_stride=cout * k * k * cin if planes_stride is None else planes_stride)
    f.update(kw)
    return _lib.SpConvDesc(**f)


def _plan(desc, cfg=-1):
    from spotter_amd import _lib

    L = _lib.load()
    L.sp_set_conv_config(cfg)
    try:
        info = _lib.SpConvPlanInfo()
        rc = L.sp_conv_plan(C.byref(desc), C.byref(info))
        return {f: getattr(info, f) for f, _ in info._fields_} if rc == 0 else L.sp_last_error().decode()
    finally:
        L.sp_set_conv_config(-1)


def _x2_ids():
    src = open(os.path.join(ROOT, "spotter_amd", "csrc", "conv_plan.h")).read()
    (body,) = re.findall(r"constexpr int kGldsX2Ids\[\] = \{([^}]*)\};", src)
    return {int(v) for v in body.split(",")}


# (name, descriptor keywords, forced id): the by-shape choice and forced ids built for two planes
PLAN_CASES = [
    ("1x1 fast path", dict(n=32, h=40, w=40, cin=256, cout=512), -1),
    ("1x1 narrow output", dict(cin=32, cout=4), -1),
    ("1x1 table shape 51200x1024x256", dict(n=32, h=40, w=40, cin=256, cout=1024), -1),
    ("3x3 stride 2", dict(n=8, h=80, w=80, cin=128, cout=128, k=3, stride=2, pad=1), -1),
    ("3x3 stride 1, 256-wide", dict(n=32, h=40, w=40, cin=256, cout=256, k=3, pad=1), -1),
    ("Cin 24 generic", dict(h=12, w=12, cin=24, cout=64, k=3, pad=1), -1),
    ("A2 addend", dict(n=32, h=1, w=300, cin=256, cout=512, A2=5 << 20, lda2=256), -1),
    ("A2 addend, forced LDS-DMA id", dict(n=32, h=1, w=300, cin=256, cout=512, A2=5 << 20, lda2=256), 45),
    ("split-K with a workspace", dict(h=10, w=10, cin=256, cout=256, k=3, pad=1, workspace=6 << 20,
                                      workspace_elems=1 << 24), -1),
    ("split-K with counters", dict(h=10, w=10, cin=256, cout=256, k=3, pad=1, workspace=6 << 20,
                                   workspace_elems=1 << 24, splitk_counters=7 << 20, splitk_counters_len=4096), -1),
    ("slab-eligible expand with res1", dict(n=32, h=40, w=40, cin=256, cout=1024, scale=8 << 20, shift=9 << 20,
                                           res1=10 << 20, ldr1=1024, act=1), -1),
    ("by-shape tile with the slab epilogue", dict(n=32, h=40, w=40, cin=256, cout=512, scale=8 << 20, shift=9 << 20,
                                                  res1=10 << 20, ldr1=512, act=1), -1),
    ("forced 16x16x32 tile", dict(n=32, h=40, w=40, cin=256, cout=512), 41),
    ("forced k16 tile", dict(n=32, h=40, w=40, cin=256, cout=512), 46),
    ("forced slab form", dict(n=32, h=40, w=40, cin=256, cout=512, scale=8 << 20, shift=9 << 20), 145),
    ("forced direct-store form", dict(n=32, h=40, w=40, cin=256, cout=512, res1=10 << 20, ldr1=512), 245),
    ("forced register-staged id", dict(n=32, h=40, w=40, cin=256, cout=512), 1),
]


@pytest.mark.parametrize("name,kw,cfg", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_two_plane_plan_equals_the_three_plane_plan(name, kw, cfg):
    """With SP_PREC_F32X2 the planner reports planes == 2 and otherwise takes every choice it takes for
    SP_PREC_F32X3 on the same descriptor: family, tile, generic, fast path, epilogue, splits, counters."""
    p3 = _plan(_desc(SP_PREC_F32X3, **kw), cfg)
    p2 = _plan(_desc(SP_PREC_F32X2, **kw), cfg)
    assert isinstance(p3, dict) and isinstance(p2, dict), (p3, p2)
    assert p3["planes"] == 3 and p2["planes"] == 2
    assert {k: v for k, v in p2.items() if k != "planes"} == {k: v for k, v in p3.items() if k != "planes"}
    if p2["family"] == SP_CONV_GLDS:
        assert p2["tile"] in _x2_ids()


def test_the_cases_reach_the_paths_they_name():
    """The plan cases above are worth their names: fast path, generic gather, split-K (both combines), the slab and
    direct-store epilogues and a register-staged tile all occur."""
    got = {name: _plan(_desc(SP_PREC_F32X2, **kw), cfg) for name, kw, cfg in PLAN_CASES}
    assert got["1x1 fast path"]["family"] == SP_CONV_GLDS and got["1x1 fast path"]["fast_1x1"] == 1
    assert got["3x3 stride 2"]["family"] == SP_CONV_GLDS and got["3x3 stride 2"]["fast_1x1"] == 0
    assert got["Cin 24 generic"]["generic"] == 1 and got["Cin 24 generic"]["family"] != SP_CONV_GLDS
    assert got["A2 addend"]["family"] != SP_CONV_GLDS and got["A2 addend, forced LDS-DMA id"]["family"] != SP_CONV_GLDS
    assert got["split-K with a workspace"]["splits"] > 1 and got["split-K with a workspace"]["counters"] == 0
    assert got["split-K with counters"]["splits"] > 1 and got["split-K with counters"]["counters"] == 1
    # the stage-3 expand: tile_table.h's split-operand entry is 245, the slab epilogue's direct-store form
    assert got["slab-eligible expand with res1"]["tile"] == 45 and got["slab-eligible expand with res1"]["epilogue"] == 4
    assert got["by-shape tile with the slab epilogue"]["epilogue"] == 2
    assert got["1x1 table shape 51200x1024x256"]["tile"] == 45  # tile_table.h's split-operand entry (245)
    assert got["forced 16x16x32 tile"]["tile"] == 41 and got["forced k16 tile"]["tile"] == 46
    assert got["forced slab form"]["tile"] == 45 and got["forced slab form"]["epilogue"] == 2
    assert got["forced direct-store form"]["tile"] == 45 and got["forced direct-store form"]["epilogue"] == 4
    assert got["forced register-staged id"]["tile"] == 1 and got["forced register-staged id"]["family"] != SP_CONV_GLDS


@pytest.mark.parametrize("cfg", [11, 15, 111, 220, 38])
def test_forced_id_outside_the_two_plane_set_falls_back_by_shape(cfg):
    """An LDS-DMA tile that is not compiled for two planes (outside kGldsX2Ids) is no id with SP_PREC_F32X2: the
    plan is the by-shape plan, while the 3-way split honours the id."""
    kw = dict(n=32, h=40, w=40, cin=256, cout=512)
    assert cfg % 100 not in _x2_ids()
    by_shape = _plan(_desc(SP_PREC_F32X2, **kw), -1)
    p2 = _plan(_desc(SP_PREC_F32X2, **kw), cfg)
    p3 = _plan(_desc(SP_PREC_F32X3, **kw), cfg)
    assert p2 == by_shape and p2["tile"] in _x2_ids()
    assert p3["tile"] == cfg % 100


def test_bad_arguments_fail_with_the_split_modes_messages():
    """One-plane stride, missing Wt_bf16 and bf16 output rows: the same error text for two planes as for three."""
    bad = [dict(planes_stride=64 * 32 - 8), dict(Wt_bf16=None), dict(C=None, C_bf16=3 << 20),
           dict(res1_bf16=10 << 20, ldr1=64)]
    for kw in bad:
        e3 = _plan(_desc(SP_PREC_F32X3, **kw))
        e2 = _plan(_desc(SP_PREC_F32X2, **kw))
        assert isinstance(e3, str) and e2 == e3, (kw, e2, e3)
    assert "wt_plane_stride" in _plan(_desc(SP_PREC_F32X2, planes_stride=64 * 32 - 8))
    assert "needs Wt_bf16" in _plan(_desc(SP_PREC_F32X2, Wt_bf16=None))
    assert "bf16 operand mode" in _plan(_desc(SP_PREC_F32X2, C=None, C_bf16=3 << 20))
    assert "precision 4" in _plan(_desc(4))


def test_header_and_binding_agree_on_the_new_precision():
    from spotter_amd import _lib, ops

    hdr = open(os.path.join(ROOT, "include", "spotter_hip.h")).read()
    assert re.search(r"SP_PREC_F32X2\s*=\s*3\b", hdr) and re.search(r"#define SP_ABI_VERSION 20\b", hdr)
    assert re.search(r"SP_CONV_GLDS\s*=\s*%d\b" % SP_CONV_GLDS, hdr)
    assert _lib.ABI_VERSION == 20 and _lib.load().sp_abi_version() == 20
    assert ops.PREC_BY_PLANES == {1: SP_PREC_BF16, 3: SP_PREC_F32X3, 2: SP_PREC_F32X2}
    assert ops.PREC_TAG[SP_PREC_F32X2] == "x2"


def test_precision_name_is_public_and_pickles():
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRECISIONS, check_precision

    assert check_precision("fp32-x2") == "fp32-x2" and PRECISIONS["fp32-x2"] == ("x2", "x2")
    m = SpotterForObjectDetection.from_pretrained("synthetic:r18vd", precision="fp32-x2")
    assert m.precision == "fp32-x2" and m._engine is None
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.precision == "fp32-x2" and m2._engine is None and m2.cfg.name == "r18vd"
