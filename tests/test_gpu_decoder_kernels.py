"""The kernels behind query selection, the decoder loop and post-processing (sp_msda, sp_topk_rows, sp_rowmax,
sp_gather_rows, sp_ref_init, sp_box_refine, sp_postprocess) against the fp64 references of tests/decoder_refs.py,
over the descriptors their C-ABI accepts: every MSDA kernel path and lane count, strided views on both sides,
samples on pixel centres / cell borders / far outside, the top-k reduction and tie paths, special values.

Index work is exact. The fp32 bars are measured, not chosen: each case computes on the CPU how far the fp32 numpy
oracle lies from the fp64 reference on the same inputs and allows the kernel 4× that (or the stated rounding
floor); both figures go to the parity-margins JSON (tests/margins.py). tests/test_decoder_refs.py validates the
references and the inputs' preconditions without a GPU.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_refs as refs  # noqa: E402
import margins  # noqa: E402

F32 = np.float32
FLT_MAX = refs.FLT_MAX
SP_TUNE_MSDA_GENERIC = 4


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def strided(dev, rows2d, ld=None, off=0, fill=np.nan):
    """rows2d [rows, cols] placed as rows of `ld` elements from element `off` of a flat device buffer whose other
    elements hold `fill`; returns the ops.V view."""
    from spotter_amd.ops import V

    rows, cols = rows2d.shape
    ld = cols if ld is None else ld
    buf = np.full(off + rows * ld, fill, rows2d.dtype)
    buf[off:].reshape(rows, ld)[:, :cols] = rows2d
    return V(T(buf, dev), off, ld)


def read_view(t, rows, cols, ld, off):
    """(the view's [rows, cols], every other element of the flat buffer) of a device tensor."""
    flat = t.cpu().numpy()
    inside = np.zeros(flat.shape, bool)
    for r in range(rows):
        inside[off + r * ld:off + r * ld + cols] = True
    return flat[inside].reshape(rows, cols), flat[~inside]


def last_error():
    from spotter_amd._lib import lib

    return lib().sp_last_error().decode(errors="replace")


# ----------------------------------------------------------------------------- sp_msda
def _msda_views(dev, case, exp, inp):
    """The case's operands in the layouts under test: value columns [8, 8 + C) of wider rows (odd stride for
    "odd_ld"), offset rows one float wider for "aw_pad", output columns [4, 4 + C) of rows of C + 8 pre-filled with
    NaN. Everything outside the views is NaN, so a read outside them shows in the output."""
    C = case.heads * case.head_dim
    R = case.B * case.Q
    ldv = C + 16 + (1 if case.layout == "odd_ld" else 0)
    if exp.bits is not None:
        value = strided(dev, np.pad(exp.bits, ((0, 0), (8, ldv - C - 8)), constant_values=np.int16(0x7FC0)), fill=0)
    else:
        value = strided(dev, np.pad(exp.value, ((0, 0), (8, ldv - C - 8)), constant_values=np.nan))
    off_aw = strided(dev, inp.off_aw, ld=inp.off_aw.shape[1] + (1 if case.layout == "aw_pad" else 0))
    from spotter_amd.ops import V

    out = V(torch.full((R * (C + 8),), float("nan"), device=dev), 4, C + 8)
    return value, 8, off_aw, out


@pytest.mark.parametrize("case,bf16", refs.MSDA_RUNS, ids=[f"{c.id}-{'bf16' if b else 'f32'}" for c, b in refs.MSDA_RUNS])
def test_msda_matches_fp64(dev, case, bf16):
    """sp_msda against the fp64 reference, per kernel path (the id's prefix: h8l = point-sharing kernel, vecN =
    per-lane kernel at N lanes per query, scalar = one thread per channel; tests/test_decoder_refs.py checks the
    mapping). Rows: a crafted block (pixel centres, cell borders, ix = −1 / −0.5 / W − 0.5 / W, map corners, far
    outside, ref_wh = 0, softmax edges) and a random block with about a third of the samples outside the map.
    Bar: max(4 × the fp32 oracle's error against fp64, (4·L·P + 8)·2⁻²⁴·max|value|), and never looser than
    rtol 1e-4 / atol 2e-5; far-outside rows are exactly 0; nothing outside the output view is written."""
    from spotter_amd import ops
    from spotter_amd._lib import lib

    inp = refs.msda_inputs(case)
    exp = refs.msda_expected(case, bf16)
    C, R = case.heads * case.head_dim, case.B * case.Q
    value, col, off_aw, out = _msda_views(dev, case, exp, inp)
    try:
        if case.generic:
            assert lib().sp_set_tuning(SP_TUNE_MSDA_GENERIC, 1) == 0
        ops.msda(value, col, off_aw, T(inp.ref, dev), out, case.B, inp.S, case.Q, case.heads, case.head_dim,
                 list(case.shapes), list(inp.starts), case.points, refs.OFFSET_SCALE)
    finally:
        lib().sp_set_tuning(SP_TUNE_MSDA_GENERIC, 0)
    got, outside = read_view(out.t, R, C, out.ld, out.off)
    assert np.isnan(outside).all(), "sp_msda wrote outside its output view"
    assert np.isfinite(got).all()
    scale = np.abs(exp.ref).max()
    err = float(np.abs(got - exp.ref).max())
    print(f"msda {case.id} bf16={bf16}: kernel err {err / scale:.3e}, fp32 oracle err {exp.oracle_err / scale:.3e}, "
          f"accumulation bound {exp.acc_bound / scale:.3e} (of max|ref| = {scale:.3f})")
    margins.record(f"msda/{case.id}/{'bf16' if bf16 else 'f32'}", kernel_err_vs_fp64=err / scale,
                   fp32_oracle_err_vs_fp64=exp.oracle_err / scale, bar=exp.bar / scale)
    assert err <= exp.bar, (err, exp.bar)
    np.testing.assert_allclose(got, exp.ref, rtol=1e-4, atol=2e-5)
    assert np.all(got[inp.far_rows] == 0)


def test_msda_argument_checks(dev):
    """Each descriptor the kernels' indexing does not cover is refused (< 0, with a message) before any launch:
    B or Q not positive, offset rows shorter than heads·L·P·3, output rows shorter than C, value rows shorter than
    value_col + C. The unmodified descriptor runs."""
    from spotter_amd._lib import SpMsdaDesc, lib

    heads, dh, P = 8, 32, 4
    shapes = [(2, 2), (1, 1)]
    B, Q, S, C, LP = 1, 3, 5, heads * dh, 2 * P
    value = torch.zeros(B * S * (C + 8), device=dev)
    off_aw = torch.zeros(B * Q * heads * LP * 3, device=dev)
    ref = torch.full((B * Q * 4,), 0.5, device=dev)
    out = torch.zeros(B * Q * C, device=dev)

    def desc(**kw):
        d = SpMsdaDesc()
        d.value, d.ld_value, d.value_col = value.data_ptr(), C + 8, 8
        d.off_aw, d.ld_off_aw = off_aw.data_ptr(), heads * LP * 3
        d.ref, d.out, d.ld_out = ref.data_ptr(), out.data_ptr(), C
        d.B, d.S, d.Q, d.heads, d.head_dim, d.levels, d.points = B, S, Q, heads, dh, 2, P
        for i, ((h, w), s0) in enumerate(zip(shapes, (0, 4))):
            d.level_h[i], d.level_w[i], d.level_start[i] = h, w, s0
        d.offset_scale = 0.5
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    assert L.sp_msda(ctypes.byref(desc()), stream) == 0, last_error()
    torch.cuda.synchronize()
    for kw in ({"B": 0}, {"Q": 0}, {"B": -1}, {"ld_off_aw": heads * LP * 3 - 1}, {"ld_out": C - 1},
               {"ld_value": C + 7}, {"value_col": -4}):
        assert L.sp_msda(ctypes.byref(desc(**kw)), stream) < 0, kw
        assert "sp_msda" in last_error(), (kw, last_error())


# ----------------------------------------------------------------------------- sp_topk_rows
ROWS = 3


def _run_topk(dev, x, n, k, reduce_c, ld=None, off=0, sigmoid=False, want_vals=True):
    """x [3, n·reduce_c] as rows of ld floats from element `off`, +FLT_MAX in the padding (never selectable
    unless the kernel reads outside its rows) → (idx [3, k], vals [3, k] or None)."""
    from spotter_amd import ops

    idx = torch.full((ROWS * k,), -1, dtype=torch.int32, device=dev)
    vals = torch.full((ROWS * k,), float("nan"), device=dev) if want_vals else None
    ops.topk_rows(strided(dev, x, ld=ld, off=off, fill=F32(FLT_MAX)), ROWS, n, k, idx, vals, reduce_c=reduce_c,
                  apply_sigmoid=sigmoid)
    return idx.cpu().numpy().reshape(ROWS, k), (vals.cpu().numpy().reshape(ROWS, k) if want_vals else None)


def _check_topk_exact(dev, x, n, k, reduce_c, **kw):
    red = x.reshape(ROWS, n, reduce_c).max(-1)
    exp = refs.topk_stable(red, k)
    idx, vals = _run_topk(dev, x, n, k, reduce_c, **kw)
    np.testing.assert_array_equal(idx, exp)
    if vals is not None:
        np.testing.assert_array_equal(vals, np.take_along_axis(red, exp, 1))


def _tied(rng, shape):
    return (np.round(rng.standard_normal(shape) * 8) / 8).astype(F32)  # multiples of 1/8: ties across the cut


@pytest.mark.parametrize("n,k,reduce_c,off,pad", [
    # the per-thread reduction loop: reduce_c % 4 != 0, or a base that is not 16-byte aligned
    (33, 20, 3, 0, 0), (1000, 300, 3, 0, 0), (33, 20, 91, 0, 0), (1000, 300, 91, 0, 0),
    (33, 20, 80, 1, 0), (1000, 300, 80, 1, 0),
    # ldx = n·reduce_c + 8 with +FLT_MAX in the padding, on every load path
    (1000, 300, 1, 0, 8), (1000, 300, 80, 0, 8), (33, 33, 3, 0, 8), (1000, 300, 4, 0, 8), (33, 20, 80, 1, 8)])
def test_topk_reduction_paths_and_padded_rows(dev, n, k, reduce_c, off, pad):
    rng = np.random.default_rng(refs.seed("topk", n, k, reduce_c, off, pad))
    x = _tied(rng, (ROWS, n * reduce_c))
    _check_topk_exact(dev, x, n, k, reduce_c, ld=n * reduce_c + pad, off=off)


@pytest.mark.parametrize("n,k,want_vals", [(500, 100, False), (1, 1, True), (5, 5, True), (64, 64, True),
                                           (512, 512, True), (512, 512, False)])
def test_topk_without_vals_and_k_equal_n(dev, n, k, want_vals):
    rng = np.random.default_rng(refs.seed("topk_misc", n, k))
    _check_topk_exact(dev, _tied(rng, (ROWS, n)), n, k, 1, want_vals=want_vals)


@pytest.mark.parametrize("reduce_c,off,saturated", [(1, 0, 0.02), (1, 1, 0.02), (80, 0, 0.002), (80, 1, 0.002)])
def test_topk_apply_sigmoid(dev, reduce_c, off, saturated):
    """apply_sigmoid on logits from the grid j/64 plus the saturated {20, 25, 30}: adjacent grid values lie ≥ 4665
    fp32 ulp apart after the sigmoid and the saturated ones are all exactly 1.0f (tests/test_decoder_refs.py), so the
    order is determined: stable argsort of −float32(sigmoid_fp64(x)); vals within 1e-7 of the fp64 sigmoid.
    reduce_c = 80 at offset 0 takes the float4 reduction, at offset 1 (and reduce_c = 1) the per-thread loop."""
    n, k = 1000, 300
    rng = np.random.default_rng(refs.seed("topk_sigmoid", reduce_c, off))
    x = refs.grid_logits(rng, (ROWS, n * reduce_c), saturated=saturated)
    red = x.reshape(ROWS, n, reduce_c).max(-1)
    exp = refs.sigmoid_order(red, k)
    assert ((red >= 20).sum(1) > 5).all() and ((red >= 20).sum(1) < k).all()  # the tie class at 1.0, and more below
    idx, vals = _run_topk(dev, x, n, k, reduce_c, off=off, sigmoid=True)
    np.testing.assert_array_equal(idx, exp)
    np.testing.assert_allclose(vals, np.take_along_axis(refs.sigmoid(red), exp, 1), rtol=0, atol=1e-7)


@pytest.mark.parametrize("reduce_c", [1, 4])
def test_topk_special_values(dev, reduce_c):
    """±inf, ±FLT_MAX, ±1e-40 denormals and signed zeros among ordinary values, an all-negative row and a row of one
    repeated value, through the per-thread loop (reduce_c 1) and the float4 reduction (4): exact order and values."""
    n, k = 200, 60
    x = refs.special_rows(n, reduce_c, np.random.default_rng(7 + reduce_c))
    _check_topk_exact(dev, x, n, k, reduce_c)
    _check_topk_exact(dev, x, n, n, reduce_c)


def test_topk_signed_zeros_tie_by_index(dev):
    """−0.0 == +0.0: a run of zeros of both signs across the cut comes back in index order (before the key was
    canonicalised the +0.0 entries were taken first)."""
    n, k = 100, 40
    x = refs.signed_zero_rows(n, k, np.random.default_rng(8))
    _check_topk_exact(dev, x, n, k, 1)


def test_topk_argument_checks(dev):
    from spotter_amd._lib import lib

    x = torch.zeros(16, device=dev)
    idx = torch.zeros(1024, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    L = lib()
    # (ldx, n, reduce_c, k): n above the 36,864 keys of LDS, k above 512, k > n, reduce_c = 0
    for ldx, n, reduce_c, k in ((36865, 36865, 1, 300), (1024, 1024, 1, 513), (8, 8, 1, 9), (8, 8, 0, 4)):
        rc = L.sp_topk_rows(x.data_ptr(), ldx, 1, n, reduce_c, 0, k, None, idx.data_ptr(), stream)
        assert rc < 0, (n, reduce_c, k)
        assert "sp_topk_rows" in last_error()


# ----------------------------------------------------------------------------- sp_rowmax
@pytest.mark.parametrize("rows", [1, 255, 257])
@pytest.mark.parametrize("c,ld,off", [(1, 1, 0), (1, 3, 1), (7, 9, 1), (12, 16, 1), (80, 80, 0), (80, 84, 0),
                                      (80, 84, 2)])
def test_rowmax_views_and_special_values(dev, rows, c, ld, off):
    """c = 1, ld > c on a misaligned base (the scalar kernel even where c % 4 == 0), the float4 kernel on padded
    rows, rows around one 256-thread block; −inf and ±FLT_MAX among the values, a row of only −inf; exact."""
    from spotter_amd import ops

    rng = np.random.default_rng(refs.seed("rowmax", rows, c, ld, off))
    x = rng.standard_normal((rows, c)).astype(F32)
    sp = np.array([-np.inf, FLT_MAX, -FLT_MAX], F32)
    pos = rng.permutation(rows * c)[:max(1, rows * c // 5)]
    x.reshape(-1)[pos] = sp[np.arange(len(pos)) % 3]
    x[rows // 2] = -np.inf
    out = torch.full((rows + 1,), float("nan"), device=dev)
    ops.rowmax(strided(dev, x, ld=ld, off=off, fill=F32(FLT_MAX)), rows, c, out)
    got = out.cpu().numpy()
    np.testing.assert_array_equal(got[:rows], x.max(1))
    assert np.isnan(got[rows])


# ----------------------------------------------------------------------------- sp_gather_rows / sp_ref_init / sp_box_refine
@pytest.mark.parametrize("d", [1, 4, 257])
def test_gather_rows_batched_views(dev, d):
    """batch 3 (each image's indices address its own src_rows), source and destination as column slices of wider
    buffers, indices 0, src_rows − 1 and repeats: exact, and nothing outside the destination view is written."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    batch, src_rows, k = 3, 50, 7
    rng = np.random.default_rng(refs.seed("gather", d))
    src = rng.standard_normal((batch * src_rows, d)).astype(F32)
    idx = rng.integers(0, src_rows, (batch, k)).astype(np.int32)
    idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3] = 0, src_rows - 1, idx[:, 4], src_rows - 1
    dst = V(torch.full((batch * k * (d + 3),), float("nan"), device=dev), 2, d + 3)
    ops.gather_rows(strided(dev, src, ld=d + 5, off=3), src_rows, T(idx, dev), k, batch, d, dst)
    got, outside = read_view(dst.t, batch * k, d, dst.ld, dst.off)
    exp = src.reshape(batch, src_rows, d)[np.arange(batch)[:, None], idx].reshape(batch * k, d)
    np.testing.assert_array_equal(got, exp)
    assert np.isnan(outside).all()


def _sigmoid_bar(name, got, ref64, restated32):
    """The two sigmoid kernels' bar: 4 × the error of the fp32 numpy restatement against fp64 on the same inputs,
    and never less than 2⁻²³ (one ulp of an output near 1)."""
    err = float(np.abs(got - ref64).max())
    err32 = float(np.abs(restated32.astype(np.float64) - ref64).max())
    bar = max(4.0 * err32, 2.0 ** -23)
    print(f"{name}: kernel err {err:.3e}, fp32 restatement err {err32:.3e}, bar {bar:.3e}")
    margins.record(name, kernel_err_vs_fp64=err, fp32_oracle_err_vs_fp64=err32, bar=bar)
    assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("ld_delta", [4, 12])
def test_ref_init_matches_fp64(dev, ld_delta):
    """ref = sigmoid(delta + anchors[idx]) (M2:1599-1613) with anchors from oracle.rtdetr_np.anchors_for: rows
    invalidated to FLT_MAX are selected (sigmoid(FLT_MAX + δ) is exactly 1), deltas include 0, ±20, ±100."""
    from spotter_amd import ops

    batch, k = 2, 37
    anchors, valid, idx, delta = refs.ref_init_inputs(batch, k, np.random.default_rng(9))
    ref = torch.full((batch * k * 4 + 4,), float("nan"), device=dev)
    ops.ref_init(strided(dev, delta, ld=ld_delta), T(anchors, dev), T(idx, dev), batch, k, ref)
    got = ref.cpu().numpy()
    assert np.isnan(got[batch * k * 4:]).all()
    got = got[:batch * k * 4].reshape(batch * k, 4)
    a = anchors[idx.reshape(-1)]
    ref64 = refs.sigmoid(refs.f64(delta) + refs.f64(a))
    _sigmoid_bar(f"ref_init/ld{ld_delta}", got, ref64, refs.sigmoid32(delta + a))
    assert np.all(got[~valid[idx.reshape(-1)]] == 1.0)


@pytest.mark.parametrize("ld_delta", [4, 8])
def test_box_refine_matches_fp64(dev, ld_delta):
    """ref ← sigmoid(delta + inverse_sigmoid(ref)) (M2:1689-1693), twice in place as the decoder chains it; each
    application is judged from the values it read (the second from the kernel's own first result). ref holds
    exactly 0, 1, 1e-5, 1 − 1e-5, 5e-6, values just outside [0, 1] and interior values; deltas include 0, ±15."""
    from oracle.rtdetr_np import inverse_sigmoid
    from spotter_amd import ops

    rows = 300
    ref0, deltas = refs.box_refine_inputs(rows, np.random.default_rng(4))
    ref = T(np.concatenate([ref0.reshape(-1), np.full(4, np.nan, F32)]), dev)
    cur = ref0
    for step, delta in enumerate(deltas):
        ops.box_refine(strided(dev, delta, ld=ld_delta), ref, rows)
        got = ref.cpu().numpy()
        assert np.isnan(got[rows * 4:]).all()
        got = got[:rows * 4].reshape(rows, 4)
        ref64 = refs.sigmoid(refs.f64(delta) + refs.inverse_sigmoid(cur))
        _sigmoid_bar(f"box_refine/ld{ld_delta}/pass{step + 1}", got, ref64, refs.sigmoid32(delta + inverse_sigmoid(cur)))
        cur = got


# ----------------------------------------------------------------------------- sp_postprocess
@pytest.mark.parametrize("q,c,k", [(300, 91, 300), (300, 80, 100), (7, 3, 21), (50, 80, 512), (100, 1, 100)])
def test_postprocess_matches_fp64(dev, q, c, k):
    """All k entries per image (scores, labels, boxes, counts), on grid logits whose order is determined
    (test_topk_apply_sigmoid): an image whose top k straddle score == 0.5 exactly (not kept at threshold 0.5: HF
    keeps score > threshold), a saturated image (more than k scores of 1.0f: the k lowest flat indices win),
    thresholds 0.5, 1.0 (nothing kept) and 0.0 (all k kept), target sizes from (1, 3000) to (4320, 7680)."""
    from spotter_amd import ops

    rng = np.random.default_rng(refs.seed("postprocess", q, c, k))
    logits, boxes = refs.postprocess_inputs(q, c, k, rng)
    ts = refs.TARGET_SIZES
    B = len(ts)
    d_logits, d_boxes, d_ts = T(logits, dev), T(boxes, dev), T(ts, dev)
    for thr in (0.5, 1.0, 0.0):
        sc = torch.full((B * k,), float("nan"), device=dev)
        lb = torch.full((B * k,), -1, dtype=torch.int64, device=dev)
        bx = torch.full((B * k * 4,), float("nan"), device=dev)
        cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
        work = torch.full((B * k,), -1, dtype=torch.int32, device=dev)
        ops.postprocess(d_logits, d_boxes, d_ts, k, thr, sc, lb, bx, cnt, work)
        exp = refs.postprocess(logits, boxes, ts, k, thr)
        np.testing.assert_array_equal(work.cpu().numpy().reshape(B, k), exp["idx"])
        np.testing.assert_array_equal(lb.cpu().numpy().reshape(B, k), exp["labels"])
        np.testing.assert_allclose(sc.cpu().numpy().reshape(B, k), exp["scores"], rtol=0, atol=1e-7)
        np.testing.assert_allclose(bx.cpu().numpy().reshape(B, k, 4), exp["boxes"], rtol=1e-6, atol=1e-4)
        np.testing.assert_array_equal(cnt.cpu().numpy(), exp["counts"])
    # (the reference's counts at 0.5 exclude the k // 3 scores that equal it: tests/test_decoder_refs.py)


def test_postprocess_refuses_more_keys_than_lds_holds(dev):
    """Q·C = 300·128 = 38,400 keys exceed the 36,864 of the top-k's LDS: < 0 before any launch, counts untouched."""
    from spotter_amd._lib import lib

    B, q, c, k = 1, 300, 128, 300
    logits = torch.zeros(B * q * c, device=dev)
    boxes = torch.zeros(B * q * 4, device=dev)
    ts = T(np.array([[640, 640]], np.int32), dev)
    sc = torch.zeros(B * k, device=dev)
    lb = torch.zeros(B * k, dtype=torch.int64, device=dev)
    bx = torch.zeros(B * k * 4, device=dev)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=dev)
    work = torch.zeros(B * k, dtype=torch.int32, device=dev)
    rc = lib().sp_postprocess(logits.data_ptr(), boxes.data_ptr(), ts.data_ptr(), B, q, c, k, 0.5, sc.data_ptr(),
                              lb.data_ptr(), bx.data_ptr(), cnt.data_ptr(), work.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    assert rc < 0
    assert "sp_topk_rows" in last_error()
    torch.cuda.synchronize()
    assert cnt.cpu().numpy().tolist() == [-7]
