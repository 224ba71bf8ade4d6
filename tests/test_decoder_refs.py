"""The fp64 references of tests/decoder_refs.py against independent implementations, on the CPU: oracle/rtdetr_np.py
(the fp32 numpy restatement the golden parity rests on) and torch float64, on the edge inputs the GPU tests of
tests/test_gpu_decoder_kernels.py use. Also the preconditions those GPU tests state about their inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decoder_refs as refs  # noqa: E402

torch = pytest.importorskip("torch")

F32 = np.float32
SHAPE_CASES = [c for c in refs.MSDA_CASES if c.layout == "aligned" and not c.generic]  # one per distinct input set


def _msda_torch64(value, off_aw, ref, case):
    """The HF formulation (M2:44-115, 200-215) on torch float64: F.grid_sample on 2·loc − 1."""
    import torch.nn.functional as Fn

    B, Q, nH, dh, P = case.B, case.Q, case.heads, case.head_dim, case.points
    shapes = case.shapes
    LP = len(shapes) * P
    v = torch.from_numpy(np.asarray(value, np.float64)).reshape(B, -1, nH, dh)
    oa = torch.from_numpy(np.asarray(off_aw, np.float64))
    off = oa[:, :nH * LP * 2].reshape(B, Q, nH, LP, 2)
    aw = torch.softmax(oa[:, nH * LP * 2:].reshape(B, Q, nH, LP), -1)
    r = torch.from_numpy(np.asarray(ref, np.float64)).reshape(B, Q, 4)
    loc = r[:, :, None, None, :2] + off * (1.0 / P) * r[:, :, None, None, 2:] * refs.OFFSET_SCALE
    grids = 2 * loc - 1
    vals = v.split([h * w for h, w in shapes], dim=1)
    sampled = []
    for l, (h, w) in enumerate(shapes):
        vl = vals[l].flatten(2).transpose(1, 2).reshape(B * nH, dh, h, w)
        g = grids[:, :, :, l * P:(l + 1) * P].transpose(1, 2).flatten(0, 1)  # [B·nH, Q, P, 2]
        sampled.append(Fn.grid_sample(vl, g, mode="bilinear", padding_mode="zeros", align_corners=False))
    s = torch.cat(sampled, -1)  # [B·nH, dh, Q, L·P]
    a = aw.transpose(1, 2).reshape(B * nH, 1, Q, LP)
    out = (s * a).sum(-1).view(B, nH * dh, Q).transpose(1, 2)
    return out.reshape(B * Q, nH * dh).numpy()


@pytest.mark.parametrize("case", SHAPE_CASES, ids=lambda c: c.id)
def test_msda_reference_matches_torch_float64_and_oracle(case):
    inp = refs.msda_inputs(case)
    exp = refs.msda_expected(case, False)
    scale = np.abs(exp.ref).max()
    t64 = _msda_torch64(inp.value, inp.off_aw, inp.ref, case)
    assert np.abs(t64 - exp.ref).max() <= 1e-12 * scale
    # the fp32 oracle agrees to fp32 rounding; the far-outside rows are exactly 0 in all three
    assert exp.oracle_err <= 1e-5 * scale, exp.oracle_err / scale
    if case.B * case.Q >= 74:
        assert len(inp.far_rows) == 5
        assert np.all(exp.ref[inp.far_rows] == 0) and np.all(t64[inp.far_rows] == 0)
        o32 = refs.msda_oracle32(inp.value, inp.off_aw, inp.ref, case.B, case.Q, case.heads, case.head_dim,
                                 case.shapes, case.points, refs.OFFSET_SCALE)
        assert np.all(o32[inp.far_rows] == 0)
        assert 0.22 <= refs.outside_fraction(case) <= 0.45, refs.outside_fraction(case)  # roughly a third
    # the bar the GPU test derives from these figures is never looser than the old test's rtol 1e-4 / atol 2e-5
    # at the scale of the outputs
    assert exp.bar <= 1e-4 * scale + 2e-5, (exp.bar, scale)
    assert np.isfinite(exp.ref).all() and scale > 0.1


def test_msda_bf16_reference_uses_the_rounded_values():
    case = refs.MSDA_CASES[0]
    exp = refs.msda_expected(case, True)
    assert exp.bits.dtype == np.int16
    back = (exp.bits.view(np.uint16).astype(np.uint32) << 16).view(F32)
    assert np.array_equal(back, exp.value)
    assert np.abs(exp.value - refs.msda_inputs(case).value).max() <= 2.0 ** -8 * np.abs(exp.value).max()
    t64 = _msda_torch64(exp.value, refs.msda_inputs(case).off_aw, refs.msda_inputs(case).ref, case)
    assert np.abs(t64 - exp.ref).max() <= 1e-12 * np.abs(exp.ref).max()


def test_msda_cases_reach_every_kernel_path():
    """The dispatch conditions of sp_msda restated: which kernel each case's descriptor selects."""
    def path(c):
        C = c.heads * c.head_dim
        vec = c.head_dim % 4 == 0 and 256 % (C // 4) == 0 and c.layout != "odd_ld"
        h8 = (vec and C == 256 and c.head_dim == 32 and c.levels == 3 and c.points == 4 and not c.generic
              and c.layout != "aw_pad")
        return "h8l" if h8 else (f"vec{C // 4}" if vec else "scalar")

    for c in refs.MSDA_CASES:
        assert c.id.startswith(path(c)), (c.id, path(c))
        assert (c.heads * c.head_dim) % 64 == 0 and c.heads * c.head_dim <= 1024
    assert {path(c) for c in refs.MSDA_CASES} == {"h8l", "vec16", "vec32", "vec64", "vec128", "vec256", "scalar"}
    assert {c.heads * c.head_dim for c in refs.MSDA_CASES if path(c) == "scalar"} >= {192, 256, 320, 768}


def test_grid_sample_edges_match_torch_and_oracle():
    """Pixel centres, cell borders, ix = −1 / −0.5 / W − 0.5 / W and far outside, on one map."""
    from oracle.rtdetr_np import grid_sample_bilinear
    import torch.nn.functional as Fn

    rng = np.random.default_rng(3)
    h, w, d = 8, 4, 5
    value = rng.standard_normal((2, h, w, d)).astype(F32)
    xs = refs._axis_specials(w) + [1e6, -1e6, 2.5e8, -2.5e8]
    ys = refs._axis_specials(h) + [1e6, -1e6]
    loc = np.array([[x, y] for x in xs for y in ys], F32)[None].repeat(2, 0)  # [2, M, 2]
    got = refs.grid_sample(value, loc)
    t = Fn.grid_sample(torch.from_numpy(value.astype(np.float64)).permute(0, 3, 1, 2),
                       torch.from_numpy(2 * loc.astype(np.float64) - 1)[:, :, None, :], mode="bilinear",
                       padding_mode="zeros", align_corners=False)[..., 0].permute(0, 2, 1).numpy()
    assert np.abs(got - t).max() <= 1e-13
    o = grid_sample_bilinear(value, loc[:, :, None, :])[:, :, 0]
    assert np.abs(got - o).max() <= 2e-6
    # a pixel centre returns that pixel; a location a whole pixel outside returns 0
    c = refs.grid_sample(value, np.array([[[(2 + 0.5) / w, (5 + 0.5) / h], [-0.5 / w, 0.3], [0.3, (h + 0.5) / h]]] * 2))
    assert np.array_equal(c[:, 0], value[:, 5, 2].astype(np.float64))
    assert np.all(c[:, 1:] == 0)


def test_sigmoid_and_inverse_sigmoid_match_oracle_and_torch():
    from oracle.rtdetr_np import inverse_sigmoid, sigmoid

    rng = np.random.default_rng(4)
    ref, deltas = refs.box_refine_inputs(300, rng)
    inv = refs.inverse_sigmoid(ref)
    assert np.abs(inv - inverse_sigmoid(ref)).max() <= 2e-6  # one fp32 ulp of |log(1e-5)| = 11.5 is 9.5e-7
    x = torch.from_numpy(ref.astype(np.float64)).clamp(0, 1)
    t = torch.log(x.clamp(min=refs.EPS32) / (1 - x).clamp(min=refs.EPS32)).numpy()
    assert np.abs(inv - t).max() <= 1e-14
    # the clips: 0 and below give log(1e-5f / 1), 1 and above log(1 / 1e-5f), and nothing lies outside them
    lo, hi = np.log(refs.EPS32 / 1.0), np.log(1.0 / refs.EPS32)
    flat, iflat = ref.reshape(-1), inv.reshape(-1)
    assert np.all(iflat[flat <= 0] == lo) and np.all(iflat[flat >= 1] == hi)
    assert np.all(iflat[flat == F32(5e-6)] == np.log(refs.EPS32 / (1.0 - float(F32(5e-6)))))  # below the clip
    assert np.all((iflat >= lo) & (iflat <= hi))
    logits = np.concatenate([refs.GRID, refs.SATURATED, [-100.0, -87.0, 100.0, 0.0, refs.FLT_MAX]])
    s = refs.sigmoid(logits)
    assert np.abs(s - torch.sigmoid(torch.from_numpy(logits)).numpy()).max() <= 1e-15
    assert np.abs(s - refs.sigmoid32(logits)).max() <= 1.2e-7
    assert np.abs(s[:len(refs.GRID)] - sigmoid(refs.GRID.astype(F32))).max() <= 1.2e-7
    assert s[-1] == 1.0 and s[-2] == 0.5


def test_sigmoid_grid_preconditions():
    """What the apply_sigmoid top-k and post-process cases rest on: adjacent grid logits give fp32 sigmoids at
    least 4665 ulp apart (so any fp32 sigmoid within a few ulp orders them the same way), and every logit
    ≥ 17.4 is exactly 1.0f whether evaluated in fp32 or in fp64 and rounded."""
    s32 = refs.sigmoid(refs.GRID).astype(F32)
    gaps = refs.ulp_gaps32(s32)
    assert gaps.min() >= 4665, gaps.min()
    sat = np.concatenate([[17.4], refs.SATURATED])
    assert np.all(refs.sigmoid(sat).astype(F32) == F32(1.0))
    assert np.all(refs.sigmoid32(sat) == F32(1.0))
    assert not ((refs.GRID > 16) | (refs.GRID < -87)).any()  # where fp32 implementations may differ
    # the fp32 numpy sigmoid orders the grid + saturated logits exactly as the reference order says
    rng = np.random.default_rng(6)
    x = refs.grid_logits(rng, (3, 4000), saturated=0.02, zeros=0.01)
    assert set(np.unique(x[x >= 17])) == {20.0, 25.0, 30.0}
    exp = refs.sigmoid_order(x, 300)
    got = np.argsort(-refs.sigmoid32(x), axis=-1, kind="stable")[:, :300]
    assert np.array_equal(exp, got)
    tv = torch.topk(torch.from_numpy(refs.sigmoid(x).astype(F32)), 300, dim=-1).values.numpy()
    assert np.array_equal(tv, np.take_along_axis(refs.sigmoid(x).astype(F32), exp, 1))


@pytest.mark.parametrize("reduce_c", [1, 4])
def test_topk_reference_on_special_values(reduce_c):
    from oracle.rtdetr_np import topk_desc

    rng = np.random.default_rng(7 + reduce_c)
    n, k = 200, 60
    x = refs.special_rows(n, reduce_c, rng)
    red = x.reshape(3, n, reduce_c).max(-1)
    exp = refs.topk_stable(red, k)
    assert np.array_equal(exp, topk_desc(red, k))
    tv = torch.topk(torch.from_numpy(red), k, dim=-1).values.numpy()
    assert np.array_equal(tv, np.take_along_axis(red, exp, 1))
    assert np.isinf(red[0]).any() and (np.abs(red[0]) == F32(1e-40)).any() and (red[1] < 0).all()
    assert np.array_equal(exp[2], np.arange(k))  # one repeated value: index order
    full = refs.topk_stable(red, n)  # k == n is a permutation
    assert np.array_equal(np.sort(full, -1), np.broadcast_to(np.arange(n), (3, n)))


def test_topk_reference_orders_signed_zeros_by_index():
    from oracle.rtdetr_np import topk_desc

    rng = np.random.default_rng(8)
    n, k = 100, 40
    x = refs.signed_zero_rows(n, k, rng)
    exp = refs.topk_stable(x, k)
    assert np.array_equal(exp, topk_desc(x, k))
    for r in range(3):
        zeros = np.flatnonzero(x[r] == 0)
        taken = exp[r][x[r][exp[r]] == 0]
        assert 0 < len(taken) < len(zeros)  # the cut falls inside the run of zeros
        assert np.array_equal(taken, zeros[:len(taken)])  # … which is taken in index order, whatever the signs
        signs = np.signbit(x[r][zeros[:len(taken) + 1]])
        assert signs.any() and not signs.all()
    tv = torch.topk(torch.from_numpy(x), k, dim=-1).values.numpy()
    assert np.array_equal(tv, np.take_along_axis(x, exp, 1))
    # the rows tell the two orders apart: sorting by the raw sign-magnitude bit key (−0.0 below +0.0, what the
    # radix select did before it canonicalised the zero) gives another index order on every row
    u = x.view(np.uint32).astype(np.int64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    by_bits = np.lexsort((np.broadcast_to(np.arange(n), x.shape), -key), axis=-1)[:, :k]
    assert all(not np.array_equal(by_bits[r], exp[r]) for r in range(3))


POSTPROCESS_CASES = [(300, 91, 300), (300, 80, 100), (7, 3, 21), (50, 80, 512), (100, 1, 100)]


@pytest.mark.parametrize("q,c,k", POSTPROCESS_CASES)
def test_postprocess_reference_matches_oracle(q, c, k):
    """oracle.rtdetr_np.post_process takes k = Q and returns the kept prefix: the two agree on it where k == Q; the
    flat-index decode, the scaling and the threshold edges hold for every k."""
    from oracle.rtdetr_np import post_process

    rng = np.random.default_rng(refs.seed("postprocess", q, c, k))
    logits, boxes = refs.postprocess_inputs(q, c, k, rng)
    ts = refs.TARGET_SIZES
    B, n = 4, q * c
    for thr in (0.5, 0.0, 1.0):
        got = refs.postprocess(logits, boxes, ts, k, thr)
        assert np.array_equal(got["labels"], got["idx"] % c)
        assert np.all(np.diff(got["scores"].astype(F32), axis=1) <= 0)
        if k == q:
            exp = post_process(logits, boxes, ts.tolist(), thr)
            for i in range(B):
                m = got["counts"][i]
                assert m == len(exp[i]["scores"])
                assert np.array_equal(got["labels"][i, :m], exp[i]["labels"])
                np.testing.assert_allclose(got["scores"][i, :m], exp[i]["scores"], rtol=0, atol=1e-7)
                np.testing.assert_allclose(got["boxes"][i, :m], exp[i]["boxes"], rtol=1e-6, atol=1e-4)
        if thr == 0.0:
            assert np.all(got["counts"] == k)
        if thr == 1.0:
            assert np.all(got["counts"] == 0)
    half = refs.postprocess(logits, boxes, ts, k, 0.5)
    flat = logits.reshape(B, n)
    # image 0: the top k hold every positive logit, then zeros (score == 0.5: not kept), then negatives
    assert half["counts"][0] == k // 3 == (flat[0] > 0).sum()
    assert (flat[0][half["idx"][0]] == 0).sum() == k // 3 and (flat[0][half["idx"][0]] < 0).any()
    # image 1: one tie class at 1.0, resolved by flat index
    sat = np.flatnonzero(flat[1] >= 20)
    assert len(sat) == min(n, k + 17) and np.array_equal(half["idx"][1], sat[:k])
    assert np.all(half["scores"][1].astype(F32) == 1.0) and half["counts"][1] == k
    assert flat[2].max() < 17


def test_box_kernel_inputs_hold_their_edges():
    rng = np.random.default_rng(9)
    anchors, valid, idx, delta = refs.ref_init_inputs(2, 37, rng)
    assert (~valid).sum() >= 3 and valid.sum() >= 100
    assert np.all(anchors[~valid] == refs.FLT_MAX) and np.isfinite(anchors[valid]).all()
    assert (~valid[idx]).sum() >= 6 and 0 in idx and len(anchors) - 1 in idx
    assert {0.0, 20.0, -20.0, 100.0, -100.0} <= set(delta.reshape(-1).tolist())
    u = refs.f64(delta).reshape(2, 37, 4) + refs.f64(anchors)[idx]
    s = refs.sigmoid(u)
    assert np.all(s[~valid[idx]] == 1.0)  # sigmoid(FLT_MAX + δ) is exactly 1
    ref, deltas = refs.box_refine_inputs(300, rng)
    for v in (0.0, 1.0, 1e-5, 1 - 1e-5, 5e-6):
        assert (ref == F32(v)).any()
    assert (ref < 0).any() and (ref > 1).any()
    for d in deltas:
        assert {0.0, 15.0, -15.0} <= set(d.reshape(-1).tolist())
