"""The direct split-MFMA 3×3 kernels of the fp32 path (sp_conv3x3_c64_x3, sp_conv3x3_c32_x3): bit-identity with
the x3 implicit GEMM on the same fp32 operands, accuracy against fp64, and the Engine dispatch knobs."""
import os
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import margins  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _reset_conv_config():
    yield
    from spotter_amd import ops

    ops.force_conv_config(None)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _operands(case, n, h, w, cin, cout, dev):
    rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
    x = rng.standard_normal((n, h, w, cin)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32)
    wk = T(wt.transpose(0, 2, 3, 1).reshape(cout, -1), dev)
    sc = T((0.5 + rng.random(cout)).astype(np.float32), dev)
    sh = T(rng.standard_normal(cout).astype(np.float32), dev)
    return x, wt, wk, sc, sh


def _gemm_x3(xv, n, h, w, cin, wk, planes, cout, sc, sh, act, dev, cfg, ldy=None, off=0):
    """The x3 implicit GEMM on the same operands, into a NaN-prefilled [m, ldy] buffer. No split-K workspace:
    these small maps would otherwise sum K in two partial passes, which is not the order of the production shapes."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    ldy = ldy or cout
    out = torch.full((n * h * w * ldy,), float("nan"), device=dev)
    ops.force_conv_config(cfg)
    ops.conv2d(xv, n, h, w, cin, wk, cout, 3, 1, 1, V(out, off, ldy), scale=sc, shift=sh, act=act, wt_planes=planes)
    ops.force_conv_config(None)
    return out.cpu().numpy()


SHAPES = [(13, 70), (9, 129), (4, 64), (1, 1), (17, 200)]
CFGS = ["14", None]


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("act", ["relu", None])
def test_c32_x3_bit_identical_to_gemm(dev, hw, cout, act):
    """sp_conv3x3_c32_x3 equals conv2d(wt_planes=split_bf16x3(w)) bit for bit, forced tile "14" and default pick."""
    from spotter_amd import ops
    from spotter_amd.ops import view

    n, (h, w) = 2, hw
    x, _, wk, sc, sh = _operands(("c32", hw, cout), n, h, w, 32, cout, dev)
    planes = ops.split_bf16x3(wk)
    xv = view(T(x.reshape(-1), dev), 32)
    out = torch.full((n * h * w * cout,), float("nan"), device=dev)
    ops.conv3x3_c32_x3(xv, planes, sc, sh, view(out, cout), n, h, w, cout, act=act)
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    for cfg in CFGS:
        ref = _gemm_x3(xv, n, h, w, 32, wk, planes, cout, sc, sh, act, dev, cfg)
        assert np.array_equal(got, ref), cfg


@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("act", ["relu", None])
@pytest.mark.parametrize("lds", [(64, 64), (128, 192), (64, 128)])
def test_c64_x3_bit_identical_to_gemm(dev, hw, act, lds):
    """sp_conv3x3_c64_x3 on channel-slice views (ldx, ldy) equals the x3 implicit GEMM bit for bit; the output is
    prefilled with NaN and the columns outside the 64-channel slice stay untouched."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    n, (h, w) = 2, hw
    ldx, ldy = lds
    xoff, yoff = ldx - 64, (ldy - 64) // 2 // 4 * 4  # the slice sits at the end of x's rows, inside y's
    m = n * h * w
    x, _, wk, sc, sh = _operands(("c64", hw), n, h, w, 64, 64, dev)
    planes = ops.split_bf16x3(wk)
    xw = np.random.default_rng(7).standard_normal((m, ldx)).astype(np.float32)
    xw[:, xoff:xoff + 64] = x.reshape(m, 64)
    xv = V(T(xw.reshape(-1), dev), xoff, ldx)
    out = torch.full((m * ldy,), float("nan"), device=dev)
    ops.conv3x3_c64_x3(xv, planes, sc, sh, V(out, yoff, ldy), n, h, w, act=act)
    got = out.cpu().numpy().reshape(m, ldy)
    inside = np.zeros(ldy, bool)
    inside[yoff:yoff + 64] = True
    assert np.isfinite(got[:, inside]).all()
    assert np.isnan(got[:, ~inside]).all()  # columns outside the slice unchanged
    for cfg in CFGS:
        ref = _gemm_x3(xv, n, h, w, 64, wk, planes, 64, sc, sh, act, dev, cfg, ldy=ldy, off=yoff).reshape(m, ldy)
        assert np.array_equal(got[:, inside], ref[:, inside]), cfg
        assert np.isnan(ref[:, ~inside]).all()


@pytest.mark.parametrize("kind", ["c64", "c32-32", "c32-64"])
def test_persistent_loop_bit_identical(dev, kind):
    """More than twice the CU count of tiles (n = 4 of 200 × 200: 700 tiles of 8 × 32), so every workgroup's later
    tiles come through the register prefetch and, where the weights stream, the ring running on across tiles."""
    from spotter_amd import ops
    from spotter_amd.ops import view

    n, h, w = 4, 200, 200
    cin, cout = (64, 64) if kind == "c64" else (32, int(kind[-2:]))
    assert n * ((h + 7) // 8) * ((w + 31) // 32) > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    x, _, wk, sc, sh = _operands(("loop", kind), n, h, w, cin, cout, dev)
    planes = ops.split_bf16x3(wk)
    xv = view(T(x.reshape(-1), dev), cin)
    out = torch.full((n * h * w * cout,), float("nan"), device=dev)
    if cin == 64:
        ops.conv3x3_c64_x3(xv, planes, sc, sh, view(out, cout), n, h, w, act="relu")
    else:
        ops.conv3x3_c32_x3(xv, planes, sc, sh, view(out, cout), n, h, w, cout, act="relu")
    got = out.cpu().numpy()
    for cfg in CFGS:
        assert np.array_equal(got, _gemm_x3(xv, n, h, w, cin, wk, planes, cout, sc, sh, "relu", dev, cfg)), cfg


@pytest.mark.parametrize("kind", ["c64", "c32-32", "c32-64"])
def test_direct_x3_is_fp32_accurate(dev, kind):
    """Against an fp64 conv of the same fp32 operands at (2, 13, 70), the bar of test_conv2d_f32x3_is_fp32_accurate:
    max error <= 2 × the fp32-MFMA path's on the same inputs + 1e-6 of the output scale, and <= 1e-5 of the output
    scale outright. Both errors are recorded per case (tests/margins.py)."""
    from spotter_amd import ops
    from spotter_amd.ops import view

    n, h, w = 2, 13, 70
    cin, cout = (64, 64) if kind == "c64" else (32, int(kind[-2:]))
    x, wt, wk, _, _ = _operands(("acc", kind), n, h, w, cin, cout, dev)
    xt = torch.from_numpy(x.astype(np.float64)).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xt, torch.from_numpy(wt.astype(np.float64)), padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(-1, cout).numpy()
    one, zero = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    xv = view(T(x.reshape(-1), dev), cin)
    m = n * h * w
    o32 = torch.empty(m * cout, device=dev)
    ops.conv2d(xv, n, h, w, cin, wk, cout, 3, 1, 1, view(o32, cout), scale=one, shift=zero,
               workspace=torch.empty(4 << 20, device=dev))
    ox3 = torch.empty(m * cout, device=dev)
    planes = ops.split_bf16x3(wk)
    if cin == 64:
        ops.conv3x3_c64_x3(xv, planes, one, zero, view(ox3, cout), n, h, w)
    else:
        ops.conv3x3_c32_x3(xv, planes, one, zero, view(ox3, cout), n, h, w, cout)
    scale = np.abs(ref).max()
    e32 = np.abs(o32.cpu().numpy().reshape(m, cout).astype(np.float64) - ref).max()
    ex3 = np.abs(ox3.cpu().numpy().reshape(m, cout).astype(np.float64) - ref).max()
    margins.record(f"direct_x3_{kind}", err_x3_rel=ex3 / scale, err_f32_rel=e32 / scale)
    print(f"direct_x3 {kind}: ex3 {ex3:.3e} e32 {e32:.3e} scale {scale:.3e}")
    assert ex3 <= 2 * e32 + 1e-6 * scale, (ex3, e32, scale)
    assert ex3 <= 1e-5 * scale, (ex3, scale)


def test_engine_knobs(dev):
    """Engine(precision="fp32") on R18vd at bs16 of 640² (stem maps 16 × 320², stage-0 maps 16 × 160²: both clear
    their pixel gates). The stage-0 knob swaps the x3 implicit GEMM for its bit-identical direct kernel, so the
    logits, boxes and selected anchors are equal bit for bit with it on and off. The stem knob swaps the
    exact-product fp32 kernel for the split kernel (another fp32-accurate rounding of the same sums), so each of
    its settings is held to the parity bar of test_gpu_model.py against the HF goldens: per image the detections,
    and every decoder query aligned by its anchor, scores within 1e-3, boxes within 0.5 px."""
    from test_gpu_model import check_image, run_tiled_batch

    from spotter_amd import SpotterForObjectDetection, ops
    from spotter_amd.config import PRESETS

    model = SpotterForObjectDetection(PRESETS["r18vd"], use_graphs=False, precision="fp32")
    eng = model.engine
    assert all(cw.x3p is not None for cw in eng.stem[1:]) == eng.direct_c32_x3
    if not eng.direct_c32_x3:  # the planes are built at load only when the knob is on
        for cw in eng.stem[1:]:
            cw.x3p = T(ops.split_bf16x3_host(cw.host), dev)
    default = (eng.direct_c64_x3, eng.direct_c32_x3)
    B, H, W = 16, 640, 640
    res, seen = {}, {}
    for knobs in ((True, True), (False, True), (True, False), (False, False)):
        eng.direct_c64_x3, eng.direct_c32_x3 = knobs
        shapes = []
        ops.set_launch_hook(lambda kind, launch, flops, nbytes, shape: (shapes.append(shape), launch()))
        try:
            _, g, dets, logits, boxes, topk = run_tiled_batch("r18vd", 4, "fp32", model=model)
        finally:
            ops.set_launch_hook(None)
        assert logits.shape[0] == B
        res[knobs] = (logits, boxes, topk)
        seen[knobs] = {s[:3] for s in shapes if s is not None and len(s) > 6 and s[5:7] == ("x3", "direct")}
        for b in range(B):
            check_image(g, b % 4, dets[b], logits[b], boxes[b], topk[b],
                        case=f"r18vd_640_fp32_bs16_direct_x3_c64{int(knobs[0])}_c32{int(knobs[1])}")
    eng.direct_c64_x3, eng.direct_c32_x3 = default
    m0, m1 = B * (H // 4) * (W // 4), B * (H // 2) * (W // 2)
    assert seen[(True, True)] == {(m0, 64, 576), (m1, 32, 288), (m1, 64, 288)}
    assert seen[(False, True)] == {(m1, 32, 288), (m1, 64, 288)}
    assert seen[(True, False)] == {(m0, 64, 576)} and not seen[(False, False)]
    for c32 in (True, False):  # the stage-0 knob: bit-identical
        for a, b in zip(res[(True, c32)], res[(False, c32)]):
            assert np.array_equal(a, b), c32
