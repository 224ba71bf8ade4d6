"""sp_winograd_f43_expand: a bottleneck's conv2 F(4×4) output transform fused into its 1×1 expand. Bit-identity with
the unfused pair (sp_winograd_f43_output, then sp_conv2d on a 32x32x16 LDS-DMA tile), accuracy against fp64, the
fallback to the unfused pair (plan query on the host, result on the GPU) and the Engine knob."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wino_refs as WR  # noqa: E402

gpu = pytest.mark.gpu
KS = (128, 256)  # the built instances
CIN2 = 32        # conv2's own Cin: the kernel never sees it (it reads M), so the smallest the stages take


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
    ops.force_splitk_config(None)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Pair:
    """conv2 (3×3, CIN2 → K, as F(4×4)) and the expand (1×1, K → Cout, + res1) on device buffers: M filled by the
    real input and gemm stages; the output / residual rows may sit inside wider rows (ldc / ldr1 > Cout)."""

    def __init__(self, dev, case, n, h, w, k, cout, act2="relu", act="relu", res=True, wide=False, workspace=None):
        from spotter_amd import ops
        from spotter_amd.ops import V, view

        rng = np.random.default_rng(zlib.crc32(repr(case).encode()))
        self.n, self.h, self.w, self.k, self.cout, self.m = n, h, w, k, cout, n * h * w
        m = self.m
        self.x = rng.standard_normal((n, h, w, CIN2)).astype(np.float32)
        self.w2 = (rng.standard_normal((k, 3, 3, CIN2)) / np.sqrt(9 * CIN2)).astype(np.float32)
        self.we = (rng.standard_normal((cout, k)) / np.sqrt(k)).astype(np.float32)
        self.e2 = dict(scale=(0.5 + rng.random(k)).astype(np.float32), shift=rng.standard_normal(k).astype(np.float32),
                       r1=None, r2=None, act=act2)
        self.ldc = cout + 32 if wide else cout
        self.ldr = cout + 64 if wide else cout
        self.coff, self.roff = (8, 16) if wide else (0, 0)
        r1 = rng.standard_normal((m, cout)).astype(np.float32) if res else None
        self.ee = dict(scale=(0.5 + rng.random(cout)).astype(np.float32),
                       shift=rng.standard_normal(cout).astype(np.float32), r1=r1, r2=None, act=act)
        d = lambda a: T(a, dev)  # noqa: E731
        self.xd = view(d(self.x.reshape(-1)), CIN2)
        self.w2d, self.wed = d(self.w2.reshape(k, -1)), d(self.we)
        self.sc2, self.sh2, self.sce, self.she = d(self.e2["scale"]), d(self.e2["shift"]), d(self.ee["scale"]), d(self.ee["shift"])
        self.wino = T(ops.split_bf16x3_host(ops.winograd_weights_host(self.w2, 4)), dev)
        self.planes = ops.split_bf16x3(self.wed)
        self.frag = ops.pack_expand_frag(self.planes, cout, k)
        self.T = n * ((h + 3) // 4) * ((w + 3) // 4)
        self.work = torch.zeros(ops.wino_work_elems(4, self.T, CIN2, k), device=dev)
        self.t2 = torch.full((m * k,), float("nan"), device=dev)
        self.res = None
        if res:
            rw = rng.standard_normal((m, self.ldr)).astype(np.float32)
            rw[:, self.roff:self.roff + cout] = r1
            self.res = V(d(rw.reshape(-1)), self.roff, self.ldr)
        self.dev, self.workspace = dev, workspace
        self.d2, _ = ops.conv_desc(self.xd, n, h, w, CIN2, self.w2d, k, 3, 1, 1, view(self.t2, k), scale=self.sc2,
                                   shift=self.sh2, act=act2)
        self.stages = ops.wino_desc(self.d2, (self.wino, self.work, 4))
        ops.wino_launch(self.stages, only="input")
        ops.wino_launch(self.stages, only="gemm")

    def expand_desc(self, out, planes=True):
        from spotter_amd import ops
        from spotter_amd.ops import V, view

        return ops.conv_desc(view(self.t2, self.k), self.n, self.h, self.w, self.k, self.wed, self.cout, 1, 1, 0,
                             V(out, self.coff, self.ldc), scale=self.sce, shift=self.she, act=self.ee["act"],
                             res1=self.res, workspace=self.workspace, wt_planes=self.planes if planes else None)

    def new_out(self):
        return torch.full((self.m * self.ldc,), float("nan"), device=self.dev)

    def fused(self, cfg, min_pixels=0, frag=True):
        """The entry point under forced tile cfg → (output rows [m, ldc], whether it fused, t2 afterwards)."""
        from spotter_amd import ops

        self.t2.fill_(float("nan"))
        out = self.new_out()
        de, hook = self.expand_desc(out)
        ops.force_conv_config(cfg)
        try:
            did = ops.wino_expand(self.stages, self.d2, self.work, de, hook, self.frag if frag else None, min_pixels)
        finally:
            ops.force_conv_config(None)
        return out.cpu().numpy().reshape(self.m, self.ldc), did, self.t2.cpu().numpy()

    def entry(self, cfg, min_pixels=0):
        """sp_winograd_f43_expand itself (no host-side choice between the paths) → output rows."""
        from spotter_amd import ops
        from spotter_amd._lib import call

        self.t2.fill_(float("nan"))
        out = self.new_out()
        de, _ = self.expand_desc(out)
        ops.force_conv_config(cfg)
        try:
            call("sp_winograd_f43_expand", C.byref(self.d2), self.work.data_ptr(), self.work.numel(), C.byref(de),
                 self.frag.data_ptr(), self.frag.numel(), int(min_pixels), ops.stream())
        finally:
            ops.force_conv_config(None)
        return out.cpu().numpy().reshape(self.m, self.ldc)

    def unfused(self, cfg, planes=True):
        """sp_winograd_f43_output, then sp_conv2d under forced tile cfg → output rows."""
        from spotter_amd import ops

        self.t2.fill_(float("nan"))
        ops.wino_launch(self.stages, only="output")
        out = self.new_out()
        de, hook = self.expand_desc(out, planes)
        ops.force_conv_config(cfg)
        try:
            ops.conv_launch(de, hook)
        finally:
            ops.force_conv_config(None)
        return out.cpu().numpy().reshape(self.m, self.ldc)

    def inside(self):
        c = np.zeros(self.ldc, bool)
        c[self.coff:self.coff + self.cout] = True
        return c


# (Cout, act2, act, res1, wide rows): every Cout, residual on / off, relu / none on either conv, ld = / > Cout
VARIANTS = [(32, "relu", "relu", True, True), (96, None, None, False, False), (256, "relu", None, True, False),
            (96, None, "relu", True, True)]
MAPS = [(1, 1), (3, 3), (4, 4), (5, 7), (6, 10), (8, 8)]  # clipped tiles; a last unit of one Winograd tile


@gpu
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("n", [1, 2])
def test_bit_identical_to_unfused_pair(dev, n, hw, k):
    """Fused under forced tile "46" equals sp_winograd_f43_output + sp_conv2d under "46" and under "245", bit for bit,
    into NaN-prefilled rows; columns outside the Cout slice stay NaN and conv2's own output rows are not written."""
    for cout, act2, act, res, wide in VARIANTS:
        p = Pair(dev, ("bit", n, hw, k, cout), n, hw[0], hw[1], k, cout, act2, act, res, wide)
        got, did, t2 = p.fused("46")
        assert did, (cout, "the plan did not fuse")
        assert np.isnan(t2).all()
        c = p.inside()
        assert np.isfinite(got[:, c]).all() and np.isnan(got[:, ~c]).all()
        for cfg in ("46", "245"):
            ref = p.unfused(cfg)
            assert np.array_equal(got[:, c], ref[:, c]), (cout, cfg, np.abs(got[:, c] - ref[:, c]).max())
        assert np.array_equal(p.entry("46")[:, c], got[:, c])


@gpu
def test_persistent_loop_bit_identical(dev):
    """3 × 40 × 40 at K = 256, Cout = 64: 150 units, and Cout below a chunk (six of the eight waves idle)."""
    p = Pair(dev, "loop", 3, 40, 40, 256, 64)
    got, did, _ = p.fused("46")
    assert did
    for cfg in ("46", "245"):
        assert np.array_equal(got, p.unfused(cfg)), cfg


@gpu
@pytest.mark.parametrize("k", KS)
def test_many_units_per_workgroup_bit_identical(dev, k):
    """More units than three per CU (8 × 56 × 56: 784 units), so every workgroup walks several pixel tiles, some of
    three units and some of fewer; Cout 288: a second chunk that only one wave takes."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = Pair(dev, ("many", k), 8, 56, 56, k, 288)
    assert (p.T + 1) // 2 > 3 * cus or cus > 256
    got, did, _ = p.fused("46")
    assert did
    assert np.array_equal(got, p.unfused("46"))


@gpu
@pytest.mark.parametrize("k", KS)
def test_fused_is_fp32_accurate(dev, k):
    """Against fp64 from the same M (wino_refs.output_ref, epilogue; the expand in fp64 on the fp64 map), under the
    bar of test_conv2d_f32x3_is_fp32_accurate: max error <= 2 × the fp32-MFMA expand's on the same inputs (the
    unfused pair with the expand on fp32 weights) + 1e-6 of the output scale, and <= 1e-5 of the output scale."""
    n, h, w, cout = 2, 6, 10, 96
    p = Pair(dev, ("acc", k), n, h, w, k, cout)
    M = p.work[36 * p.T * CIN2:].cpu().numpy().reshape(36, p.T, k)
    t2 = WR.epilogue(WR.output_ref(M, n, h, w, 4), p.e2)[3]
    ref = WR.epilogue(t2 @ p.we.astype(np.float64).T, p.ee)[3]
    got, did, _ = p.fused("46")
    assert did
    f32 = p.unfused(None, planes=False)
    scale = np.abs(ref).max()
    ex3, e32 = np.abs(got - ref).max(), np.abs(f32 - ref).max()
    print(f"wino_expand K={k}: ex3 {ex3:.3e} e32 {e32:.3e} scale {scale:.3e}")
    assert ex3 <= 2 * e32 + 1e-6 * scale, (ex3, e32, scale)
    assert ex3 <= 1e-5 * scale, (ex3, scale)


def _fake_pair(n, h, w, k, cout, workspace=False):
    """conv2 / expand descriptors on fake aligned pointers (no device): the plan query reads no memory."""
    from spotter_amd._lib import SpConvDesc

    P = 1 << 20
    d2 = SpConvDesc(A=P, lda=CIN2, N=n, H=h, W=w, Cin=CIN2, KH=3, KW=3, stride=1, pad=1, Ho=h, Wo=w, Wt=2 * P, Cout=k,
                    scale=3 * P, shift=4 * P, act=1, C=5 * P, ldc=k, precision=2)
    de = SpConvDesc(A=5 * P, lda=k, N=n, H=h, W=w, Cin=k, KH=1, KW=1, stride=1, pad=0, Ho=h, Wo=w, Wt=6 * P, Cout=cout,
                    scale=7 * P, shift=8 * P, act=1, res1=9 * P, ldr1=cout, C=10 * P, ldc=cout, precision=2,
                    Wt_bf16=11 * P, wt_plane_stride=cout * k)
    if workspace:
        de.workspace, de.workspace_elems = 12 * P, 1 << 24
    T_ = n * ((h + 3) // 4) * ((w + 3) // 4)
    return d2, de, 36 * T_ * (CIN2 + k)


def test_plan_query_on_host():
    """sp_winograd_expand_plan without a device: fused on a 32x32x16 LDS-DMA tile; not on a 16x16x32 tile, a split-K
    plan, an unbuilt K, Cout % 32 != 0, without fragments, below the pixel gate; a mismatched pair is refused."""
    from spotter_amd import ops

    d2, de, we = _fake_pair(2, 8, 8, 256, 96)
    try:
        ops.force_conv_config("46")
        p = ops.wino_expand_plan(d2, we, de)
        assert p["fused"] == 1 and p["tiles"] == 8 and p["units"] == 4
        assert (p["expand"]["family"], p["expand"]["tile"], p["expand"]["planes"], p["expand"]["splits"]) == (2, 46, 3, 1)
        assert ops.wino_expand_plan(d2, we, de, has_frag=False)["fused"] == 0
        assert ops.wino_expand_plan(d2, we, de, min_pixels=129)["fused"] == 0
        assert ops.wino_expand_plan(d2, we, de, min_pixels=128)["fused"] == 1
        ops.force_conv_config("47")  # cfg 45 on 16x16x32 MFMAs
        p = ops.wino_expand_plan(d2, we, de)
        assert p["fused"] == 0 and p["expand"]["tile"] == 47
        ops.force_conv_config("46")
        for k, cout in ((64, 96), (512, 96), (256, 80)):
            a, b, c = _fake_pair(2, 8, 8, k, cout)
            assert ops.wino_expand_plan(a, c, b)["fused"] == 0, (k, cout)
        ops.force_conv_config(None)
        a, b, c = _fake_pair(2, 8, 8, 256, 96, workspace=True)  # 128 rows, eight k-tiles: split-K
        p = ops.wino_expand_plan(a, c, b)
        assert p["expand"]["splits"] > 1 and p["fused"] == 0
        ops.set_plan_batch(2, 64)  # planned as 64 images: 4096 rows against the gate
        ops.force_conv_config("46")
        assert ops.wino_expand_plan(d2, we, de, min_pixels=4096)["fused"] == 1
        assert ops.wino_expand_plan(d2, we, de, min_pixels=4097)["fused"] == 0
        ops.set_plan_batch(0, 0)
        de.lda = 260
        with pytest.raises(RuntimeError, match="conv2's output rows"):
            ops.wino_expand_plan(d2, we, de)
    finally:
        ops.set_plan_batch(0, 0)
        ops.force_conv_config(None)


@gpu
@pytest.mark.parametrize("how", ["m16", "splitk", "gate"])
def test_fallback_result(dev, how):
    """Where the plan declines, the entry point itself launches the output transform and the planned expand: conv2's
    rows are written, and the result equals the unfused pair's."""
    ws = torch.empty(1 << 22, device=dev) if how == "splitk" else None
    p = Pair(dev, ("fb", how), 2, 6, 10, 256, 96, workspace=ws)
    cfg = "47" if how == "m16" else None if how == "splitk" else "46"
    _, did, _ = p.fused(cfg, min_pixels=121 if how == "gate" else 0)
    assert not did
    got = p.entry(cfg, min_pixels=121 if how == "gate" else 0)
    assert np.isfinite(p.t2.cpu().numpy()).all()
    assert np.array_equal(got, p.unfused(cfg))


@gpu
def test_engine_knob(dev):
    """R101vd at bs2 of 320² with the pixel gates (the fused kernel's and F(4×4)'s own) lowered on the instance: the knob on / off gives identical logits and
    boxes; on, the stride-1 bottlenecks whose expand is planned on a 32x32x16 LDS-DMA tile run one fused launch (hook
    shape (M, Cout, K, 1, 1, "x3", "epi:res")) in place of the output transform and the expand."""
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor, ops
    from spotter_amd.config import PRESETS
    from spotter_amd.engine import Engine
    from spotter_amd.synthetic import synthetic_image

    cfg = PRESETS["r101vd"]
    w = SpotterForObjectDetection(cfg)._host_weights()
    proc = SpotterImageProcessor(size={"height": 320, "width": 320})
    x = proc(images=[synthetic_image(11), synthetic_image(12)])["pixel_values"].cuda()
    res, names = {}, {}
    for knob in (True, False):
        eng = Engine(cfg, w, "cuda", wino_expand=knob)
        eng.WINO_EXPAND_MIN_PIXELS = eng.WINO43_MIN_WORK = 0  # these maps are below the F(4x4) gate as well
        assert any(b["layers"][2].xfrag is not None for b in eng.blocks if b["type"] == "bottleneck") == knob
        seen = []
        real = ops.call

        def spy(name, *args):
            seen.append(name)
            return real(name, *args)

        ops.call = spy
        try:
            lg, bx = eng.forward(x)
            torch.cuda.synchronize()
        finally:
            ops.call = real
        res[knob] = (lg.cpu().numpy(), bx.cpu().numpy())
        names[knob] = seen
    assert np.array_equal(res[True][0], res[False][0]) and np.array_equal(res[True][1], res[False][1])
    nf = names[True].count("sp_winograd_f43_expand")
    assert nf > 0 and "sp_winograd_f43_expand" not in names[False]
    # each fused launch replaces one output transform and one sp_conv2d
    assert names[False].count("sp_winograd_f43_output") - names[True].count("sp_winograd_f43_output") == nf
    assert names[False].count("sp_conv2d") - names[True].count("sp_conv2d") == nf
    for n_ in ("sp_winograd_f43_input", "sp_winograd_f43_gemm"):
        assert names[True].count(n_) == names[False].count(n_)


@gpu
def test_two_stream_forward_is_deterministic_with_knob(dev):
    """test_gpu_model.py::test_two_stream_forward_is_deterministic's check with the fused kernel on the path (R101vd,
    bs4 of 320², gate lowered): repeated two-stream forwards are bit-identical."""
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.config import PRESETS
    from spotter_amd.engine import Engine
    from spotter_amd.synthetic import synthetic_image

    cfg = PRESETS["r101vd"]
    w = SpotterForObjectDetection(cfg)._host_weights()
    proc = SpotterImageProcessor(size={"height": 320, "width": 320})
    x = proc(images=[synthetic_image(s) for s in (1, 2, 3, 4)])["pixel_values"].cuda()
    eng = Engine(cfg, w, "cuda", wino_expand=True)
    eng.WINO_EXPAND_MIN_PIXELS = eng.WINO43_MIN_WORK = 0
    outs = []
    with torch.no_grad():
        for _ in range(4):
            outs.append([t.clone() for t in eng.forward(x, microbatches=2)])
    torch.cuda.synchronize()
    for lg, bx in outs[1:]:
        assert torch.equal(lg, outs[0][0]) and torch.equal(bx, outs[0][1])
