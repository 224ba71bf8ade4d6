"""The Winograd path (csrc/winograd.hip) stage by stage against the fp64 references of tests/wino_refs.py.

One test per transform stage and tile size, one per component-GEMM target tuple, one per whole-path operand mode.
Each case builds its descriptor once (ops.conv_desc + ops.wino_desc), asserts through ops.wino_plan that the
stages would run what the case was built for, launches that very descriptor's stage(s) into NaN-prefilled buffers
(guard rows around the map, gap columns in A / C / residual rows, a guard tail behind C and behind the workspace)
and compares through conv_refs.compare: the exact families (ints, probe, impulse) bit for bit, the range family
element by element against the derived bound. A stage's foreign half of the workspace must come back untouched.

tests/test_wino_refs.py proves on the host that the matrix reaches what it must and that defective emulations
fail it; DESIGN.md ("Winograd stages against fp64") has the arguments and the figures measured on the MI355X.
-s prints the worst err / bound per stage and the file's wall time."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as R  # noqa: E402
import wino_refs as W  # noqa: E402

NAN = float("nan")
WORST, TIMES, LAUNCHES = {}, {}, {"n": 0}


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    t0 = time.perf_counter()
    yield torch.device("cuda", 0)
    slow = max(TIMES.items(), key=lambda kv: kv[1]) if TIMES else ("-", 0.0)
    print(f"\nwinograd stages: {LAUNCHES['n']} launches in {time.perf_counter() - t0:.1f} s, slowest test "
          f"{slow[0]} {slow[1]:.2f} s; worst range err / bound: "
          + ", ".join(f"{'/'.join(map(str, k))} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rows(a, ld, off, numel, dev):
    """[rows, cols] values → a NaN-filled device buffer of numel floats holding them as rows `ld` apart from `off`."""
    buf = np.full(numel, np.nan, np.float32)
    if a is not None:
        rows, cols = a.shape
        buf[off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]] = a.astype(np.float32)
    return T(buf, dev)


class Launch:
    """The device buffers, descriptor and stage launches of one case."""

    def __init__(self, c, r, dev):
        from spotter_amd import ops
        from spotter_amd.ops import V

        n, h, w, cin, cout = c["shape"]
        L = self.L = W.layout(c)
        wm, m = c["wm"], L["M"]
        self.c, self.keep = c, []
        xrows = r["x"].reshape(-1, cin) if "x" in r else None  # the GEMM / output stages must not read A: all NaN
        self.a = _rows(xrows, L["lda"], L["a_off"], L["a_numel"], dev)
        self.out = torch.full((L["c_numel"],), NAN, device=dev)
        kw = dict(act=r.get("act"))
        for name in ("scale", "shift"):
            if r.get(name) is not None:
                kw[name] = T(r[name], dev)
        for key, name, ld in (("r1", "res1", L["ldr1"]), ("r2", "res2", L["ldr2"])):
            if r.get(key) is not None:
                kw[name] = V(_rows(r[key], ld, 0, m * ld, dev), 0, ld)
        wt = torch.zeros(cout * 9 * cin, device=dev)  # sp_conv2d's fp32 weights: the Winograd stages do not read them
        nplanes = {"x3": 3, "x2": 2, "bf16": 1}[c["mode"]]
        if "planes" in r:
            self.planes = T(r["planes"], dev)
        else:
            self.planes = torch.zeros((nplanes, L["NC"] * cout * cin), dtype=torch.int16, device=dev)
        self.work = torch.full((L["work_numel"],), NAN, device=dev)
        self.d, _ = ops.conv_desc(V(self.a, L["a_off"], L["lda"]), n, h, w, cin, wt, cout, 3, 1, 1,
                                  V(self.out, L["c_off"], L["ldc"]), **kw)
        self.keep += [wt, kw]
        self.stages = ops.wino_desc(self.d, (self.planes, self.work, wm))
        with W.forced(c["cfg"]):
            key, comps, tiles, in_vw, out_vw = W.plan_of(self.d, wm)
        assert key == W.expected_plan(c) and comps == L["NC"] and tiles == L["T"], (c["id"], key, W.expected_plan(c))
        assert c["tile"] is None or key[1] == c["tile"] % 100, (c["id"], key)
        assert c["in_vw"] is None or in_vw == c["in_vw"], (c["id"], in_vw)

    def run(self, only=None):
        from spotter_amd import ops

        with W.forced(self.c["cfg"]):
            ops.wino_launch(self.stages, only)
        LAUNCHES["n"] += 1 if only else 3

    def V(self):
        L, cin = self.L, self.c["shape"][3]
        return self.work[:L["v_el"]].cpu().numpy().reshape(L["NC"], L["T"], cin)

    def M(self):
        L, cout = self.L, self.c["shape"][4]
        return self.work[L["v_el"]:L["v_el"] + L["m_el"]].cpu().numpy().reshape(L["NC"], L["T"], cout)

    def work_tail_is_nan(self, start):
        return bool(torch.isnan(self.work[start:]).all())

    def output(self):
        """[M, Cout] rows of C; asserts that every gap / guard element is still NaN."""
        L, cout = self.L, self.c["shape"][4]
        o = self.out.cpu().numpy()
        idx = L["c_off"] + np.arange(L["M"])[:, None] * L["ldc"] + np.arange(cout)[None, :]
        written = np.zeros(o.shape, bool)
        written[idx] = True
        assert np.isnan(o[~written]).all(), f"{self.c['id']}: a guard element of C was overwritten"
        return o[idx]


def _judge(c, r, got, fails, stage_key):
    bad, w, msg = W.compare(c, r, got)
    if c["fam"] == "range":
        WORST[stage_key] = max(WORST.get(stage_key, 0.0), w)
    if bad:
        fails.append(msg)


@pytest.mark.parametrize("wm", [2, 4])
def test_input_transform(dev, wm):
    """sp_winograd_f{2,4}3_input alone: V = Bᵀ d B bit for bit on integer maps (every coefficient, every ragged
    tile edge, the padded single tile, the F(2×2) pair kernel's odd tile count, both VW forms of F(4×4)), inside
    γ(n_row + n_col)·|Bᵀ||d||B| on the three range maps. The padding comes from the kernel's own zeros (NaN around
    and between the map's rows); M and the workspace tail stay NaN, C is not written."""
    fails = []
    for c in W.cases("in"):
        if c["wm"] != wm:
            continue
        r = W.build(c)
        q = Launch(c, r, dev)
        q.run("input")
        _judge(c, r, q.V(), fails, ("in", wm))
        assert q.work_tail_is_nan(q.L["v_el"]), f"{c['id']}: the input transform wrote behind V"
        assert bool(torch.isnan(q.out).all()), f"{c['id']}: the input transform wrote C"
    assert not fails, (len(fails), fails[:5])


@pytest.mark.parametrize("wm", [2, 4])
def test_output_transform(dev, wm):
    """sp_winograd_f{2,4}3_output alone on an M the test wrote: Y = Aᵀ M A and the epilogue (each part alone and
    all together, ldr1 != ldr2 != ldc) bit for bit on integers, inside the derived bound on the range family. V is
    NaN: the stage must not read it. Gap columns of C and its tail stay NaN, M is unchanged."""
    fails = []
    for c in W.cases("out"):
        if c["wm"] != wm:
            continue
        r = W.build(c)
        q = Launch(c, r, dev)
        L = q.L
        q.work[L["v_el"]:L["v_el"] + L["m_el"]] = T(r["m"].reshape(-1), dev)
        q.run("output")
        _judge(c, r, q.output(), fails, ("out", wm))
        assert np.array_equal(q.M(), r["m"]), f"{c['id']}: the output transform changed M"
        assert bool(torch.isnan(q.work[:L["v_el"]]).all()) and q.work_tail_is_nan(L["v_el"] + L["m_el"]), c["id"]
    assert not fails, (len(fails), fails[:5])


def _gemm_targets(chunk=24):
    """[(target tuple, part, cases)]: the cases of one tuple, in parts of at most `chunk` so that no test function
    takes more than a few seconds of fp64 reference building."""
    t = {}
    for c in W.cases("gemm"):
        t.setdefault(W.expected_plan(c), []).append(c)
    return [(k, i // chunk, v[i:i + chunk]) for k, v in sorted(t.items()) for i in range(0, len(v), chunk)]


@pytest.mark.parametrize("want,part,cases", _gemm_targets(),
                         ids=["-".join(map(str, k)) + f"-part{p}" for k, p, _ in _gemm_targets()])
def test_component_gemm(dev, want, part, cases):
    """sp_winograd_f{2,4}3_gemm alone on a V the test wrote and U planes chosen directly (different for every one
    of the 16 / 36 batch members): the mode's kept-product model bit for bit (probe, ints), e_acc on the range
    family; every forced id and every branch of the tile rule, asserted through sp_winograd_plan. V is unchanged,
    everything behind M is still NaN, C is not written."""
    fails = []
    for c in cases:
        r = W.build(c)
        q = Launch(c, r, dev)
        L = q.L
        q.work[:L["v_el"]] = T(r["v"].reshape(-1), dev)
        q.run("gemm")
        _judge(c, r, q.M(), fails, ("gemm", c["mode"]))
        assert np.array_equal(q.V(), r["v"]), f"{c['id']}: the component GEMM changed V"
        assert q.work_tail_is_nan(L["v_el"] + L["m_el"]), f"{c['id']}: the component GEMM wrote behind M"
        assert bool(torch.isnan(q.out).all()), f"{c['id']}: the component GEMM wrote C"
    assert not fails, (len(fails), fails[:5])


@pytest.mark.parametrize("mode", W.MODES)
def test_whole_path(dev, mode):
    """The three stages through ops.conv2d's Winograd form, both tile sizes: the impulse family equals the direct
    3×3 cross-correlation bit for bit (through the host weight transform, the handoff between the stages and the
    dyadic epilogue), the range family stays inside the propagated bound; and sp_conv3x3_winograd writes the same
    bits as the three F(2×2) stage calls."""
    from spotter_amd._lib import call
    from spotter_amd.ops import stream

    fails = []
    for c in W.cases("path"):
        if c["mode"] != mode:
            continue
        r = W.build(c)
        q = Launch(c, r, dev)
        q.run()
        got = q.output()
        _judge(c, r, got, fails, ("path", c["wm"], mode))
        assert q.work_tail_is_nan(q.L["v_el"] + q.L["m_el"]), c["id"]
        if c["wm"] == 2:
            first = q.out.clone()
            q.out.fill_(NAN)
            q.work.fill_(NAN)
            call("sp_conv3x3_winograd", C.byref(q.d), q.planes.data_ptr(), q.planes.shape[1], q.work.data_ptr(),
                 q.work.numel(), stream())
            LAUNCHES["n"] += 3
            assert np.array_equal(first.cpu().numpy().view(np.uint32), q.out.cpu().numpy().view(np.uint32)), c["id"]
    assert not fails, (len(fails), fails[:5])


LOOPS = ["in2", "in4", "out2", "out4"]


@pytest.mark.parametrize("kernel", LOOPS)
def test_grid_stride_loop(dev, kernel):
    """Each transform kernel's grid-stride loop: stream_grid caps the grid at 16 blocks of 256 threads per CU, so a
    launch of at least 1.5 × CUs·16·256 work items (the CU count read from the device) sends threads round the
    loop. Integer operands, period-3 images: the reference of three 7×6 images is compared with every group of
    three on the device, bit for bit."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    stage, wm = kernel[:-1], int(kernel[-1])
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    need = int(1.5 * cus * 16 * 256)
    h, w = 7, 6
    cin, cout = (32, 4) if stage == "in" else (32, 132)
    th, tw, t1 = W.tiles_of(1, h, w, wm)
    if stage == "in":
        per_image = (th * ((tw + 1) // 2) * cin // 4) if wm == 2 else t1 * cin // 2
    else:
        per_image = t1 * cout // 4 if wm == 2 else t1 * cout
    n = 3 * (-(-need // (3 * per_image)) + 1)
    assert n * per_image >= need, (n, per_image, need)
    c3 = W._case(stage, "ints", wm, "x3", (3, h, w, cin, cout))
    r = W.build(c3)
    nc, g = W.nc_of(wm), n // 3
    T3, T_all = 3 * t1, n * t1
    work = torch.full((nc * T_all * (cin + cout) + R.TAIL,), NAN, device=dev)
    out = torch.full((n * h * w * cout + R.TAIL,), NAN, device=dev)
    if stage == "in":
        a = T(r["x"], dev).repeat(g, 1, 1, 1).contiguous().view(-1)
    else:
        a = torch.full((n * h * w * cin,), NAN, device=dev)
        m = T(r["m"], dev)[:, None].expand(nc, g, T3, cout).contiguous().view(-1)
        work[nc * T_all * cin:nc * T_all * (cin + cout)] = m
    planes = torch.zeros((3, nc * cout * cin), dtype=torch.int16, device=dev)
    wt = torch.zeros(cout * 9 * cin, device=dev)
    d, _ = ops.conv_desc(V(a, 0, cin), n, h, w, cin, wt, cout, 3, 1, 1, V(out, 0, cout))
    stages = ops.wino_desc(d, (planes, work, wm))
    p = ops.wino_plan(d, wm)
    assert p["tiles"] == T_all and (wm == 2 or (p["in_vw"], p["out_vw"]) == (2, 1)), p
    ops.wino_launch(stages, "input" if stage == "in" else "output")
    LAUNCHES["n"] += 1
    if stage == "in":
        ref = T(r["ref"].astype(np.float32), dev)  # [NC, 3·t1, Cin]
        got = work[:nc * T_all * cin].view(nc, g, T3, cin)
        assert bool((got == ref[:, None]).all()), kernel
        assert bool(torch.isnan(work[nc * T_all * cin:]).all()) and bool(torch.isnan(out).all()), kernel
    else:
        ref = T(r["ref"].astype(np.float32), dev)  # [3·h·w, Cout]
        got = out[:n * h * w * cout].view(g, 3 * h * w, cout)
        assert bool((got == ref[None]).all()), kernel
        assert bool(torch.isnan(out[n * h * w * cout:]).all()), kernel
        assert bool(torch.isnan(work[:nc * T_all * cin]).all()), kernel  # V was not read into anything written


@pytest.mark.parametrize("wm", [2, 4])
def test_refusals_leave_the_output_untouched(dev, wm):
    """Every descriptor the stages must refuse, on real device buffers: each stage returns < 0, sp_last_error names
    the argument, and C and the workspace are still NaN."""
    from spotter_amd._lib import lib

    c = W._case("path", "range", wm, "x3", (1, 4, 6, 32, 4), epi=("affine", "res1", "act", "res2"))
    r = W.build(c)
    q = Launch(c, r, dev)
    L = lib()
    f = f"sp_winograd_f{wm}3_"
    wp, wn, pp, ps = q.work.data_ptr(), q.work.numel(), q.planes.data_ptr(), q.planes.shape[1]
    need = q.L["v_el"] + q.L["m_el"]

    def stage_calls(d, work_ptr=wp, work_elems=wn, planes_ptr=pp, stride=ps, gemm_only=False):
        s = torch.cuda.current_stream().cuda_stream
        out = [("gemm", getattr(L, f + "gemm")(C.byref(d), planes_ptr, stride, work_ptr, work_elems, s))]
        if not gemm_only:  # (the weight-plane arguments are the GEMM stage's alone)
            out += [("input", getattr(L, f + "input")(C.byref(d), work_ptr, work_elems, s)),
                    ("output", getattr(L, f + "output")(C.byref(d), work_ptr, work_elems, s))]
        return out

    def copy_with(**kw):
        from spotter_amd._lib import SpConvDesc

        d = SpConvDesc.from_buffer_copy(q.d)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    a, cp, r1 = q.d.A, q.d.C, q.d.res1
    cases = [(dict(lda=28), "lda"), (dict(ldc=0), "ldc"), (dict(ldr1=0), "ldr1"), (dict(ldr2=0), "ldr2"),
             (dict(A_bf16=a), "bf16 rows"), (dict(C_bf16=cp), "bf16 rows"), (dict(res1_bf16=r1), "bf16 rows"),
             (dict(res2_bf16=r1), "bf16 rows"), (dict(Ho=5), "3x3 stride-1"), (dict(Cin=48), "Cin % 32"),
             (dict(Cout=6), "Cout % 4"), (dict(A=a + 4), "16-byte aligned"), (dict(A2=a), "A2"),
             (dict(row_scale=a, row_period=3), "row_scale"), (dict(out_rows_per_group=2), "grouped rows"),
             (dict(ln_gamma=a), "LayerNorm")]
    for kw, word in cases:
        for stage, rc in stage_calls(copy_with(**kw)):
            assert rc < 0 and word in L.sp_last_error().decode(), (kw, stage, rc, L.sp_last_error())
    for stage, rc in stage_calls(q.d, work_elems=need - 1):
        assert rc < 0 and "workspace" in L.sp_last_error().decode(), (stage, rc)
    for stage, rc in stage_calls(q.d, work_ptr=wp + 4):
        assert rc < 0 and "16-byte aligned" in L.sp_last_error().decode(), (stage, rc)
    for stride, word in ((q.L["NC"] * 4 * 32 - 8, "wino_plane_stride"), (q.L["NC"] * 4 * 32 + 4, "16-byte aligned")):
        rc = dict(stage_calls(q.d, stride=stride, gemm_only=True))["gemm"]
        assert rc < 0 and word in L.sp_last_error().decode(), (stride, rc)
    rc = dict(stage_calls(q.d, planes_ptr=pp + 2, gemm_only=True))["gemm"]
    assert rc < 0 and "16-byte aligned" in L.sp_last_error().decode()
    torch.cuda.synchronize()
    assert bool(torch.isnan(q.out).all()) and bool(torch.isnan(q.work).all())
    q.run()  # and the unchanged descriptor still runs
    W_bad, w, msg = W.compare(c, r, q.output())
    assert not W_bad, msg
