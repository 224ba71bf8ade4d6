"""The encoder-side small kernels (sp_attention, sp_attention_bf16, sp_layernorm, sp_layernorm_bf16, sp_add_rows)
against the fp64 references of tests/encoder_refs.py: tile edges, the engine's buffer layout, the XCD-grouped work
mapping and its remainder branch, online-softmax extremes, LayerNorm shapes / row families / kernel selection, the
grid-stride loop and special values of sp_add_rows, and every argument the entry points refuse.

Every output buffer starts as NaN (int16 −1 for bf16 rows), so an unwritten element fails, and every padding
element is checked to be untouched. The error bars are the derived bounds of encoder_refs (from the operands, never
from a kernel's output); each case records the worst err/tol it saw in the parity-margins JSON (tests/margins.py).
tests/test_encoder_refs.py validates references, inputs and bounds without a GPU.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import encoder_refs as refs  # noqa: E402
import margins  # noqa: E402

F32 = np.float32
NAN_BITS = 0x7FC00000  # torch.full(nan) / np.nan as float32


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def last_error():
    from spotter_amd._lib import lib

    return lib().sp_last_error().decode(errors="replace")


def padded(rows2d, ld, off=0, fill=np.nan):
    """rows2d as rows of ld elements from element `off` of a flat host buffer, `fill` everywhere else."""
    rows, cols = rows2d.shape
    buf = np.full(off + rows * ld, fill, rows2d.dtype)
    buf[off:].reshape(rows, ld)[:, :cols] = rows2d
    return buf


def split_view(flat, rows, cols, ld, off):
    """(the [rows, cols] view, every other element) of a flat host array."""
    inside = np.zeros(flat.shape, bool)
    inside[off:off + rows * ld].reshape(rows, ld)[:, :cols] = True
    return flat[inside].reshape(rows, cols), flat[~inside]


# ----------------------------------------------------------------------------- attention
def run_attention(dev, inp, bf16, launches=1):
    """The engine's layout: q and k the two halves of one [rows, 2D] buffer, v in a buffer of its own with
    ldv = D + 8 (NaN padding), the output in columns [8, 8 + D) of NaN-filled rows of D + 16.
    → ([B, H, n, dh] float32 outputs, one per launch)."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    B, H, n, dh = inp.q.shape
    D, rows = H * dh, B * n
    qk = T(np.concatenate([refs.to_rows(inp.q), refs.to_rows(inp.k)], 1).reshape(-1), dev)
    v = T(padded(refs.to_rows(inp.v), D + 8), dev)
    outs = []
    for _ in range(launches):
        out = torch.full((rows * (D + 16),), float("nan"), device=dev)
        ops.attention(V(qk, 0, 2 * D), V(qk, D, 2 * D), V(v, 0, D + 8), V(out, 8, D + 16), B, n, H, dh, inp.scale,
                      bf16=bf16)
        flat = out.cpu().numpy()
        # a [rows, D + 16] buffer viewed from column 8: the last row's trailing 8 columns lie past the view's span
        full = flat.reshape(rows, D + 16)
        got = full[:, 8:8 + D]
        outside = np.concatenate([full[:, :8], full[:, 8 + D:]], 1)
        assert np.all(outside.view(np.uint32) == NAN_BITS), "attention wrote outside its output slice"
        assert not np.isnan(got).any(), f"{int(np.isnan(got).any(-1).sum())} output rows hold unwritten elements"
        outs.append(np.ascontiguousarray(got.reshape(B, n, H, dh).transpose(0, 2, 1, 3)))
    return outs


def check_attention(dev, family, B, H, n, dh, bf16, tag, launches=1):
    case = refs.attn_case(family, B, H, n, dh, bf16)
    outs = run_attention(dev, case.inp, bf16, launches)
    got = outs[0]
    assert np.isfinite(got).all()
    frac = np.abs(got - case.ref) / case.tol
    worst = float(frac.max())
    print(f"attention {tag} {family} B{B} H{H} n{n} dh{dh} {'bf16' if bf16 else 'f32'}: worst err/tol {worst:.4f}")
    margins.record(f"enc/attn/{'bf16' if bf16 else 'f32'}/{tag}/{family}/n{n}h{H}d{dh}b{B}", err_over_tol=worst)
    assert worst <= 1.0, (worst, np.unravel_index(frac.argmax(), frac.shape))
    for other in outs[1:]:
        assert np.array_equal(other.view(np.uint32), got.view(np.uint32)), "two launches differ"
    return got


KERNELS = pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])


@KERNELS
@pytest.mark.parametrize("dh", [32, 48, 64])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 129])
def test_attention_tile_edges(dev, n, dh, bf16):
    """Key counts around the 16-key block and the 64-key LDS tile / 64-query workgroup, two images, two heads."""
    got = check_attention(dev, "normal", 2, 2, n, dh, bf16, "edges")
    if n == 1:  # a single key: weight exactly 1, the output is V (rounded to bf16 by the bf16 kernel)
        v = refs.attn_inputs("normal", 2, 2, 1, dh).v
        assert np.array_equal(got, refs.bf16_round(v) if bf16 else v)


@KERNELS
@pytest.mark.parametrize("family", refs.ATTN_FAMILIES)
@pytest.mark.parametrize("H,n,dh", [(2, 129, 32), (2, 129, 48), (2, 129, 64), (8, 300, 32)])
def test_attention_families(dev, family, H, n, dh, bf16):
    """Every input family (sharp scores, a maximum rising in every block, a dominant first block, uniform
    weights, one-hot winners with |s| > 1000, V of 1e4) within the derived bound, twice with identical bits."""
    B = 2 if n == 129 and dh == 32 else 1
    check_attention(dev, family, B, H, n, dh, bf16, "families", launches=2)


@KERNELS
@pytest.mark.parametrize("n,H,B", [(1, 1, 511), (1, 1, 513), (1, 3, 173), (65, 8, 33)],
                         ids=["wg511-launch-order", "wg513-rem1", "wg519-rem7", "wg528-rem0"])
def test_attention_work_mapping(dev, n, H, B, bf16):
    """attn_work's XCD grouping (grids of ≥ 512 workgroups) with every remainder class of total mod 8 that the
    branch distinguishes (none, 1, 7) next to the launch-order grid just under the threshold. Data differ per
    (image, head), the output starts as NaN: a mapping that is no bijection leaves rows unwritten or computes a
    head from another's operands."""
    assert ((n + 63) // 64) * H * B in (511, 513, 519, 528)
    check_attention(dev, "normal", B, H, n, 32, bf16, "mapping")


@pytest.mark.parametrize("n,H,dh", refs.BIAS_SHAPES)
def test_attention_bf16_rounds_p_to_nearest(dev, n, H, dh):
    """The bf16 kernel's rounding of P is unbiased: on positive V, mean((got − ref)/ref) stays within 2⁻¹², where
    truncation would sit at −2.4e-3 (tests/test_encoder_refs.py shows both sides on a float32 emulation)."""
    inp = refs.bias_inputs(n, H, dh)
    ref, _, _ = refs.attention(refs.bf16_round(inp.q), refs.bf16_round(inp.k), refs.bf16_round(inp.v), inp.scale)
    got = run_attention(dev, inp, True)[0]
    mean, worst = refs.bias_statistic(got, ref)
    print(f"attention bf16 bias n{n} dh{dh}: mean rel {mean:+.3e}, max |rel| {worst:.3e}")
    margins.record(f"enc/attn/bf16/bias/n{n}h{H}d{dh}", mean_rel_abs=abs(mean), max_rel=worst,
                   bar=refs.BIAS_BAR)
    assert abs(mean) <= refs.BIAS_BAR, mean


def _refused(call, name, sentinel, what):
    before = sentinel.clone()
    rc = call()
    assert rc == -1, (what, rc)
    assert name in last_error(), (what, last_error())
    torch.cuda.synchronize()
    assert torch.equal(sentinel.view(torch.int32), before.view(torch.int32)), f"{what}: output touched"


@KERNELS
def test_attention_argument_checks(dev, bf16):
    """Each argument the kernels' indexing or float4 accesses do not cover is refused (−1, a message) before any
    launch: the sentinel output keeps its bits. The unmodified call runs."""
    from spotter_amd._lib import lib

    L = lib()
    fn = L.sp_attention_bf16 if bf16 else L.sp_attention
    B, n, H, dh = 2, 5, 2, 32
    D = H * dh
    buf = torch.zeros(B * n * 3 * D + 64, device=dev)
    out = torch.full((B * n * D + 64,), 3.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    base = dict(q=buf.data_ptr(), ldq=3 * D, k=buf.data_ptr() + 4 * D, ldk=3 * D, v=buf.data_ptr() + 8 * D,
                ldv=3 * D, o=out.data_ptr(), ldo=D, batch=B, n=n, heads=H, dh=dh)

    def call(**kw):
        a = dict(base, **kw)
        return fn(a["q"], a["ldq"], a["k"], a["ldk"], a["v"], a["ldv"], a["o"], a["ldo"], a["batch"], a["n"],
                  a["heads"], a["dh"], dh ** -0.5, stream)

    assert call() == 0, last_error()
    torch.cuda.synchronize()
    assert not torch.equal(out[:B * n * D], torch.full_like(out[:B * n * D], 3.0))
    out.fill_(3.0)
    bad = [{"q": None}, {"k": None}, {"v": None}, {"o": None}, {"n": 0}, {"n": -1}, {"batch": 0}, {"batch": -2},
           {"heads": 0}, {"heads": -1}, {"dh": 16}, {"dh": 40}, {"dh": 128}, {"dh": 0},
           {"ldq": 3 * D + 2}, {"ldk": 3 * D + 1}, {"ldv": 3 * D + 3}, {"ldo": D + 2},
           {"ldq": D - 4}, {"ldk": D - 4}, {"ldv": D - 4}, {"ldo": D - 4}, {"ldo": 0}, {"ldv": -3 * D},
           {"q": base["q"] + 4}, {"k": base["k"] + 4}, {"v": base["v"] + 8}, {"o": base["o"] + 4},
           {"o": base["o"] + 12}]
    for kw in bad:
        _refused(lambda: call(**kw), "sp_attention", out, kw)


# ----------------------------------------------------------------------------- layernorm
def run_layernorm(dev, x, g, b, ldx, ldy, xoff=0, goff=0, yoff=0, bf16=False):
    """x rows ldx apart from element xoff (NaN padding), gamma / beta from element goff of their buffers, the
    output rows ldy apart from element yoff of a buffer of NaN (int16 −1 for bf16 rows) → [rows, d]; asserts
    that nothing outside the output view changed."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    rows, d = x.shape
    xt = T(padded(x, ldx, xoff), dev)
    gt = T(np.concatenate([np.full(goff, np.nan, F32), g]), dev)[goff:]
    bt = T(np.concatenate([np.full(goff, np.nan, F32), b]), dev)[goff:]
    if bf16:
        y = torch.full((yoff + rows * ldy,), -1, dtype=torch.int16, device=dev)
    else:
        y = torch.full((yoff + rows * ldy,), float("nan"), device=dev)
    ops.layernorm(V(xt, xoff, ldx), gt, bt, V(y, yoff, ldy), rows, d, refs.LN_EPS)
    flat = y.cpu().numpy()
    got, outside = split_view(flat, rows, d, ldy, yoff)
    if bf16:
        assert np.all(outside == -1), "sp_layernorm_bf16 wrote outside its rows"
        return got.view(np.uint16)
    assert np.all(outside.view(np.uint32) == NAN_BITS), "sp_layernorm wrote outside its rows"
    return got


def check_layernorm(dev, family, rows, d, tag, **layout):
    c = refs.ln_case(family, rows, d)
    layout.setdefault("ldx", d + 4)
    layout.setdefault("ldy", d + 8)
    got = run_layernorm(dev, c.x, c.g, c.b, **layout)
    assert np.isfinite(got).all(), "unwritten or non-finite outputs"
    frac = np.abs(got - c.ref) / c.tol
    worst = float(frac.max())
    margins.record(f"enc/ln/{tag}/{family}/d{d}r{rows}", err_over_tol=worst)
    assert worst <= 1.0, (family, rows, d, layout, worst, np.unravel_index(frac.argmax(), frac.shape))
    if family == "const":
        assert np.array_equal(got.view(np.uint32), np.broadcast_to(c.b, got.shape).view(np.uint32)), \
            "constant rows must give beta bit for bit"
    return got, worst


@pytest.mark.parametrize("d,rows", refs.LN_SHAPES, ids=[f"d{d}-r{r}" for d, r in refs.LN_SHAPES])
def test_layernorm_shapes_and_families(dev, d, rows):
    """Every row family at every width (1 .. 1024: empty, partly and completely filled lane slots of all three
    kernels) and at row counts around the 4- and 16-row blocks, rows ldx = d + 4 apart, the output in rows of
    d + 8. d % 4 == 0 takes the float4 kernels (d = 256 its own), anything else the scalar one."""
    worst = {}
    for family in refs.LN_FAMILIES:
        _, worst[family] = check_layernorm(dev, family, rows, d, "shapes")
    print(f"layernorm d{d} rows{rows}: err/tol " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


LN_PATHS = [
    # d, layout, what runs
    (256, dict(ldx=260, ldy=264), "layernorm256_kernel"),
    (256, dict(ldx=257, ldy=264), "scalar: ldx mod 4"),
    (256, dict(ldx=260, ldy=259), "scalar: ldy mod 4"),
    (256, dict(ldx=260, ldy=264, xoff=1), "scalar: x off by one float"),
    (256, dict(ldx=260, ldy=264, yoff=1), "scalar: y off by one float"),
    (256, dict(ldx=260, ldy=264, goff=1), "scalar: gamma / beta off by one float"),
    (260, dict(ldx=264, ldy=268), "layernorm4_kernel"),
    (260, dict(ldx=261, ldy=268), "scalar: ldx mod 4"),
    (260, dict(ldx=264, ldy=268, xoff=3), "scalar: x off by three floats"),
    (260, dict(ldx=264, ldy=268, goff=1), "scalar: gamma / beta off by one float"),
]


def _path_id(d, what):
    return f"d{d}-" + what.replace(": ", "-").replace(" / ", " ").replace(" ", "_")


@pytest.mark.parametrize("d,layout,what", LN_PATHS, ids=[_path_id(d, w) for d, _, w in LN_PATHS])
def test_layernorm_kernel_selection(dev, d, layout, what):
    """The launcher's fall-back from the float4 kernels to the scalar one on a misaligned pointer or an ld that is
    no multiple of 4: each layout runs (a float4 kernel on such rows would fault or read the NaN padding) and is
    within the bound on every family. The two paths need not agree bit for bit."""
    for family in refs.LN_FAMILIES:
        check_layernorm(dev, family, 17, d, "paths/" + what.split(":")[0], **layout)


@pytest.mark.parametrize("rows", [5, 17])
def test_layernorm_bf16_is_the_fp32_kernel_rounded(dev, rows):
    """sp_layernorm_bf16 = the fp32 d = 256 kernel's bits rounded RNE, on every row family."""
    for family in refs.LN_FAMILIES:
        c = refs.ln_case(family, rows, 256)
        y32 = run_layernorm(dev, c.x, c.g, c.b, 260, 264)
        y16 = run_layernorm(dev, c.x, c.g, c.b, 260, 264, bf16=True)
        assert np.array_equal(y16, refs.bf16_bits(y32).reshape(rows, 256)), family


def test_layernorm_argument_checks(dev):
    """sp_layernorm / sp_layernorm_bf16 refuse (−1, a message, nothing launched): null pointers, rows ≤ 0,
    d ∈ {0, 1025, −1}, ldx or ldy < d; the bf16 form also d ≠ 256, ld % 4 and misaligned pointers."""
    from spotter_amd._lib import lib

    L = lib()
    rows = 4
    x = torch.ones(rows * 1100 + 16, device=dev)
    g = torch.ones(1100, device=dev)
    y = torch.full((rows * 1100 + 16,), 3.0, device=dev)
    y16 = torch.full((rows * 264 + 16,), 3, dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(fn, out, d=256, **kw):
        a = dict(x=x.data_ptr(), ldx=d, g=g.data_ptr(), b=g.data_ptr(), y=out.data_ptr(), ldy=d, rows=rows, d=d)
        a.update(kw)
        return fn(a["x"], a["ldx"], a["g"], a["b"], a["y"], a["ldy"], a["rows"], a["d"], 1e-5, stream)

    assert call(L.sp_layernorm, y) == 0, last_error()
    assert call(L.sp_layernorm, y, d=1024) == 0, last_error()
    assert call(L.sp_layernorm_bf16, y16) == 0, last_error()
    torch.cuda.synchronize()
    y.fill_(3.0)
    y16.fill_(3)
    for kw in ({"x": None}, {"g": None}, {"b": None}, {"y": None}, {"rows": 0}, {"rows": -1},
               {"d": 0, "ldx": 8, "ldy": 8}, {"d": -1, "ldx": 8, "ldy": 8}, {"d": 1025, "ldx": 1028, "ldy": 1028},
               {"ldx": 255}, {"ldy": 255},
               {"ldx": 252}, {"ldy": 0}, {"ldx": -256}, {"d": 257, "ldx": 256, "ldy": 260}):
        _refused(lambda: call(L.sp_layernorm, y, **kw), "sp_layernorm", y, kw)
    for kw in ({"x": None}, {"g": None}, {"b": None}, {"y": None}, {"rows": 0}, {"d": 260, "ldx": 260, "ldy": 260},
               {"d": 128, "ldx": 256, "ldy": 256}, {"ldx": 258}, {"ldy": 258}, {"ldx": 252}, {"ldy": 252},
               {"x": x.data_ptr() + 4}, {"g": g.data_ptr() + 8}, {"b": g.data_ptr() + 4}, {"y": y16.data_ptr() + 2},
               {"y": y16.data_ptr() + 4}):
        _refused(lambda: call(L.sp_layernorm_bf16, y16, **kw), "sp_layernorm_bf16", y16, kw)


# ----------------------------------------------------------------------------- add_rows
def run_add_rows(dev, a, b, cols, ldy, bf16):
    from spotter_amd import ops
    from spotter_amd.ops import V

    rows = a.shape[0]
    if bf16:
        out = torch.full((rows * ldy,), -1, dtype=torch.int16, device=dev)
    else:
        out = torch.full((rows * ldy,), float("nan"), device=dev)
    ops.add_rows(V(T(a.reshape(-1), dev), 0, a.shape[1]), V(T(b.reshape(-1), dev), 0, b.shape[1]), V(out, 0, ldy),
                 rows, cols)
    got = out.cpu().numpy().reshape(rows, ldy)
    if bf16:
        assert np.all(got[:, cols:] == -1)
        return got[:, :cols].view(np.uint16)
    assert np.all(got[:, cols:].view(np.uint32) == NAN_BITS)
    return got[:, :cols]


@KERNELS
def test_add_rows_grid_stride_loop(dev, bf16):
    """4200 × 2048: 1 075 200 eight-column items for a grid capped at 4096 × 256 = 1 048 576 threads, so the first
    26 624 threads take a second item. fp32 sums bit-exact, bf16 the fp32 sum rounded RNE."""
    rows, cols = 4200, 2048
    assert rows * (cols // 8) > 4096 * 256
    rng = np.random.default_rng(refs.seed("enc_add_rows_big"))
    a = rng.standard_normal((rows, cols + 4), dtype=F32)
    b = rng.standard_normal((rows, cols + 8), dtype=F32) * F32(3)
    want = a[:, :cols] + b[:, :cols]
    got = run_add_rows(dev, a, b, cols, cols + 8, bf16)
    if bf16:
        assert np.array_equal(got, refs.bf16_bits(want).reshape(rows, cols))
    else:
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@KERNELS
def test_add_rows_special_values(dev, bf16):
    """±inf and NaN propagate (any NaN payload), −0.0 + −0.0 stays −0.0, finite sums past bf16's largest finite
    value round to ±inf in the bf16 form and stay finite in fp32."""
    a, b, ns = refs.add_rows_special()
    with np.errstate(invalid="ignore", over="ignore"):
        want = a + b
    got = run_add_rows(dev, a, b, a.shape[1], a.shape[1] + 8, bf16)
    if bf16:
        wbits = refs.bf16_bits(want).reshape(want.shape)
        gotf = refs.bf16_float(got)
        over = np.isfinite(want) & (np.abs(want) > refs.BF16_MAX)
        assert over.any() and np.all(np.isinf(gotf[over]))
    else:
        wbits, gotf = want.view(np.uint32), got
        got = got.view(np.uint32)
    nan = np.isnan(want)
    assert nan.any() and np.array_equal(np.isnan(gotf), nan)
    assert np.array_equal(got[~nan], wbits[~nan])
    negz = (want == 0) & np.signbit(want)
    assert negz.any() and np.all(np.signbit(gotf[negz]))


def test_add_rows_argument_checks(dev):
    """sp_add_rows refuses (−1, a message, nothing launched): null operands, both or neither output, rows / cols
    ≤ 0, cols % 8, lda / ldb % 4, ldy % 8, an ld below cols, a pointer off a 16-byte boundary."""
    from spotter_amd._lib import lib

    L = lib()
    rows, cols = 3, 64
    a = torch.ones(rows * 80 + 16, device=dev)
    y = torch.full((rows * 80 + 16,), 3.0, device=dev)
    y16 = torch.full((rows * 80 + 16,), 3, dtype=torch.int16, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call(**kw):
        p = dict(a=a.data_ptr(), lda=72, b=a.data_ptr(), ldb=68, y=y.data_ptr(), y16=None, ldy=72, rows=rows,
                 cols=cols)
        p.update(kw)
        return L.sp_add_rows(p["a"], p["lda"], p["b"], p["ldb"], p["y"], p["y16"], p["ldy"], p["rows"], p["cols"],
                             stream)

    assert call() == 0, last_error()
    assert call(y=None, y16=y16.data_ptr()) == 0, last_error()
    torch.cuda.synchronize()
    y.fill_(3.0)
    y16.fill_(3)
    for kw in ({"a": None}, {"b": None}, {"y": None}, {"y16": y16.data_ptr()}, {"rows": 0}, {"rows": -1}, {"cols": 0},
               {"cols": 60}, {"cols": 68, "ldb": 72}, {"lda": 70}, {"ldb": 66}, {"ldy": 68}, {"lda": 60}, {"ldb": 56},
               {"ldy": 56}, {"a": a.data_ptr() + 4}, {"b": a.data_ptr() + 8}, {"y": y.data_ptr() + 4},
               {"y": None, "y16": y16.data_ptr() + 8}):
        before16 = y16.clone()
        _refused(lambda: call(**kw), "sp_add_rows", y, kw)
        assert torch.equal(y16, before16), kw
