"""Everything between the uint8 image and ResNet stage 0 on the MI355X against the references of tests/front_refs.py
(DESIGN.md 5.15): sp_preprocess_u8, the stem conv, the five direct 3×3 kernels, the pools, the upsample and the layout
copy. Exact families are compared bit for bit, `range` per element against a bound derived from the operands.

Every output buffer starts as NaN (bf16 rows: 0x7FC0) with 8 guard columns per row where the entry point takes an
ld, and a guard tail; the guards must keep their bits.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_refs as cr  # noqa: E402
import front_refs as R  # noqa: E402
import margins  # noqa: E402

F32, F64 = np.float32, np.float64
NAN32, NAN16 = 0x7FC00000, 0x7FC0
GUARD, TAIL = R.GUARD, R.TAIL


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def cus(dev):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _count_launches():
    from spotter_amd import ops

    seen = []
    ops.set_launch_hook(lambda kind, launch, flops, nbytes, shape: (seen.append(kind), launch()))
    yield
    ops.set_launch_hook(None)
    if seen:
        margins.record("front/launches", launches_n=len(seen))


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def last_error():
    from spotter_amd._lib import lib

    return lib().sp_last_error().decode(errors="replace")


def nan_buf(numel, bf16, dev):
    """A NaN output of numel elements + the guard tail: float32, or int16 bit patterns 0x7FC0."""
    if bf16:
        return torch.full((numel + TAIL,), NAN16, dtype=torch.int16, device=dev)
    return torch.full((numel + TAIL,), float("nan"), dtype=torch.float32, device=dev)


def rows_in(a2, ld, off, bf16, dev):
    """[rows, cols] fp32 values as device rows of ld elements from column off, NaN elsewhere (bf16: bit patterns)."""
    rows, cols = a2.shape
    if bf16:
        buf = np.full((rows, ld), NAN16, np.uint16)
        buf[:, off:off + cols] = R.bf16_bits(a2)
        return T(buf.view(np.int16).reshape(-1), dev)
    buf = np.full((rows, ld), np.nan, F32)
    buf[:, off:off + cols] = a2
    return T(buf.reshape(-1), dev)


def rows_out(out, rows, ld, off, cols, bf16, what):
    """The [rows, cols] block of an output buffer as (fp32 values, raw bf16 bits or None); asserts that every guard
    column and the tail kept the fill's bits."""
    host = out.cpu().numpy()
    raw = host.view(np.uint16) if bf16 else host.view(np.uint32)
    fill = NAN16 if bf16 else NAN32
    body = raw[:rows * ld].reshape(rows, ld)
    guard = np.ones(ld, bool)
    guard[off:off + cols] = False
    assert (body[:, guard] == fill).all(), f"{what}: a guard column was written"
    assert (raw[rows * ld:] == fill).all(), f"{what}: the guard tail was written"
    blk = np.ascontiguousarray(body[:, off:off + cols])
    return (cr.bf16_val(blk), blk) if bf16 else (blk.view(F32), None)


# =============================================================================================== stem conv 1
def run_stem(x, wt, sc, sh, cout, relu, bf16, dev):
    from spotter_amd import ops

    n, _, h, w = x.shape
    ho, wo = R.stem_out(h, w)
    m = n * ho * wo
    out = nan_buf(m * cout, bf16, dev)
    ops.stem_conv_nchw(T(x, dev), T(wt, dev), T(sc, dev), T(sh, dev), ops.V(out, 0, cout), cout,
                       act="relu" if relu else None)
    return rows_out(out, m, cout, 0, cout, bf16, "stem")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cout", [32, 64])
@pytest.mark.parametrize("fam", ["ints", "real"])
def test_stem_bit_for_bit(dev, fam, cout, bf16):
    """sp_stem_conv3x3s2_nchw(_bf16) equals stem_model on every shape, act none and relu."""
    for shape in R.STEM_SHAPES:
        x, wt, sc, sh = R.build_stem(fam, shape, cout)
        for relu in (False, True):
            ref = R.stem_model(x, wt, sc, sh, relu, bf16)
            got, _ = run_stem(x, wt, sc, sh, cout, relu, bf16, dev)
            bad = int((~R.same_bits(got, ref, relu)).sum())
            print(f"stem {fam} {shape} cout {cout} relu {relu} bf16 {bf16}: {bad} of {ref.size} differ")
            margins.record(f"front/stem/{fam}", differing=bad)
            assert bad == 0, (shape, relu)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("poison", R.POISONS, ids=["nan", "inf"])
def test_stem_poison(dev, poison, bf16):
    """NaN / +inf at pixel (0, 0) of every image and channel (where the out-of-map taps point): output (0, 0) of each
    image is non-finite (NaN for a NaN), everything else keeps the clean run's bits."""
    for shape in [(3, 4, 6), (3, 17, 31), (2, 5, 5)]:
        n, h, w = shape
        ho, wo = R.stem_out(h, w)
        x0, wt, sc, sh = R.build_stem("real", shape, 32)
        clean, _ = run_stem(x0, wt, sc, sh, 32, False, bf16, dev)
        x1 = R.build_stem("real", shape, 32, poison=poison)[0]
        got, _ = run_stem(x1, wt, sc, sh, 32, False, bf16, dev)
        first = np.zeros((n, ho, wo), bool)
        first[:, 0, 0] = True
        first = first.reshape(-1)
        assert not np.isfinite(got[first]).any(), shape
        if np.isnan(poison):
            assert np.isnan(got[first]).all(), shape
        assert np.array_equal(R.bits32(got[~first]), R.bits32(clean[~first])), shape
        ref = R.stem_model(x1, wt, sc, sh, False, bf16)
        assert np.array_equal(R.bits32(got[~first]), R.bits32(ref[~first])), shape


# =============================================================================================== the direct 3×3s
def run_conv(kind, b, n, h, w, cout, act, dev, ldx=None, ldy=None, ldr=None):
    """Launch one of the five direct kernels on a built case. Channel slices: x at the end of rows of ldx, y from
    column 8 of rows of ldy, the residual from column 8 of rows of ldr."""
    from spotter_amd import ops
    from spotter_amd.ops import V

    q = R.KINDS[kind]
    cin, bf = q["cin"], q["bf16"]
    m = n * h * w
    ldx, ldy = ldx or cin, ldy or cout
    xoff, yoff = ldx - cin, GUARD if ldy >= cout + GUARD else 0
    xv = V(rows_in(b["x"].reshape(m, cin), ldx, xoff, bf, dev), xoff, ldx)
    out = nan_buf(m * ldy, bf, dev)
    yv = V(out, yoff, ldy)
    sc, sh = T(b["scale"], dev), T(b["shift"], dev)
    if kind == "c32":
        ops.conv3x3_c32(xv, T(b["w"], dev), sc, sh, yv, n, h, w, cout, act=act)
    elif kind == "c32_bf16":
        ops.conv3x3_c32_bf16(xv, T(b["w_bits"].view(np.int16), dev), sc, sh, yv, n, h, w, cout, act=act)
    elif kind == "c64_bf16":
        rv = None
        if b["res"] is not None:
            ldr = ldr or 64
            roff = GUARD if ldr >= 64 + GUARD else 0
            rv = V(rows_in(b["res"], ldr, roff, True, dev), roff, ldr)
        ops.conv3x3_c64_bf16(xv, T(b["w_bits"].view(np.int16), dev), sc, sh, yv, n, h, w, act=act, res1=rv)
    else:
        planes = T(ops.split_bf16x3_host(b["w"]), dev)
        if kind == "c32_x3":
            ops.conv3x3_c32_x3(xv, planes, sc, sh, yv, n, h, w, cout, act=act)
        else:
            ops.conv3x3_c64_x3(xv, planes, sc, sh, yv, n, h, w, act=act)
    return rows_out(out, m, ldy, yoff, cout, bf, b["id"])


def check_conv(kind, fam, shape, cout, act, dev, res=False, **ld):
    b = R.build_conv(kind, fam, shape, cout, act, res=res)
    got, bits = run_conv(kind, b, *shape, cout, act, dev, **ld)
    worst, msg = R.judge(b, got, bits, relu=act == "relu")
    print(msg)
    margins.record(f"front/{kind}/{fam}", **({"differing": worst} if fam == "ints" else {"err_over_bound": worst}))
    assert (worst == 0) if fam == "ints" else (worst <= 1.0), msg


KIND_COUT = [(kind, cout) for kind, q in R.KINDS.items() for cout in q["couts"]]


@pytest.mark.parametrize("kind,cout", KIND_COUT)
def test_conv_geometry_ints(dev, kind, cout):
    """1×1 maps, one tile exactly, a row / column short of and past one tile, 2×2 tiles plus a ragged edge: n = 2."""
    for i, shape in enumerate(R.geometry(kind)):
        check_conv(kind, "ints", shape, cout, ("relu", None)[i % 2], dev)


@pytest.mark.parametrize("kind,cout", KIND_COUT)
def test_conv_geometry_range(dev, kind, cout):
    """Scaled N(0,1) rows and channels, FrozenBN constants: every element inside the bound built from the operands."""
    for i, shape in enumerate(R.geometry(kind)):
        check_conv(kind, "range", shape, cout, (None, "relu")[i % 2], dev)


@pytest.mark.parametrize("kind,cout", KIND_COUT)
def test_conv_persistent_walk(dev, cus, kind, cout):
    """Narrow maps of cap + 3 and 2·cap + 1 tiles: some workgroups run two tiles, then three (a second prefetch while
    the in-map mask is reused). Every tile has an out-of-map bottom row and right columns."""
    cap = R.grid_cap(kind, cout, cus)
    for shape in R.walk(kind, cout, cus):
        assert R.tiles(kind, *shape) > cap, (shape, cap)  # cannot pass without looping
        check_conv(kind, "ints", shape, cout, "relu", dev, res=kind == "c64_bf16")
    assert R.tiles(kind, *R.walk(kind, cout, cus)[1]) > 2 * cap


@pytest.mark.parametrize("kind", ["c64_bf16", "c64_x3"])
@pytest.mark.parametrize("lds", R.SLICES, ids=lambda v: f"{v[0]}-{v[1]}")
def test_conv_c64_channel_slices(dev, kind, lds):
    """Rows in and out as channel slices of wider buffers (NaN in every other column of both); c64_bf16 also with
    the residual from a slice with its own ldr."""
    ldx, ldy = lds
    shape = R.geometry(kind)[3]
    check_conv(kind, "ints", shape, 64, "relu", dev, ldx=ldx, ldy=ldy)
    if kind == "c64_bf16":
        check_conv(kind, "ints", shape, 64, "relu", dev, res=True, ldx=ldx, ldy=ldy, ldr=80)
        check_conv(kind, "ints", shape, 64, None, dev, res=True, ldx=ldx, ldy=ldy, ldr=64)
        check_conv(kind, "range", shape, 64, "relu", dev, res=True, ldx=ldx, ldy=ldy, ldr=80)


@pytest.mark.parametrize("kind,cout", KIND_COUT)
@pytest.mark.parametrize("poison", R.POISONS, ids=["nan", "inf"])
def test_conv_poison(dev, kind, cout, poison):
    """NaN / +inf in all channels of pixel (0, 0) of image 0, the element the out-of-map halo chunks load: only the
    outputs whose 3×3 window holds that pixel are non-finite, all others keep the clean run's bits."""
    for shape in R.geometry(kind):
        n, h, w = shape
        b0 = R.build_conv(kind, "ints", shape, cout, None)
        clean, cbits = run_conv(kind, b0, n, h, w, cout, None, dev)
        b1 = R.build_conv(kind, "ints", shape, cout, None, poison=poison)
        got, gbits = run_conv(kind, b1, n, h, w, cout, None, dev)
        win = R.poison_window(n, h, w)
        assert not np.isfinite(got[win]).any(), shape
        assert np.isfinite(got[~win]).all(), (shape, int((~np.isfinite(got[~win])).sum()))
        assert np.array_equal(R.bits32(got[~win]), R.bits32(clean[~win])), shape


# =============================================================================================== pools
def run_pool(which, x, bf16, dev):
    """Pool x [n, h, w, c] into a channel slice: column 8 of rows of c + 16."""
    from spotter_amd import ops

    n, h, w, c = x.shape
    ho, wo = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if which == "max" else ((h + 1) // 2, (w + 1) // 2)
    m, ldy = n * ho * wo, c + 2 * GUARD
    xt = T(R.bf16_bits(x).view(np.int16), dev) if bf16 else T(x, dev)
    out = nan_buf(m * ldy, bf16, dev)
    (ops.maxpool3x3s2 if which == "max" else ops.avgpool2x2_ceil)(xt, ops.V(out, GUARD, ldy), n, h, w, c)
    got, _ = rows_out(out, m, ldy, GUARD, c, bf16, f"{which}pool")
    return got.reshape(n, ho, wo, c)


POOL_BIG = [R.POOL_RPC4, R.POOL_CHUNKS, R.POOL_ROWS]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_maxpool_by_value(dev, bf16):
    """sp_maxpool3x3s2(_bf16) equals the reference by value (a max is one of its inputs, so no rounding; ±0 ties
    compare equal), ±inf and all -inf windows included; the 4-row chunk walk with a partial last chunk, and more
    chunks than gridDim.y."""
    for shape in R.POOL_SHAPES + POOL_BIG:
        for fam, special in (("ints", None), ("real", None), ("real", "inf")):
            if shape in POOL_BIG and fam == "ints":
                continue
            x = R.build_pool(fam, shape, bf16, special)
            got = run_pool("max", x, bf16, dev)
            ref = R.maxpool_ref(x)
            bad = int((got != ref).sum())
            print(f"maxpool {shape} {fam} {special} bf16 {bf16}: {bad} differ")
            margins.record("front/maxpool", differing=bad)
            assert bad == 0, (shape, fam, special)
    for shape in (R.POOL_RPC4, R.POOL_CHUNKS):
        ho, wo, gx, rpc, chunks = R.maxpool_geom(*shape, 8 if bf16 else 4)
        assert rpc == R.MP_ROWS, shape
    assert chunks > R.GRID_Y


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_avgpool_bit_for_bit(dev, bf16):
    """sp_avgpool2x2_ceil(_bf16) equals avgpool_model bit for bit: ragged edges (divisors 1, 2, 4), more than 65535
    output rows, a sum that overflows to +inf."""
    for shape in R.POOL_SHAPES + [R.POOL_ROWS]:
        for fam, special in (("ints", None), ("real", None), ("real", "big")):
            x = R.build_pool(fam, shape, bf16, special)
            got = run_pool("avg", x, bf16, dev)
            ref = R.avgpool_model(x, bf16)
            if special == "big" and shape[1] > 1:
                assert np.isposinf(ref).any()
            bad = int((~R.same_bits(got, ref)).sum())
            print(f"avgpool {shape} {fam} {special} bf16 {bf16}: {bad} differ")
            margins.record("front/avgpool", differing=bad)
            assert bad == 0, (shape, fam, special)


# =============================================================================================== upsample, layout
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_upsample_slices_bit_for_bit(dev, bf16):
    """Input from a channel slice (column offset c of rows of 2c), output into one (column 8 of rows of c + 16): a
    second, partial x-block (264 float4s per row) and more than 65535 input rows."""
    from spotter_amd import ops

    cases = [(2, 3, 66, 32), (65600, 1, 1, 8)] if bf16 else R.UPSAMPLE_CASES
    for n, h, w, c in cases:
        assert n * h > R.GRID_Y or w * (c // 2 if bf16 else c) // 4 == 264
        x = R.build_pool("real", (n, h, w, c), bf16)
        ldx, ldy = 2 * c, c + 2 * GUARD
        xt = rows_in(x.reshape(-1, c), ldx, c, bf16, dev)
        out = nan_buf(4 * n * h * w * ldy, bf16, dev)
        ops.upsample2x(ops.V(xt, c, ldx), ops.V(out, GUARD, ldy), n, h, w, c)
        got, _ = rows_out(out, 4 * n * h * w, ldy, GUARD, c, bf16, "upsample")
        ref = R.upsample_ref(x).reshape(-1, c)
        assert np.array_equal(R.bits32(got), R.bits32(ref)), (n, h, w, c)


def test_nchw_to_nhwc_bit_for_bit(dev):
    """c = 1, 3, 4, one pixel, odd sizes, and one case past grid_for's cap (the grid-stride loop)."""
    from spotter_amd import ops

    for shape in R.NCHW_CASES:
        x = np.random.default_rng(sum(shape)).standard_normal(shape).astype(F32)
        out = nan_buf(x.size, False, dev)
        ops.nchw_to_nhwc(T(x, dev), out)
        got, _ = rows_out(out, 1, x.size, 0, x.size, False, "nchw_to_nhwc")
        assert np.array_equal(R.bits32(got.reshape(-1)), R.bits32(x.transpose(0, 2, 3, 1).reshape(-1))), shape


# =============================================================================================== preprocess
def strided_images(imgs, pads, dev):
    """uint8 [H, W, 3] device views whose rows are 3·W + pad bytes apart, the padding 0xFF."""
    out = []
    for im, pad in zip(imgs, pads):
        h, w, _ = im.shape
        buf = np.full((h, 3 * w + pad), 0xFF, np.uint8)
        buf[:, :3 * w] = im.reshape(h, 3 * w)
        t = T(buf, dev)
        out.append(torch.as_strided(t, (h, w, 3), (3 * w + pad, 3, 1)) if pad else t.view(h, w, 3))
    return out


def check_preprocess(imgs, pads, oh, ow, dev, out_off=0):
    from oracle.pil_resize import preprocess
    from spotter_amd import ops

    n = len(imgs)
    out = torch.full((out_off + n * 3 * oh * ow + TAIL,), float("nan"), device=dev)
    ops.preprocess_u8(strided_images(imgs, pads, dev), out[out_off:], oh, ow)
    raw = out.cpu().numpy()
    assert (raw[:out_off].view(np.uint32) == NAN32).all() and (raw[out_off + n * 3 * oh * ow:].view(np.uint32) == NAN32).all()
    got = raw[out_off:out_off + n * 3 * oh * ow].reshape(n, 3, oh, ow)
    for i, im in enumerate(imgs):
        assert np.array_equal(R.bits32(got[i]), R.bits32(preprocess(im, (oh, ow)))), (i, im.shape, pads[i])


def _imgs(sizes, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]


SMALL_SIZES = [(9, 14), (8, 12), (5, 7), (1, 1), (9, 12), (8, 14), (3, 13), (7, 2)]


@pytest.mark.parametrize("pad", [1, 5, 64])
def test_preprocess_row_stride(dev, pad):
    """row_stride > 3·width (0xFF between the rows), resized and same-size sources."""
    imgs = _imgs(SMALL_SIZES, pad)
    check_preprocess(imgs, [pad] * len(imgs), 8, 12, dev)
    same = _imgs([(8, 12)] * 3, pad + 1)
    check_preprocess(same, [pad] * 3, 8, 12, dev)      # pad 64: the same-size fast path on strided rows
    check_preprocess(imgs[:3], [pad] * 3, 16, 40, dev)  # up-scaling


@pytest.mark.parametrize("n", [33, 65])
def test_preprocess_chunk_loop(dev, n):
    """More than kMaxImgs = 32 images: two and three launches, the last of one image."""
    imgs = _imgs([SMALL_SIZES[i % len(SMALL_SIZES)] for i in range(n)], n)
    check_preprocess(imgs, [0] * n, 8, 12, dev)


def test_preprocess_fast_path_next_to_generic(dev):
    """40 images: the first 32 have the output size (the same-size kernel), the last 8 do not."""
    imgs = _imgs([(8, 12)] * 32 + SMALL_SIZES[:1] + SMALL_SIZES[2:] + [(9, 14)], 40)
    assert len(imgs) == 40 and all(im.shape[:2] != (8, 12) for im in imgs[32:])
    check_preprocess(imgs, [0] * 40, 8, 12, dev)


def test_preprocess_unaligned_output(dev):
    """An output 4 bytes off 16-byte alignment with out_w % 4 == 0: the scalar stores (vec4 = 0)."""
    imgs = _imgs(SMALL_SIZES, 3)
    check_preprocess(imgs, [0] * len(imgs), 8, 12, dev, out_off=1)
    check_preprocess(_imgs([(8, 12)] * 2, 4), [0, 0], 8, 12, dev, out_off=1)


def test_preprocess_lds_limit(dev):
    """A vertical scale of 30 needs 61 of the 64 source rows the LDS band holds (the second source is also wide
    enough for the generic horizontal tap loop: 9 taps); a scale of 50 needs more and is refused with the output
    untouched."""
    from spotter_amd import ops
    from spotter_amd._lib import lib

    check_preprocess(_imgs([(120, 300)], 5), [0], 4, 256, dev)
    check_preprocess(_imgs([(120, 300), (120, 1000)], 7), [0, 3], 4, 256, dev)
    src = strided_images(_imgs([(200, 300)], 6), [0], dev)
    out = torch.full((3 * 4 * 256 + TAIL,), float("nan"), device=dev)
    with pytest.raises(RuntimeError, match="needs more LDS"):
        ops.preprocess_u8(src, out, 4, 256)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == NAN32).all()
    assert lib().sp_preprocess_u8(None, 1, 4, 256, out.data_ptr(), None) < 0


# =============================================================================================== argument checks
class Refusals:
    """Calls that must be refused before a launch: rc < 0, the entry point's name in sp_last_error, the NaN output
    untouched."""

    def __init__(self, name, out):
        from spotter_amd._lib import lib

        self.fn, self.name, self.out = getattr(lib(), name), name, out

    def refused(self, what, *args):
        rc = self.fn(*args)
        assert rc < 0, (self.name, what, rc)
        assert self.name in last_error(), (what, last_error())
        torch.cuda.synchronize()
        raw = self.out.cpu().numpy()
        raw = raw.view(np.uint16) if raw.dtype == np.int16 else raw.view(np.uint32)
        assert (raw == (NAN16 if raw.dtype == np.uint16 else NAN32)).all(), f"{self.name}: {what}: output touched"

    def accepted(self, *args):
        assert self.fn(*args) == 0, (self.name, last_error())
        torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_args_stem(dev, bf16):
    x = T(np.zeros((1, 3, 4, 4), F32), dev)
    wt, sc, sh = T(np.zeros((64, 27), F32), dev), T(np.ones(64, F32), dev), T(np.zeros(64, F32), dev)
    out = nan_buf(4 * 64 + 16, bf16, dev)
    es = out.element_size()
    r = Refusals("sp_stem_conv3x3s2_nchw" + ("_bf16" if bf16 else ""), out)
    a = lambda **k: tuple({**dict(x=x.data_ptr(), wt=wt.data_ptr(), sc=sc.data_ptr(), sh=sh.data_ptr(),
                                  y=out.data_ptr(), n=1, h=4, w=4, cout=32, act=1, s=None), **k}.values())
    r.refused("y off its store width", *a(y=out.data_ptr() + (4 if bf16 else 8)))
    r.refused("y one element off", *a(y=out.data_ptr() + es))
    r.refused("cout 48", *a(cout=48))
    r.refused("act silu", *a(act=2))
    r.refused("n 0", *a(n=0))
    r.refused("null x", *a(x=None))


@pytest.mark.parametrize("name", ["sp_conv3x3_c32", "sp_conv3x3_c32_bf16"])
def test_args_c32(dev, name):
    bf16 = name.endswith("bf16")
    x = nan_buf(16 * 32 + 16, bf16, dev)
    wt = torch.zeros(64 * 288 + 16, dtype=x.dtype, device=dev)
    sc, sh = T(np.ones(64, F32), dev), T(np.zeros(64, F32), dev)
    out = nan_buf(16 * 64 + 16, bf16, dev)
    es = out.element_size()
    r = Refusals(name, out)
    a = lambda **k: tuple({**dict(x=x.data_ptr(), wt=wt.data_ptr(), sc=sc.data_ptr(), sh=sh.data_ptr(),
                                  y=out.data_ptr(), n=1, h=4, w=4, cout=32, act=1, s=None), **k}.values())
    r.refused("x off 16 bytes", *a(x=x.data_ptr() + 2 * es))
    r.refused("w off 16 bytes", *a(wt=wt.data_ptr() + 2 * es))
    r.refused("y off 16 bytes", *a(y=out.data_ptr() + 2 * es))
    r.refused("cout 48", *a(cout=48))
    r.refused("act 2", *a(act=2))
    r.refused("h 0", *a(h=0))


def test_args_c64_bf16(dev):
    x = nan_buf(16 * 64 + 16, True, dev)
    wt = torch.zeros(64 * 576 + 16, dtype=torch.int16, device=dev)
    sc, sh = T(np.ones(64, F32), dev), T(np.zeros(64, F32), dev)
    out = nan_buf(16 * 72 + 16, True, dev)
    r = Refusals("sp_conv3x3_c64_bf16", out)
    a = lambda **k: tuple({**dict(x=x.data_ptr(), ldx=64, wt=wt.data_ptr(), sc=sc.data_ptr(), sh=sh.data_ptr(),
                                  y=out.data_ptr(), ldy=64, res=None, ldr=0, n=1, h=4, w=4, act=1, s=None),
                           **k}.values())
    r.refused("ldy % 8 (68 is a multiple of 4 only)", *a(ldy=68))
    r.refused("ldx % 8", *a(ldx=68))
    r.refused("ldx < 64", *a(ldx=56))
    r.refused("ldy < 64", *a(ldy=56))
    r.refused("y off 16 bytes", *a(y=out.data_ptr() + 8))
    r.refused("x off 16 bytes", *a(x=x.data_ptr() + 8))
    r.refused("res off 16 bytes", *a(res=x.data_ptr() + 8, ldr=64))
    r.refused("ldr % 8", *a(res=x.data_ptr(), ldr=68))
    r.refused("act 2", *a(act=2))


@pytest.mark.parametrize("name", ["sp_conv3x3_c32_x3", "sp_conv3x3_c64_x3"])
def test_args_x3(dev, name):
    c64 = "c64" in name
    x = nan_buf(16 * 64 + 16, False, dev)
    wp = torch.zeros(3 * 64 * 576 + 16, dtype=torch.int16, device=dev)
    sc, sh = T(np.ones(64, F32), dev), T(np.zeros(64, F32), dev)
    out = nan_buf(16 * 64 + 16, False, dev)
    r = Refusals(name, out)
    if c64:
        a = lambda **k: tuple({**dict(x=x.data_ptr(), ldx=64, wp=wp.data_ptr(), wps=64 * 576, sc=sc.data_ptr(),
                                      sh=sh.data_ptr(), y=out.data_ptr(), ldy=64, n=1, h=4, w=4, act=1, s=None),
                               **k}.values())
        r.refused("ldx < 64", *a(ldx=60))
        r.refused("ldy % 4", *a(ldy=66))
    else:
        a = lambda **k: tuple({**dict(x=x.data_ptr(), wp=wp.data_ptr(), wps=64 * 288, sc=sc.data_ptr(),
                                      sh=sh.data_ptr(), y=out.data_ptr(), n=1, h=4, w=4, cout=32, act=1, s=None),
                               **k}.values())
        r.refused("cout 48", *a(cout=48))
    r.refused("x off 16 bytes", *a(x=x.data_ptr() + 4))
    r.refused("y off 16 bytes", *a(y=out.data_ptr() + 4))
    r.refused("act 2", *a(act=2))
    r.refused("w 0", *a(w=0))


@pytest.mark.parametrize("name", ["sp_maxpool3x3s2", "sp_avgpool2x2_ceil", "sp_maxpool3x3s2_bf16",
                                  "sp_avgpool2x2_ceil_bf16"])
def test_args_pools(dev, name):
    bf16 = name.endswith("bf16")
    x = torch.zeros(2 * 4 * 4 * 16 + 16, dtype=torch.int16 if bf16 else torch.float32, device=dev)
    out = nan_buf(2 * 2 * 2 * 24 + 16, bf16, dev)
    es, v = out.element_size(), 8 if bf16 else 4
    r = Refusals(name, out)
    a = lambda **k: tuple({**dict(x=x.data_ptr(), y=out.data_ptr(), ldy=16, n=2, h=4, w=4, c=16, s=None),
                           **k}.values())
    r.refused("x off 16 bytes", *a(x=x.data_ptr() + 8))
    r.refused("x one element off", *a(x=x.data_ptr() + es))
    r.refused("y off 16 bytes", *a(y=out.data_ptr() + es))
    r.refused("ldy < c", *a(ldy=8))
    r.refused(f"ldy % {v}", *a(ldy=16 + v // 2))
    r.refused(f"c % {v}", *a(c=v + v // 2, ldy=24))
    r.refused("n 0", *a(n=0))


def test_args_upsample_and_layout(dev):
    x = torch.zeros(2 * 2 * 2 * 8 + 16, device=dev)
    out = nan_buf(2 * 4 * 4 * 8 + 16, False, dev)
    r = Refusals("sp_upsample2x_nearest", out)
    a = lambda **k: tuple({**dict(x=x.data_ptr(), ldx=8, y=out.data_ptr(), ldy=8, n=2, h=2, w=2, c=8, s=None),
                           **k}.values())
    r.refused("x off 16 bytes", *a(x=x.data_ptr() + 4))
    r.refused("y off 16 bytes", *a(y=out.data_ptr() + 4))
    r.refused("c % 4", *a(c=6))
    r.refused("ldx % 4", *a(ldx=10))
    r.refused("ldy % 4", *a(ldy=10))
    r.refused("h 0", *a(h=0))
    r = Refusals("sp_nchw_to_nhwc", out)
    r.refused("c 0", x.data_ptr(), out.data_ptr(), 1, 0, 2, 2, None)
    r.refused("null y", x.data_ptr(), None, 1, 3, 2, 2, None)


def test_args_preprocess(dev):
    from spotter_amd._lib import SpImageU8

    src = T(np.zeros((4, 8, 3), np.uint8), dev)
    out = nan_buf(3 * 4 * 8, False, dev)
    r = Refusals("sp_preprocess_u8", out)
    arr = (SpImageU8 * 1)()
    arr[0].data, arr[0].height, arr[0].width, arr[0].row_stride = src.data_ptr(), 4, 8, 23
    r.refused("row_stride < 3·width", arr, 1, 4, 4, out.data_ptr(), None)
    arr[0].row_stride = 16
    r.refused("same-size source (the fast path's conditions) with row_stride < 3·width", arr, 1, 4, 8, out.data_ptr(), None)
    arr[0].row_stride = -24
    r.refused("same-size source with a negative row_stride", arr, 1, 4, 8, out.data_ptr(), None)
    arr[0].row_stride = 24
    r.refused("out_w 0", arr, 1, 4, 0, out.data_ptr(), None)
    r.refused("n 0", arr, 0, 4, 4, out.data_ptr(), None)
    arr[0].height = 0
    r.refused("height 0", arr, 1, 4, 4, out.data_ptr(), None)
