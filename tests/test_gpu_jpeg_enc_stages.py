"""GPU: csrc/jpeg_enc.hip stage by stage. One sp_jpeg_enc_rgb call per case of tests/jpeg_enc_cases.py into buffers of
exactly the layout's work_bytes and bits_cap, each between 256-byte guard regions of one pattern-filled allocation;
then every intermediate is read off the device and compared, exactly, with the numpy oracle
(oracle/jpeg_enc_np.py) and Pillow:

  jpeg_fdct_kernel      the quantised coefficients == scan_order_blocks
  jpeg_mcu_bits_kernel  the per-MCU bit counts     == mcu_bit_counts
  jpeg_scan_kernel      the offsets == their exclusive cumulative sum, the total == their sum; the bit words
                        zeroed under whatever the buffer held before (the pattern)
  jpeg_emit_kernel      the first ceil(nbits / 8) bytes == entropy_bits(stuff=False), the last byte's unused bits
                        zero; the four guards intact
  sp_jpeg_enc_finish    over the device's bits: Pillow's file

A failure names the first differing MCU, block and zig-zag index, MCU, or stream bit and the MCU it falls in.
tests/test_jpeg_enc_cases.py asserts on the CPU what makes this demand fair and complete (the oracle writes Pillow's
bytes for every case; the table reaches every special path of walk_mcu under both Huffman tables).

Then the input forms JpegEncoder.encode hands the kernels (4-byte pixels, cropped views: a row stride above W * pb
and an odd base address, a side stream, reused and regrown buffers with stale bits) against Pillow's bytes, and
sp_jpeg_enc_rgb's argument checks."""
import ctypes as C
import io
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_enc_cases as ec  # noqa: E402

GUARD = 256


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


def _plan(W, H, quality, sub):
    from spotter_amd._lib import SpJpegEncLayout, lib

    lay = SpJpegEncLayout()
    assert lib().sp_jpeg_enc_plan(W, H, quality, sub, C.byref(lay)) == 0, lib().sp_last_error()
    return lay


def _up(n, a):
    return -(-n // a) * a


class Arena:
    """One device allocation filled with a position-dependent byte pattern:
    [guard 256][work: work_bytes][guard 256] .. [guard 256][bits: bits_cap][guard 256], work and bits 256-byte
    aligned, and 512 spare bytes at the end so that a call the argument checks should have refused, had it run,
    would still have stayed inside the allocation."""

    def __init__(self, dev, lay):
        self.work_bytes, self.bits_cap = lay.work_bytes, lay.bits_cap
        self.work_off = GUARD
        self.bits_off = _up(self.work_off + self.work_bytes + GUARD, 256) + GUARD
        self.size = self.bits_off + self.bits_cap + GUARD + 512
        raw = torch.empty(self.size + 256, dtype=torch.uint8, device=dev)
        skew = -raw.data_ptr() % 256
        self.buf = raw[skew:skew + self.size]
        self.pattern = ((np.arange(self.size, dtype=np.int64) * 37 + 11) & 255).astype(np.uint8)
        self.buf.copy_(torch.from_numpy(self.pattern))
        self.nbits = torch.full((1,), -12345, dtype=torch.int64, device=dev)
        self.work_ptr = self.buf.data_ptr() + self.work_off
        self.bits_ptr = self.buf.data_ptr() + self.bits_off
        assert self.work_ptr % 256 == 0 and self.bits_ptr % 256 == 0

    def guards(self, host):
        """[(name, bytes found, bytes written there before the call)] for the four guards; the rest of the
        allocation outside work and bits is compared as well (as part of the guard it follows)."""
        w0, w1 = self.work_off, self.work_off + self.work_bytes
        b0, b1 = self.bits_off, self.bits_off + self.bits_cap
        spans = [("below work", 0, w0), ("above work", w1, w1 + GUARD), ("below bits", w1 + GUARD, b0),
                 ("above bits", b1, self.size)]
        return [(n, host[a:b], self.pattern[a:b]) for n, a, b in spans]

    def untouched(self):
        torch.cuda.synchronize()
        return np.array_equal(self.buf.cpu().numpy(), self.pattern) and int(self.nbits.item()) == -12345


def run_stages(dev, rgb, quality, sub):
    """sp_jpeg_enc_rgb on a packed uint8 [H, W, 3] host image -> everything the call left on the device."""
    from spotter_amd._lib import lib

    L = lib()
    H, W, _ = rgb.shape
    lay = _plan(W, H, quality, sub)
    nmcu = lay.mcux * lay.mcuy
    # the workspace layout, restated: [total int64][offsets int64 x nmcu][bits int32 x nmcu][coefficients, 256-B aligned]
    coef_off = _up(8 + 8 * nmcu + 4 * nmcu, 256)
    assert lay.work_bytes == coef_off + lay.total_blocks * 128 and lay.total_blocks == nmcu * lay.bpm
    ar = Arena(dev, lay)
    px = torch.from_numpy(np.ascontiguousarray(rgb)).to(dev)
    rc = L.sp_jpeg_enc_rgb(px.data_ptr(), W * 3, 3, C.byref(lay), ar.work_ptr, lay.work_bytes, ar.bits_ptr,
                           lay.bits_cap, ar.nbits.data_ptr(), None)
    assert rc == 0, L.sp_last_error()
    torch.cuda.synchronize()
    host = ar.buf.cpu().numpy()
    work = host[ar.work_off:ar.work_off + lay.work_bytes]
    out = types.SimpleNamespace(lay=lay, nmcu=nmcu)
    out.total = int(work[:8].view(np.int64)[0])
    out.off = work[8:8 + 8 * nmcu].view(np.int64)
    out.mbits = work[8 + 8 * nmcu:8 + 12 * nmcu].view(np.int32)
    out.coefs = work[coef_off:].view(np.int16).reshape(-1, 64)
    out.bits = host[ar.bits_off:ar.bits_off + lay.bits_cap]
    out.nbits = int(ar.nbits.item())
    out.guards = ar.guards(host)
    return out


def _first(bad):
    return int(np.flatnonzero(bad)[0])


def check_stages(dev, name):
    from spotter_amd._lib import lib

    ref = ec.reference(name)
    got = run_stages(dev, ref.rgb, ref.quality, ref.sub)
    assert (got.nmcu, got.lay.bpm) == (ref.nmcu, ref.bpm), name
    # jpeg_fdct_kernel
    assert got.coefs.shape == ref.blocks.shape, (name, got.coefs.shape, ref.blocks.shape)
    bad = got.coefs != ref.blocks
    if bad.any():
        b, k = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{name}: {int(bad.sum())} coefficients differ, first in MCU {b // ref.bpm} block "
                             f"{b % ref.bpm} zig-zag {k}: {got.coefs[b, k]} for {ref.blocks[b, k]}")
    # jpeg_mcu_bits_kernel
    bad = got.mbits != ref.mcu_bits
    if bad.any():
        m = _first(bad)
        raise AssertionError(f"{name}: {int(bad.sum())} MCU bit counts differ, first at MCU {m}: {got.mbits[m]} "
                             f"for {ref.mcu_bits[m]}")
    # jpeg_scan_kernel
    bad = got.off != ref.offsets
    if bad.any():
        m = _first(bad)
        raise AssertionError(f"{name}: {int(bad.sum())} MCU offsets differ, first at MCU {m}: {got.off[m]} for "
                             f"{ref.offsets[m]}")
    assert got.total == ref.nbits == got.nbits, (name, got.total, got.nbits, ref.nbits)
    # jpeg_emit_kernel
    nbytes = (ref.nbits + 7) // 8
    want = np.frombuffer(ref.raw, np.uint8)
    assert len(want) == nbytes <= got.lay.bits_cap
    if not np.array_equal(got.bits[:nbytes], want):
        i = _first(np.unpackbits(got.bits[:nbytes]) != np.unpackbits(want))
        m = int(np.searchsorted(ref.offsets, i, side="right")) - 1
        raise AssertionError(f"{name}: the code stream differs from bit {i} on ({ref.nbits} bits), inside MCU {m} "
                             f"(bits {ref.offsets[m]}..{ref.offsets[m] + ref.mcu_bits[m]})")
    if ref.nbits & 7:
        assert got.bits[nbytes - 1] & (0xFF >> (ref.nbits & 7)) == 0, (name, "bits past the stream's end are set")
    for gname, found, before in got.guards:
        bad = found != before
        assert not bad.any(), f"{name}: guard {gname} overwritten, {int(bad.sum())} bytes, first at {_first(bad)}"
    # the host finish over the device's bits
    L = lib()
    cap = L.sp_jpeg_enc_max_bytes(C.byref(got.lay), got.nbits, 0)
    out = C.create_string_buffer(cap)
    n = C.c_int64()
    stream = np.ascontiguousarray(got.bits[:nbytes + 1])
    assert L.sp_jpeg_enc_finish(C.byref(got.lay), stream.ctypes.data, got.nbits, b"", 0, out, cap, C.byref(n)) == 0
    assert out.raw[:n.value] == ref.pillow, f"{name}: {n.value} vs {len(ref.pillow)} bytes"


@pytest.mark.parametrize("h", ec.GEOMETRY_SIZES)
def test_geometry(dev, h):
    """Luma dummy blocks to the right, below and both; the chroma row and column clamps; each subsampling."""
    names = [c[0] for c in ec.geometry_cases() if c[0].startswith(f"geo {h}x")]
    assert len(names) == 27
    for name in names:
        check_stages(dev, name)


@pytest.mark.parametrize("name", [c[0] for c in ec.run_cases()])
def test_steered_runs(dev, name):
    """walk_mcu's 8-zero fast path, 1 / 2 / 3 ZRL codes, a block without EOB, every run 0..15, in both tables."""
    check_stages(dev, name)


@pytest.mark.parametrize("group", ["wb", "by", "rc", "noise"])
def test_saturation(dev, group):
    """Full-amplitude input at quality 100 and 1: the quantiser's uint32 product, DC-difference size 11 and AC size
    10 in both tables."""
    names = [c[0] for c in ec.saturation_cases() if c[0].startswith(f"sat {group} ")]
    assert len(names) >= 4
    for name in names:
        check_stages(dev, name)


@pytest.mark.parametrize("sub", ec.SUBS)
def test_flat_rows_share_words(dev, sub):
    """MCUs of 14 bits (4:4:4): several MCUs OR their codes into each 32-bit word."""
    names = [c[0] for c in ec.flat_cases() if c[0].endswith(f"s{sub}")]
    assert len(names) == len(ec.FLAT_VALUES)
    for name in names:
        if sub == 0:
            assert (ec.reference(name).mcu_bits[1:] == 14).all()
        check_stages(dev, name)


@pytest.mark.parametrize("name", [c[0] for c in ec.mcu_count_cases()])
def test_mcu_counts(dev, name):
    """The workgroup edges of the four kernels (4, 256, and the scan's 1024 threads with chunk 1 / 2 / 3)."""
    check_stages(dev, name)


# ------------------------------------------------------------------------------------------------ input forms


def _pillow(img, quality=-1, sub=-1):
    kw = {k: v for k, v in (("quality", quality), ("subsampling", sub)) if v != -1}
    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img)).save(b, "JPEG", **kw)
    return b.getvalue()


FORM_SIZES = [(17, 33), (8, 8), (40, 71)]


def _forms(dev, img, rng):
    """(label, device tensor [H, W, 3 or 4] showing img) in every form a caller can hand encode()."""
    H, W, _ = img.shape
    x4 = np.concatenate([img, rng.integers(0, 256, (H, W, 1), dtype=np.uint8)], axis=2)
    yield "rgbx", torch.from_numpy(x4).to(dev)
    for pb in (3, 4):
        big = rng.integers(0, 256, (H + 9, W + 11 + (W % 2 == 0), pb), dtype=np.uint8)
        big[3:3 + H, 5:5 + W] = x4[..., :pb]
        view = torch.from_numpy(big).to(dev)[3:3 + H, 5:5 + W]
        assert view.stride(0) > W * pb and view.stride(1) == pb
        if pb == 3:
            assert view.data_ptr() % 2 == 1  # an odd base address
        yield f"crop{pb}", view


def test_four_byte_pixels_and_cropped_views(dev):
    """pixel_bytes == 4 from a device tensor (the fourth byte random), and views x[3:3+H, 5:5+W] of larger 3- and
    4-channel tensors, on the current and on a side stream: Pillow's bytes."""
    from spotter_amd.jpeg import JpegEncoder

    enc = JpegEncoder(dev)
    rng = np.random.default_rng(3)
    side = torch.cuda.Stream(dev)
    for (H, W) in FORM_SIZES:
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        for sub in ec.SUBS:
            want = _pillow(img, 90, sub)
            for label, t in _forms(dev, img, rng):
                assert enc.encode(t, 90, sub) == want, (H, W, sub, label)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    got = enc.encode(t, 90, sub)
                torch.cuda.current_stream(dev).wait_stream(side)
                assert got == want, (H, W, sub, label, "side stream")


def test_reused_and_regrown_buffers(dev):
    """One encoder: a small image before and after one whose workspace and bit buffer exceed the first allocation
    (the small one then runs over the large one's stale coefficients and bits), then two sizes alternating."""
    from spotter_amd.jpeg import JpegEncoder

    enc = JpegEncoder(dev)
    rng = np.random.default_rng(4)
    small = rng.integers(0, 256, (17, 33, 3), dtype=np.uint8)
    large = rng.integers(0, 256, (520, 512, 3), dtype=np.uint8)  # 4:4:4: 12480 blocks, 1.6 MB of coefficients
    other = rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)
    ts, tl, to = (torch.from_numpy(a).to(dev) for a in (small, large, other))
    want_s, want_l, want_o = _pillow(small), _pillow(large, 100, 0), _pillow(other, 100, 0)
    assert enc.encode(ts) == want_s
    first = enc._work.data_ptr(), enc._bits.data_ptr()
    assert enc.plan(512, 520, 100, 0).work_bytes > enc._work.numel()
    assert enc.encode(tl, 100, 0) == want_l
    assert (enc._work.data_ptr(), enc._bits.data_ptr()) != first
    assert enc.encode(ts) == want_s
    for _ in range(3):
        assert enc.encode(to, 100, 0) == want_o
        assert enc.encode(ts) == want_s
    assert enc.encode(tl, 100, 0) == want_l


# ------------------------------------------------------------------------------------------ argument checks


def test_argument_checks_refuse_and_touch_nothing(dev):
    """Every refusal returns non-zero, leaves its reason in sp_last_error and writes nothing: work, bits, the
    guards and the bit count keep what they held. The altered layouts and sizes never describe more memory than
    the arena holds."""
    from spotter_amd._lib import SpJpegEncLayout, lib

    L = lib()
    H, W = 17, 33
    img = torch.from_numpy(np.random.default_rng(6).integers(0, 256, (H, W, 3), dtype=np.uint8)).to(dev)
    lay = _plan(W, H, -1, -1)
    ar = Arena(dev, lay)

    def call(rgb=img.data_ptr(), stride=W * 3, pb=3, layout=lay, work=ar.work_ptr, work_bytes=lay.work_bytes,
             bits=ar.bits_ptr, bits_cap=lay.bits_cap, nbits=ar.nbits.data_ptr()):
        return L.sp_jpeg_enc_rgb(rgb, stride, pb, C.byref(layout) if layout is not None else None, work,
                                 work_bytes, bits, bits_cap, nbits, None)

    def altered(field, fn):
        c = SpJpegEncLayout.from_buffer_copy(lay)
        fn(c)
        assert bytes(c) != bytes(lay), field
        return c

    def bump(name, by):
        return lambda c: setattr(c, name, getattr(c, name) + by)

    def poke(name, t, i):
        def f(c):
            getattr(c, name)[t][i] ^= 1
        return f

    refusals = [("null rgb", dict(rgb=None), "null"), ("null layout", dict(layout=None), "null"),
                ("null work", dict(work=None), "null"), ("null bits", dict(bits=None), "null"),
                ("null nbits", dict(nbits=None), "null"),
                ("pixel_bytes 2", dict(pb=2), "pixel_bytes 2"),
                ("pixel_bytes 4 over 3-byte rows", dict(pb=4), "row_stride"),
                ("row_stride below W * pb", dict(stride=W * 3 - 1), "row_stride"),
                ("work one byte short", dict(work_bytes=lay.work_bytes - 1), "too small"),
                ("bits one byte short", dict(bits_cap=lay.bits_cap - 1), "too small"),
                ("work misaligned by 128", dict(work=ar.work_ptr + 128), "aligned"),
                ("bits misaligned by 2", dict(bits=ar.bits_ptr + 2), "aligned")]
    for field, fn in [("quality", bump("quality", 1)), ("width", bump("width", -1)), ("mcux", bump("mcux", -1)),
                      ("wb0", bump("wb0", -1)), ("hb0", bump("hb0", -1)), ("bpm", bump("bpm", -1)),
                      ("total_blocks", bump("total_blocks", -1)), ("work_bytes", bump("work_bytes", -1)),
                      ("bits_cap", bump("bits_cap", -1)), ("quant", poke("quant", 0, 5)),
                      ("recip", poke("recip", 1, 7)), ("corr", poke("corr", 0, 63)), ("shift", poke("shift", 1, 0))]:
        refusals.append((f"layout.{field} altered", dict(layout=altered(field, fn)), "layout is not"))
    for label, kw, reason in refusals:
        rc = call(**kw)
        msg = L.sp_last_error().decode(errors="replace")
        assert rc != 0, label
        assert msg.startswith("sp_jpeg_enc_rgb") and reason in msg, (label, msg)
        assert ar.untouched(), label
    assert call() == 0, L.sp_last_error()  # the unaltered call runs, and writes
    assert not ar.untouched()
