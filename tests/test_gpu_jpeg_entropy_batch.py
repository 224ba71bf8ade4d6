"""GPU: the batched entropy decode (sp_jpeg_entropy_batch_decode, JpegDecoder(entropy="gpu").decode_many) against the
default decoder's decode(), the host entropy decoder's coefficients and Pillow, bit for bit; which path a file took is
read from decoder.batch_stats. The inputs are tests/jpeg_entropy_cases.py's, the ones the CPU emulation of the same
table walk runs in tests/test_jpeg_entropy_batch_host.py. The shapes are the small ones at which the table logic can
go wrong: a one-subsequence image next to a multi-workgroup one, a partial last workgroup, gray next to colour."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from jpeg_entropy_cases import _segment, cases, jpeg, non_eligible, resistant, tail_junk  # noqa: E402

from spotter_amd._lib import (SP_JPEG_BATCH_MAX, SpJpegBatchItem, SpJpegBatchTotals, SpJpegEntropyItem,  # noqa: E402
                              SpJpegEntropyTotals, SpJpegLayout, SpJpegScan, lib)


@pytest.fixture(scope="module")
def dev():
    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


def _one_subsequence_gray():
    return jpeg(np.full((8, 8), 130, np.uint8), mode="L", quality=50)


def _truncated(data):
    """A scan cut short with the EOI put back: the packer takes it, the host decoder refuses it."""
    return data[:len(data) * 6 // 10] + b"\xff\xd9"


def _outside_envelope(data):
    """The first quantisation table set to 255s: the stream decodes, the dequantised blocks leave the IDCT envelope."""
    p, n = _segment(data, 0xDB)
    assert n >= 67
    b = bytearray(data)
    b[p + 5:p + 5 + 64] = b"\xff" * 64
    return bytes(b)


@pytest.fixture(scope="module")
def want(dev):
    """data → what the default decoder's decode() gives for it (host pixels, or None where it raises UnsupportedJpeg):
    computed once per file, read by every test."""
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg

    d, memo = JpegDecoder(dev), {}

    def get(data):
        if data not in memo:
            try:
                px = d.decode(data).cpu().numpy()
                px.setflags(write=False)
                memo[data] = px
            except UnsupportedJpeg:
                memo[data] = None
        return memo[data]

    return get


def _same(got, ref, name):
    assert torch.is_tensor(got), f"{name}: {got!r}"
    g = got.cpu().numpy()
    assert g.shape == ref.shape and g.dtype == np.uint8, name
    bad = np.argwhere(g != ref)
    assert bad.size == 0, f"{name}: {len(bad)} samples differ, first at {bad[:3].tolist()}"


def test_mixed_batch_equals_decode_and_pillow(dev, want):
    from spotter_amd.jpeg import JpegDecoder

    files = list(cases()) + list(non_eligible()) + list(resistant())
    assert len(files) <= SP_JPEG_BATCH_MAX
    d = JpegDecoder(dev, entropy="gpu")
    for order in (np.arange(len(files)), np.random.default_rng(7).permutation(len(files))):
        got = d.decode_many([files[i][1] for i in order], max_workers=2)
        assert len(got) == len(files)
        for g, i in zip(got, order):
            name, data = files[i]
            _same(g, want(data), name)
            _same(g, np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), name)
            assert g.is_contiguous() and g.device == dev
    st = d.batch_stats
    assert st["gpu"] >= 2 * len(cases()) and st["host"] >= 2 * len(non_eligible()), st
    assert st["gpu"] + st["host"] + sum(st["fallback"].values()) == 2 * len(files) == st["images"], st
    assert st["calls"] == 2 and st["refused"] == st["flagged"] == 0
    assert d.stats == {"gpu": 0, "host": 0, "fallback": {}, "h2d_bytes": 0}  # decode()'s counters are not touched


PKG_GAP, WORK_GAP, COEF_GAP, SENTINEL = 32, 48, 24, 0x5A5A


class _Direct:
    """The arguments of a direct sp_jpeg_entropy_batch_decode call over `datas`, with guard bytes around every
    package and workspace range and sentinel int16s around every coefficient range."""

    def __init__(self, dev, datas):
        from spotter_amd.jpeg import pack_scan

        self.n = n = len(datas)
        packed = [pack_scan(d) for d in datas]
        lays, scans = (SpJpegLayout * n)(*[p[0] for p in packed]), (SpJpegScan * n)(*[p[1] for p in packed])
        self.bi, self.bt = (SpJpegBatchItem * n)(), SpJpegBatchTotals()
        assert lib().sp_jpeg_batch_plan(lays, n, self.bi, C.byref(self.bt)) == 0
        for k in range(n):
            self.bi[k].coef_off += (k + 1) * COEF_GAP
        self.coef_elems = self.bt.coef_elems + (n + 1) * COEF_GAP
        self.items, self.tot = (SpJpegEntropyItem * n)(), SpJpegEntropyTotals()
        assert lib().sp_jpeg_entropy_batch_plan(scans, lays, self.bi, n, self.items, C.byref(self.tot)) == 0
        for k in range(n):
            self.items[k].pkg_off += (k + 1) * PKG_GAP
            self.items[k].work_off += (k + 1) * WORK_GAP
        self.pkg_bytes = self.tot.pkg_bytes + (n + 1) * PKG_GAP
        self.work_bytes = self.tot.work_bytes + (n + 1) * WORK_GAP
        host = np.full(self.pkg_bytes, 0xEE, np.uint8)
        for k, p in enumerate(packed):
            host[self.items[k].pkg_off:self.items[k].pkg_off + p[2].size] = p[2]
        self.pkgs_host = host
        self.pkgs = torch.from_numpy(host).to(dev)
        self.work = torch.full((self.work_bytes,), 0xA5, dtype=torch.uint8, device=dev)
        self.coefs = torch.full((self.coef_elems,), SENTINEL, dtype=torch.int16, device=dev)
        self.status = torch.zeros(n, dtype=torch.int32, device=dev)
        self.table = torch.from_numpy(np.frombuffer(bytes(self.items), dtype=np.uint8).copy()).to(dev)

    def run(self, items=None, tot=None, pkg_bytes=None, work_bytes=None, coef_elems=None):
        return lib().sp_jpeg_entropy_batch_decode(
            self.pkgs.data_ptr(), self.pkg_bytes if pkg_bytes is None else pkg_bytes, self.table.data_ptr(),
            self.items if items is None else items, self.n, C.byref(self.tot if tot is None else tot),
            self.work.data_ptr(), self.work_bytes if work_bytes is None else work_bytes, self.coefs.data_ptr(),
            self.coef_elems if coef_elems is None else coef_elems, self.status.data_ptr(),
            torch.cuda.current_stream().cuda_stream)

    def check(self, datas, names):
        """Status 0 and the host entropy decoder's coefficients per image; every byte outside the ranges unchanged."""
        from spotter_amd.jpeg import decode_coefs

        torch.cuda.synchronize()
        assert self.status.cpu().tolist() == [0] * self.n
        co, work = self.coefs.cpu().numpy(), self.work.cpu().numpy()
        rest, wrest = np.ones(co.size, bool), np.ones(work.size, bool)
        for k, (data, name) in enumerate(zip(datas, names)):
            it = self.items[k]
            a, b = it.coef_off, it.coef_off + it.total_blocks * 64
            ref = decode_coefs(data)[1]
            bad = np.argwhere(co[a:b].reshape(-1, 64) != ref)
            assert bad.size == 0, f"{name} (image {k}): {len(bad)} coefficients differ, first at {bad[:3].tolist()}"
            rest[a:b] = False
            wrest[it.work_off:it.work_off + it.scan.work_bytes] = False
        assert rest.sum() == (self.n + 1) * COEF_GAP and (co[rest] == SENTINEL).all()
        assert wrest.sum() >= (self.n + 1) * WORK_GAP and (work[wrest] == 0xA5).all()
        assert np.array_equal(self.pkgs.cpu().numpy(), self.pkgs_host)


def test_device_coefficients_equal_the_host_decoders(dev):
    names, datas = [nm for nm, _ in cases()], [d for _, d in cases()]
    call = _Direct(dev, datas)
    assert call.run() == 0, lib().sp_last_error()
    call.check(datas, names)


def test_neighbours_do_not_reach_into_each_other(dev):
    """A one-subsequence gray image directly before and after a multi-workgroup colour image whose last workgroup is
    partial, a restart file in between: the image-local Xprev[i - 1], the 2 x ncomp table staging, the stream clamp."""
    from spotter_amd.jpeg import pack_scan

    by = dict(cases())
    tiny, big, rst = _one_subsequence_gray(), by["480x640 sub2"], by["restart rows"]
    assert pack_scan(tiny)[1].nsub == 1 and pack_scan(big)[1].nsub > 2 * 256 and pack_scan(big)[1].nsub % 256
    datas = [tiny, big, tiny, rst, big, tiny]
    call = _Direct(dev, datas)
    assert call.run() == 0, lib().sp_last_error()
    call.check(datas, ["tiny gray", "480x640 sub2", "tiny gray", "restart rows", "480x640 sub2", "tiny gray"])


def test_status_is_per_image(dev, want):
    """Files with bytes after their last block, a truncated scan and a file outside the IDCT envelope between good
    files: those, and only those, come back through the host chunk, with the host path's pixels or UnsupportedJpeg."""
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg

    by = dict(cases())
    good = [by[nm] for nm in ("233x177 sub1", "gray", "restart 1 mcu", "17x33 sub2", "noise q100 420")]
    junk = [tail_junk()[i][1] for i in (3, 120, 349)]
    bad = [junk[0], _truncated(by["233x177 sub2"]), junk[1], _outside_envelope(by["17x33 sub0"]), junk[2]]
    files = [good[0], bad[0], good[1], bad[1], bad[2], good[2], good[3], bad[3], bad[4], good[4]]
    assert want(bad[1]) is None and want(bad[3]) is None
    d = JpegDecoder(dev, entropy="gpu")
    got = d.decode_many(files)
    for i, (g, data) in enumerate(zip(got, files)):
        if want(data) is None:
            assert isinstance(g, UnsupportedJpeg), i
        else:
            _same(g, want(data), f"file {i}")
    st = d.batch_stats
    assert st["gpu"] == len(good) and sum(st["fallback"].values()) == len(bad) and st["host"] == 0, st
    assert st["fallback"].get(1) == 1  # the envelope's own bit, from sp_jpeg_batch_to_rgb, alone in its word
    assert st["chunks"] == 2 and st["images"] == len(files)  # one GPU chunk, one host chunk
    assert st["refused"] + st["flagged"] == sum(want(b) is None for b in bad)


def test_a_call_larger_than_the_cap_is_split(dev, want):
    from spotter_amd.jpeg import JpegDecoder

    by = dict(cases())
    pair = [by["2x3 sub1"], by["17x33 sub2"], _one_subsequence_gray()]
    n = SP_JPEG_BATCH_MAX + 6
    d = JpegDecoder(dev, entropy="gpu")
    got = d.decode_many([pair[i % 3] for i in range(n)])
    for i, g in enumerate(got):
        _same(g, want(pair[i % 3]), f"copy {i}")
    st = d.batch_stats
    assert st["chunks"] == 2 and st["gpu"] == st["images"] == n and st["fallback"] == {} and st["host"] == 0


def test_argument_refusals_launch_nothing(dev):
    by = dict(cases())
    datas = [by["233x177 sub2"], by["gray"], by["restart rows"], by["17x33 sub0"]]
    call = _Direct(dev, datas)
    L = lib()

    def edited(field, delta, k=2):
        c = (SpJpegEntropyItem * call.n)()
        C.memmove(c, call.items, C.sizeof(call.items))
        setattr(c[k], field, getattr(c[k], field) + delta)
        return c

    for field, delta, msg in (("first_wg_sub", 1, b"first workgroups"), ("first_wg_dc", -1, b"first workgroups"),
                              ("pkg_off", 1, b"package"), ("work_off", -WORK_GAP - 16, b"workspaces of images"),
                              ("coef_off", -COEF_GAP - 1, b"coefficients of images")):
        assert call.run(items=edited(field, delta)) == -1, field
        assert msg in L.sp_last_error(), (field, L.sp_last_error())
    for field in ("wg_sub", "wg_dc"):
        tot = SpJpegEntropyTotals.from_buffer_copy(bytes(call.tot))
        setattr(tot, field, getattr(tot, field) + 1)
        assert call.run(tot=tot) == -1 and b"totals" in L.sp_last_error()
    last = call.items[call.n - 1]
    assert call.run(pkg_bytes=last.pkg_off + last.scan.pkg_bytes - 1) == -1 and b"package" in L.sp_last_error()
    assert call.run(work_bytes=last.work_off + last.scan.work_bytes - 1) == -1 and b"workspace" in L.sp_last_error()
    assert call.run(coef_elems=last.coef_off + last.total_blocks * 64 - 1) == -1 and b"coefficients" in L.sp_last_error()
    assert L.sp_jpeg_entropy_batch_decode(call.pkgs.data_ptr(), call.pkg_bytes, None, call.items, call.n,
                                          C.byref(call.tot), call.work.data_ptr(), call.work_bytes,
                                          call.coefs.data_ptr(), call.coef_elems, call.status.data_ptr(), None) == -1
    assert b"null" in L.sp_last_error()
    torch.cuda.synchronize()
    assert (call.coefs == SENTINEL).all() and (call.work == 0xA5).all() and not call.status.any()
    assert call.run() == 0, L.sp_last_error()  # the unmodified call is accepted
    call.check(datas, ["233x177 sub2", "gray", "restart rows", "17x33 sub0"])


def test_two_decoders_on_two_streams(dev, want):
    """Two entropy="gpu" decoders, each on its own stream, interleave decode() and decode_many with nothing between
    them but the streams' own order."""
    from spotter_amd.jpeg import JpegDecoder

    by = dict(cases())
    sets = [[by[nm] for nm in ("233x177 sub2", "gray", "restart rows", "480x640 sub0")],
            [by[nm] for nm in ("test_pic baseline", "17x33 sub1", "noise q100", "gray 233x177")]]
    decs = [JpegDecoder(dev, entropy="gpu"), JpegDecoder(dev, entropy="gpu")]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    got = []
    for rep in range(2):
        for w in (0, 1):
            files = sets[(w + rep) % 2]
            with torch.cuda.stream(streams[w]):
                got.append((files[0], decs[w].decode(files[0])))
                got += list(zip(files, decs[w].decode_many(files, max_workers=2)))
                got.append((files[3], decs[w].decode(files[3])))
    torch.cuda.synchronize(dev)
    for k, (data, g) in enumerate(got):
        _same(g, want(data), f"result {k}")
    assert sum(d.batch_stats["gpu"] for d in decs) == 16 and sum(d.stats["gpu"] for d in decs) == 8


def test_bulk_detector_with_a_gpu_entropy_decoder(dev):
    """R18vd synthetic, fp32, batch 2 over [JPEG, PNG, corrupt, progressive JPEG, JPEG]: the pipeline's results with
    an entropy="gpu" decoder equal the default decoder's, bit for bit."""
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.config import PRESETS
    from spotter_amd.jpeg import JpegDecoder
    from spotter_amd.synthetic import synthetic_image

    imgs = [synthetic_image(41, 120, 200), synthetic_image(42, 233, 177), synthetic_image(43, 64, 96)]
    b = io.BytesIO()
    Image.fromarray(synthetic_image(44, 50, 70)).save(b, "PNG")
    files = [jpeg(imgs[0], quality=90, subsampling=2), b.getvalue(), b"\xff\xd8\xff\xe0 not a picture",
             jpeg(imgs[2], quality=80, subsampling=1, progressive=True), jpeg(imgs[1], quality=85, subsampling=0)]
    model = SpotterForObjectDetection(PRESETS["r18vd"], precision="fp32", use_graphs=False)
    proc = SpotterImageProcessor()
    ref = list(BulkDetector(model, proc, batch=2, threshold=0.0).detect(files))
    dec = JpegDecoder(dev, entropy="gpu")
    got = list(BulkDetector(model, proc, batch=2, threshold=0.0, decoder=dec).detect(files))
    assert len(got) == len(ref) == 5 and set(got[2]) == set(ref[2]) == {"error"}
    for i in (0, 1, 3, 4):
        assert got[i]["size"] == ref[i]["size"] and len(ref[i]["scores"]) > 0
        for k in ("scores", "labels", "boxes"):
            assert torch.equal(got[i][k], ref[i][k]), (i, k)
    assert dec.batch_stats["gpu"] == 2 and dec.batch_stats["host"] == 1 and dec.batch_stats["fallback"] == {}
