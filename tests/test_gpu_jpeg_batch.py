"""GPU: the batched JPEG decode (sp_jpeg_batch_to_rgb, JpegDecoder.decode_many) against the single-image decode()
and Pillow, bit for bit, and the bulk pipeline (spotter_amd.bulk.BulkDetector) against the composition of the public
one-image calls it replaces."""
import ctypes as C
import io
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
from jpeg_entropy_cases import cases, jpeg, non_eligible  # noqa: E402

from spotter_amd._lib import SP_JPEG_BATCH_MAX, SpJpegBatchItem, SpJpegBatchTotals, SpJpegLayout, lib  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


def _straddlers():
    """Sizes around the kernels' units (one 8x8 block, one MCU, 32 blocks and 1024 pixels per workgroup, the
    4-pixel groups of the colour pass) in every subsampling, and 4:2:0 / 4:2:2 widths whose chroma plane is at
    most 2 samples wide (chroma_at's box-replication branch)."""
    from spotter_amd.synthetic import synthetic_image

    out = []
    for (h, w) in [(1, 1), (7, 9), (8, 8), (16, 16), (17, 33), (65, 40)]:
        img = synthetic_image(h * 5 + w, h, w) if min(h, w) >= 2 else np.full((h, w, 3), 201, np.uint8)
        for sub in (0, 1, 2):
            out.append((f"straddle {h}x{w} sub{sub}", jpeg(img, quality=88, subsampling=sub)))
    for (h, w), sub in [((9, 3), 2), ((9, 4), 2), ((5, 4), 1), ((33, 2), 2)]:
        out.append((f"narrow chroma {h}x{w} sub{sub}", jpeg(synthetic_image(h + w, h, w), quality=92, subsampling=sub)))
    return out


@pytest.fixture(scope="module")
def batch(dev):
    """(name, bytes, Pillow's pixels, decode()'s pixels) of one mixed batch: computed once, read by every test."""
    from spotter_amd.jpeg import JpegDecoder

    d = JpegDecoder(dev)
    files = list(cases()) + list(non_eligible()) + _straddlers()
    assert len(files) <= SP_JPEG_BATCH_MAX  # one chunk
    out = []
    for name, data in files:
        ref = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        one = d.decode(data).cpu().numpy()
        assert np.array_equal(one, ref), name
        ref.setflags(write=False)
        out.append((name, data, ref, one))
    return out


def _same(got, want, name):
    assert torch.is_tensor(got), f"{name}: {got!r}"
    g = got.cpu().numpy()
    assert g.shape == want.shape and g.dtype == np.uint8, name
    bad = np.argwhere(g != want)
    assert bad.size == 0, f"{name}: {len(bad)} samples differ, first at {bad[:3].tolist()}"


def test_decode_many_equals_decode_and_pillow(dev, batch):
    from spotter_amd.jpeg import JpegDecoder

    d = JpegDecoder(dev)
    got = d.decode_many([b for _, b, _, _ in batch])
    assert len(got) == len(batch) and d.batch_stats["chunks"] == 1 and d.batch_stats["images"] == len(batch)
    for g, (name, _, ref, one) in zip(got, batch):
        _same(g, one, name)
        _same(g, ref, name)
        assert g.is_contiguous() and g.device == dev
    # another order: image i's pixels depend on its own table row, not on its neighbours
    perm = np.random.default_rng(5).permutation(len(batch))
    got = d.decode_many([batch[i][1] for i in perm], max_workers=1)
    for g, i in zip(got, perm):
        _same(g, batch[i][2], batch[i][0])
    assert d.stats == {"gpu": 0, "host": 0, "fallback": {}, "h2d_bytes": 0}  # decode()'s counters are not touched


def test_a_call_larger_than_the_cap_is_split(dev, batch):
    from spotter_amd.jpeg import JpegDecoder

    by_name = {name: (data, ref) for name, data, ref, _ in batch}
    pair = [by_name["straddle 8x8 sub0"], by_name["straddle 17x33 sub2"]]
    n = SP_JPEG_BATCH_MAX + 6
    d = JpegDecoder(dev)
    got = d.decode_many([pair[i % 2][0] for i in range(n)])
    assert len(got) == n
    for i, g in enumerate(got):
        _same(g, pair[i % 2][1], f"copy {i}")
    assert d.batch_stats["chunks"] == 2 and d.batch_stats["images"] == n and d.batch_stats["calls"] == 1


def test_status_is_per_image(dev, batch):
    """One file whose coefficients leave the IDCT envelope and one truncated at 80 %: exactly those two entries are
    UnsupportedJpeg, the others are decode()'s pixels."""
    from jpeg_corpus import corpus

    from oracle.jpeg_np import simd_envelope_ok
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg, decode_coefs, layout_dict

    outside = None
    for lab, data in corpus():
        try:
            lay, co = decode_coefs(data)
        except UnsupportedJpeg:
            continue
        if not simd_envelope_ok(co, layout_dict(lay)):
            outside = data
            break
    assert outside is not None
    good = [batch[i] for i in (0, 5, 11, 17, 30)]
    whole = good[2][1]
    files = [good[0][1], outside, good[1][1], good[2][1], whole[:len(whole) * 8 // 10], good[3][1], good[4][1]]
    d = JpegDecoder(dev)
    for data in (files[1], files[4]):
        with pytest.raises(UnsupportedJpeg):
            d.decode(data)
    got = d.decode_many(files)
    assert [isinstance(g, UnsupportedJpeg) for g in got] == [False, True, False, False, True, False, False]
    for g, (name, _, ref, _) in zip([got[i] for i in (0, 2, 3, 5, 6)], good):
        _same(g, ref, name)
    assert d.batch_stats["flagged"] == 1 and d.batch_stats["refused"] == 1


def _direct(dev, batch, names):
    """Coefficients, planned table and totals of a few files, for direct sp_jpeg_batch_to_rgb calls."""
    from spotter_amd.jpeg import decode_coefs

    by_name = {name: (data, ref) for name, data, ref, _ in batch}
    lays, cos, refs = [], [], []
    for nm in names:
        lay, co = decode_coefs(by_name[nm][0])
        lays.append(lay)
        cos.append(co.reshape(-1))
        refs.append(by_name[nm][1])
    n = len(lays)
    items, tot = (SpJpegBatchItem * n)(), SpJpegBatchTotals()
    assert lib().sp_jpeg_batch_plan((SpJpegLayout * n)(*lays), n, items, C.byref(tot)) == 0
    for k in range(n):
        items[k].lay.quant = lays[k].quant
    coefs = torch.from_numpy(np.concatenate(cos)).to(dev)
    return items, tot, coefs, refs


def _table(items, dev):
    raw = np.frombuffer(bytes(items), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(dev)


def _run(items, tot, coefs, coef_elems, table, work, rgb, status):
    return lib().sp_jpeg_batch_to_rgb(coefs.data_ptr(), coef_elems, table.data_ptr() if table is not None else None,
                                      items, len(items), C.byref(tot), work.data_ptr(), work.numel(), rgb.data_ptr(),
                                      rgb.numel(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)


NAMES = ["straddle 17x33 sub2", "straddle 7x9 sub0", "gray", "straddle 65x40 sub1"]


def test_guard_bytes_around_rgb_rows_and_planes(dev, batch):
    """Strided rows (dword-aligned and not) and packed ones, gaps between the images and between the plane sets:
    every byte outside the images' pixels and outside the planned plane ranges keeps its pattern."""
    items, tot, coefs, refs = _direct(dev, batch, NAMES)
    n = len(items)
    rgb_off = work_off = 512
    spans = []
    for k, pad in enumerate((0, 5, 8, 0)):
        it = items[k]
        it.rgb_stride = 3 * it.lay.width + pad
        it.rgb_off, it.work_off = rgb_off, work_off
        spans.append((rgb_off, work_off))
        rgb_off += (it.rgb_stride * it.lay.height + 255 + 256) & ~255
        work_off += ((it.lay.plane_bytes + 15) & ~15) + 48
    rgb = torch.full((rgb_off + 1024,), 0xA5, dtype=torch.uint8, device=dev)
    work = torch.full((work_off + 1024,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    assert _run(items, tot, coefs, coefs.numel(), _table(items, dev), work, rgb, status) == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * n
    got, planes = rgb.cpu().numpy(), work.cpu().numpy()
    rest, wrest = np.ones(got.size, bool), np.ones(planes.size, bool)
    for it, ref in zip(items, refs):
        H, W = it.lay.height, it.lay.width
        for y in range(H):
            a = it.rgb_off + y * it.rgb_stride
            assert np.array_equal(got[a:a + 3 * W], ref[y].reshape(-1)), (W, H, y)
            rest[a:a + 3 * W] = False
        wrest[it.work_off:it.work_off + it.lay.plane_bytes] = False
    assert (got[rest] == 0xA5).all() and (planes[wrest] == 0x5A).all()


def test_argument_refusals_launch_nothing(dev, batch):
    items, tot, coefs, _ = _direct(dev, batch, NAMES)
    n = len(items)
    L = lib()
    rgb = torch.full((tot.rgb_bytes,), 0xA5, dtype=torch.uint8, device=dev)
    work = torch.full((tot.work_bytes,), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.zeros(n, dtype=torch.int32, device=dev)
    table = _table(items, dev)

    def copy():
        c = (SpJpegBatchItem * n)()
        C.memmove(c, items, C.sizeof(items))
        return c

    overlap = copy()
    overlap[2].rgb_off = overlap[1].rgb_off
    assert _run(overlap, tot, coefs, coefs.numel(), table, work, rgb, status) == -1
    assert b"RGB ranges of images 1 and 2 overlap" in L.sp_last_error()
    assert _run(items, tot, coefs, coefs.numel() - 1, table, work, rgb, status) == -1
    assert b"coefficients" in L.sp_last_error() and b"outside" in L.sp_last_error()
    assert _run(items, tot, coefs, coefs.numel(), table, work[:tot.work_bytes - 16], rgb, status) == -1
    assert b"planes" in L.sp_last_error()
    narrow = copy()
    narrow[0].rgb_stride = 3 * narrow[0].lay.width - 1
    assert _run(narrow, tot, coefs, coefs.numel(), table, work, rgb, status) == -1
    assert b"rgb_stride" in L.sp_last_error()
    assert _run(items, tot, coefs, coefs.numel(), None, work, rgb, status) == -1 and b"null" in L.sp_last_error()
    assert L.sp_jpeg_batch_to_rgb(coefs.data_ptr(), coefs.numel(), table.data_ptr(), None, n, C.byref(tot),
                                  work.data_ptr(), work.numel(), rgb.data_ptr(), rgb.numel(), status.data_ptr(),
                                  None) == -1 and b"null" in L.sp_last_error()
    torch.cuda.synchronize()
    assert (rgb == 0xA5).all() and (work == 0x5A).all() and not status.any()
    assert _run(items, tot, coefs, coefs.numel(), table, work, rgb, status) == 0  # the unmodified call is accepted
    torch.cuda.synchronize()


def test_two_decoders_on_two_streams(dev, batch):
    from spotter_amd.jpeg import JpegDecoder

    picks = [list(range(0, len(batch), 3)), list(range(1, len(batch), 3))]
    results, errors = [None, None], []

    def work(t):
        try:
            d, s = JpegDecoder(dev), torch.cuda.Stream(dev)
            with torch.cuda.device(dev), torch.cuda.stream(s):
                for _ in range(3):
                    got = d.decode_many([batch[i][1] for i in picks[t]], max_workers=2)
                s.synchronize()
            results[t] = got
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        for g, i in zip(results[t], picks[t]):
            _same(g, batch[i][2], batch[i][0])


def _cap_needs(entropy, datas):
    """What the decoder's run over `datas` (decode() of one file, or one decode_many chunk) asks of each KEEP_* cap,
    and what decode_many's chunker counts against it for these files, from the library's own plans: the staging
    layouts are spotter_amd/jpeg.py's (host entropy: the table behind the coefficients, 16-byte aligned; GPU entropy:
    packages, entropy table, batch table, each 16-byte aligned, and the workspace against KEEP_PKG as well)."""
    from spotter_amd import jpeg
    from spotter_amd._lib import SpJpegEntropyItem, SpJpegEntropyTotals, SpJpegScan

    def a16(v):
        return (v + 15) & ~15

    packed = [jpeg.pack_scan(d) for d in datas]
    lays, scans, n = [p[0] for p in packed], [p[1] for p in packed], len(datas)
    count = {"KEEP_COEFS": sum(lay.total_blocks * 64 for lay in lays),
             "KEEP_WORK": sum(a16(lay.plane_bytes) for lay in lays)}
    larr, items, tot = (SpJpegLayout * n)(*lays), (SpJpegBatchItem * n)(), SpJpegBatchTotals()
    assert lib().sp_jpeg_batch_plan(larr, n, items, C.byref(tot)) == 0, lib().sp_last_error()
    if entropy == "host":
        chunk = {"KEEP_COEFS": ((tot.coef_elems + 7) & ~7) + (C.sizeof(items) + 1) // 2, "KEEP_WORK": tot.work_bytes}
        one = {"KEEP_COEFS": lays[0].total_blocks * 64, "KEEP_WORK": lays[0].plane_bytes}
        count["KEEP_COEFS"] += jpeg._TABLE_ELEMS
    else:
        ent, etot = (SpJpegEntropyItem * n)(), SpJpegEntropyTotals()
        assert lib().sp_jpeg_entropy_batch_plan((SpJpegScan * n)(*scans), larr, items, n, ent, C.byref(etot)) == 0
        nbytes = a16(a16(etot.pkg_bytes) + C.sizeof(ent)) + C.sizeof(items)
        chunk = {"KEEP_PKG": max(nbytes, etot.work_bytes), "KEEP_COEFS": tot.coef_elems, "KEEP_WORK": tot.work_bytes}
        one = {"KEEP_PKG": max(scans[0].pkg_bytes, scans[0].work_bytes), "KEEP_COEFS": lays[0].total_blocks * 64,
               "KEEP_WORK": lays[0].plane_bytes}
        count["KEEP_PKG"] = max(sum(a16(s.pkg_bytes) for s in scans) + jpeg._ENT_TABLE_BYTES,
                                sum(a16(s.work_bytes) for s in scans))
    return one, chunk, count


@pytest.mark.parametrize("entropy", ["host", "gpu"])
@pytest.mark.parametrize("form", ["decode", "decode_many"])
def test_caps_exactly_met_keep_the_buffers_and_one_less_takes_temporaries(dev, monkeypatch, form, entropy):
    """The KEEP_* caps at exactly what a call needs (the kept buffers serve it) and one less, each cap in turn (the
    call, or in decode_many the larger file as a chunk of its own, runs through buffers of that call): the pixels
    and the path counted are the normal decode's, the kept buffers are neither replaced nor added to, and the
    decoder decodes normally afterwards."""
    from spotter_amd import jpeg

    by_name = dict(cases())
    a, b = by_name["233x177 sub2"], by_name["17x33 sub1"]
    d = jpeg.JpegDecoder(dev, entropy=entropy)
    st = d.stats if form == "decode" else d.batch_stats
    counted = ("gpu", "host") if form == "decode" else ("gpu", "host", "images", "refused", "flagged")
    kept_flags, take = [], d._take

    def spy(need):
        got = take(need)
        kept_flags.append(got[1])
        return got

    d._take = spy  # which of its store's two branches every run took

    def run(files):
        del kept_flags[:]
        before = dict(st)
        got = [d.decode(files[0])] if form == "decode" else d.decode_many(files, max_workers=1)
        assert st["fallback"] == {} and all(torch.is_tensor(g) for g in got), (st, got)
        return got, {k: st[k] - before[k] for k in counted}, st.get("chunks", 0) - before.get("chunks", 0)

    def ptrs():
        return {k: t.data_ptr() for k, t in d._kept.items()}

    def same(got, want, what):
        assert len(got[0]) == len(want[0]) and got[1] == want[1], (what, got[1], want[1])
        for g, w in zip(got[0], want[0]):
            assert g.shape == w.shape and torch.equal(g, w), what

    for files in ([[a], [b]] if form == "decode" else [[a, b]]):
        want = run(files)
        assert all(kept_flags) and want[1]["gpu"] == (len(files) if entropy == "gpu" else 0), (kept_flags, want[1])
        one, chunk, count = _cap_needs(entropy, files)
        exact = one if form == "decode" else {k: max(chunk[k], count[k]) for k in chunk}
        # (in decode_many one less than the call needs only splits the chunk: one less than the first file needs alone
        # is what sends a run through temporaries)
        less = one if form == "decode" else _cap_needs(entropy, files[:1])[1]
        held = ptrs()
        for name, v in exact.items():
            monkeypatch.setattr(jpeg, name, v)
        got = run(files)
        same(got, want, ("exact", exact))
        assert all(kept_flags) and got[2] == want[2] and ptrs() == held, (kept_flags, got[2], exact)
        monkeypatch.undo()
        for name, v in less.items():
            monkeypatch.setattr(jpeg, name, v - 1)
            got = run(files)
            same(got, want, (name, v - 1))
            assert not all(kept_flags) and ptrs() == held, (name, v - 1, kept_flags)
            assert got[2] == (0 if form == "decode" else 2), (name, got[2])  # the larger file ran alone
            monkeypatch.undo()
            got = run(files)
            same(got, want, ("after", name))
            assert all(kept_flags) and got[2] == want[2] and ptrs() == held, (name, kept_flags)


class _Recording:
    """A processor that keeps the pixel_values it produced."""

    def __init__(self, proc):
        self.proc, self.seen = proc, []

    def __call__(self, *a, **kw):
        out = self.proc(*a, **kw)
        self.seen.append(out["pixel_values"])
        return out

    def post_process_object_detection(self, *a, **kw):
        return self.proc.post_process_object_detection(*a, **kw)


def test_bulk_detector_equals_the_public_calls(dev):
    """R18vd synthetic, fp32, batch 2 over [JPEG, PNG, corrupt, JPEG, JPEG]: chunk by chunk, the pipeline's
    pixel_values are the stacked one-image processor outputs, and its detections are those of model + post-process
    on that stack, bit for bit."""
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.bulk import BulkDetector
    from spotter_amd.config import PRESETS
    from spotter_amd.jpeg import open_image
    from spotter_amd.synthetic import synthetic_image

    imgs = [synthetic_image(41, 120, 200), synthetic_image(42, 233, 177), synthetic_image(43, 64, 96)]
    jpegs = [jpeg(imgs[0], quality=90, subsampling=2), jpeg(imgs[1], quality=85, subsampling=0),
             jpeg(imgs[2], quality=80, subsampling=1, progressive=True)]
    b = io.BytesIO()
    Image.fromarray(synthetic_image(44, 50, 70)).save(b, "PNG")
    files = [jpegs[0], b.getvalue(), b"\xff\xd8\xff\xe0 not a picture", jpegs[1], jpegs[2]]
    model = SpotterForObjectDetection(PRESETS["r18vd"], precision="fp32", use_graphs=False)
    proc = SpotterImageProcessor()
    rec = _Recording(proc)
    got = list(BulkDetector(model, rec, batch=2, threshold=0.0).detect(files))
    assert len(got) == 5 and set(got[2]) == {"error"}
    chunks = [[0, 1], [3], [4]]  # the corrupt file left its chunk
    assert len(rec.seen) == len(chunks)
    for idx, px in zip(chunks, rec.seen):
        ims = [open_image(files[i]).convert("RGB") for i in idx]
        stack = torch.cat([proc(images=im)["pixel_values"] for im in ims])
        assert torch.equal(stack, px)
        with torch.no_grad():
            out = model(pixel_values=stack)
        sizes = [(im.size[1], im.size[0]) for im in ims]
        want = proc.post_process_object_detection(out, threshold=0.0, target_sizes=sizes)
        for i, w, (h, wd) in zip(idx, want, sizes):
            assert got[i]["size"] == (wd, h) and len(w["scores"]) > 0
            assert torch.equal(got[i]["labels"], w["labels"])
            assert torch.equal(got[i]["scores"], w["scores"]) and torch.equal(got[i]["boxes"], w["boxes"])
