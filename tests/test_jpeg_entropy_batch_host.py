"""CPU: the host half of the batched GPU entropy decode. The table (sp_jpeg_entropy_batch_plan) and the check the
launch chain runs on it (sp_jpeg_entropy_batch_check); the emulation that walks the table workgroup by workgroup as
the kernels do (sp_jpeg_entropy_batch_emulate) against the single-image emulation, which tests/test_jpeg_entropy_host.py
pins to status 0 and the host decoder's coefficients; and JpegDecoder.decode_many's routing on an entropy="gpu" decoder
with host stand-ins for the two device steps, in the style of tests/test_jpeg_batch_host.py."""
import ctypes as C
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
from jpeg_entropy_cases import cases, non_eligible, tail_junk  # noqa: E402

from spotter_amd._lib import (SP_JPEG_BATCH_MAX, SpJpegBatchItem, SpJpegBatchTotals, SpJpegEntropyItem,  # noqa: E402
                              SpJpegEntropyTotals, SpJpegLayout, SpJpegScan, lib)

K_BLOCK, DC_CHUNK = 256, 2  # csrc/jpeg_entropy_core.h kBlock, kDcChunk


def _truncated(data):
    """A scan cut short at 60 % of the file with the EOI put back: still packed, the segment's block count is short."""
    return data[:len(data) * 6 // 10] + b"\xff\xd9"


@pytest.fixture(scope="module")
def packed():
    """name → (layout, scan, package, single-image emulation's coefficients, its status): computed once, read only."""
    from spotter_amd.jpeg import emulate_entropy, pack_scan

    files = list(cases()) + [tail_junk()[i] for i in (0, 57, 203, 349)]
    files.append(("truncated", _truncated(dict(cases())["233x177 sub2"])))
    out = {}
    for name, data in files:
        lay, scan, pkg = pack_scan(data)
        _, co, status, _ = emulate_entropy(data)
        co.setflags(write=False)
        out[name] = (lay, scan, pkg, co, status)
    return out


def _work_bytes(scan, nchunk):
    n = scan.nsub
    return 3 * 16 * n + 8 * (n + 1) + 24 * (nchunk + 1) + (n + 1) // 2 * 8  # jpeg_entropy_core.h work_layout


def _nchunk(scan):
    ri = scan.restart_interval or scan.nmcu
    return -(-scan.nmcu // ri) * -(-ri // DC_CHUNK) if scan.restart_interval else -(-ri // DC_CHUNK)


def _plan(entries, coef_gap=0):
    """(rc, batch items, batch totals, entropy items, entropy totals) of a list of packed() values; coef_gap int16
    elements are left free after every image's coefficient range."""
    n = len(entries)
    lays = (SpJpegLayout * max(n, 1))(*[e[0] for e in entries])
    scans = (SpJpegScan * max(n, 1))(*[e[1] for e in entries])
    bi, bt = (SpJpegBatchItem * max(n, 1))(), SpJpegBatchTotals()
    if 1 <= n <= SP_JPEG_BATCH_MAX:
        assert lib().sp_jpeg_batch_plan(lays, n, bi, C.byref(bt)) == 0, lib().sp_last_error()
        for k in range(n):
            bi[k].coef_off += (k + 1) * coef_gap
        bt.coef_elems += (n + 1) * coef_gap
    ei, et = (SpJpegEntropyItem * max(n, 1))(), SpJpegEntropyTotals()
    rc = lib().sp_jpeg_entropy_batch_plan(scans, lays, bi, n, ei, C.byref(et))
    return rc, bi, bt, ei, et


def _disjoint(ranges, total):
    ranges = sorted(ranges)
    assert ranges[0][0] >= 0 and ranges[-1][1] <= total
    for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
        assert a0 < a1 <= b0 < b1


@pytest.mark.parametrize("n", [1, 2, 7, SP_JPEG_BATCH_MAX])
def test_plan_offsets_and_prefix_columns(packed, n):
    from spotter_amd import jpeg

    names = [nm for nm, _ in cases()]
    entries = [packed[names[(3 * i + n) % len(names)]] for i in range(n)]
    rc, bi, bt, ei, et = _plan(entries)
    assert rc == 0, lib().sp_last_error()
    wg_sub = wg_dc = 0
    for k, (lay, scan, _, _, _) in enumerate(entries):
        it = ei[k]
        assert bytes(it.scan) == bytes(scan) and it.total_blocks == lay.total_blocks
        assert it.pkg_off % 16 == 0 and it.work_off % 16 == 0 and it.coef_off == bi[k].coef_off
        assert it.dc_nchunk == _nchunk(scan)
        assert (it.first_wg_sub, it.first_wg_dc) == (wg_sub, wg_dc)  # exclusive prefix sums of the per-image counts
        wg_sub += -(-scan.nsub // K_BLOCK)
        wg_dc += -(-it.dc_nchunk // 256)
        assert scan.work_bytes == _work_bytes(scan, it.dc_nchunk)  # the single-image call's workspace, per image
        # the sizes decode_many offers the packer first (spotter_amd/jpeg.py) are the packer's own
        assert scan.tab_off == 0 and scan.seg_off + 64 == jpeg._PKG_FIXED
        assert scan.stream_off - scan.seg_off == jpeg._SEG_BYTES * (scan.nseg + 1) and scan.nseg <= scan.nmcu
    assert (et.wg_sub, et.wg_dc) == (wg_sub, wg_dc)
    _disjoint([(it.pkg_off, it.pkg_off + it.scan.pkg_bytes) for it in ei[:n]], et.pkg_bytes)
    _disjoint([(it.work_off, it.work_off + it.scan.work_bytes) for it in ei[:n]], et.work_bytes)
    _disjoint([(it.coef_off, it.coef_off + it.total_blocks * 64) for it in ei[:n]], bt.coef_elems)
    assert lib().sp_jpeg_entropy_batch_check(ei, n, C.byref(et), et.pkg_bytes, et.work_bytes, bt.coef_elems) == 0


def test_plan_refusals(packed):
    L = lib()
    names = [nm for nm, _ in cases()]
    rc = _plan([])[0]
    assert rc == -1 and b"n = 0" in L.sp_last_error()
    rc = _plan([packed[names[i % len(names)]] for i in range(SP_JPEG_BATCH_MAX + 1)])[0]
    assert rc == -1 and f"n = {SP_JPEG_BATCH_MAX + 1}".encode() in L.sp_last_error()
    two = [packed["233x177 sub2"], packed["gray"]]
    rc, bi, bt, ei, et = _plan(two)
    assert rc == 0
    lays, scans = (SpJpegLayout * 2)(*[e[0] for e in two]), (SpJpegScan * 2)(*[e[1] for e in two])
    for args in ((None, lays, bi, 2, ei, C.byref(et)), (scans, None, bi, 2, ei, C.byref(et)),
                 (scans, lays, None, 2, ei, C.byref(et)), (scans, lays, bi, 2, None, C.byref(et)),
                 (scans, lays, bi, 2, ei, None)):
        assert L.sp_jpeg_entropy_batch_plan(*args) == -1 and b"null" in L.sp_last_error()
    bad = (SpJpegScan * 2)(*[e[1] for e in two])
    bad[1].nseg += 1  # no longer what the MCU count and the restart interval give: check_scan's "segment counts"
    assert L.sp_jpeg_entropy_batch_plan(bad, lays, bi, 2, ei, C.byref(et)) == -1
    assert b"image 1: segment counts" in L.sp_last_error()
    short = (SpJpegBatchItem * 2)()
    C.memmove(short, bi, C.sizeof(bi))
    short[1].coef_off -= 1  # image 0's range no longer holds its total_blocks * 64
    assert L.sp_jpeg_entropy_batch_plan(scans, lays, short, 2, ei, C.byref(et)) == -1
    assert b"overlap" in L.sp_last_error() and b"total_blocks * 64" in L.sp_last_error()
    short[1].coef_off += 1
    short[1].lay.total_blocks -= 1
    assert L.sp_jpeg_entropy_batch_plan(scans, lays, short, 2, ei, C.byref(et)) == -1
    assert b"image 1: coefficient range" in L.sp_last_error()
    assert L.sp_jpeg_entropy_batch_plan(scans, lays, bi, 2, ei, C.byref(et)) == 0  # nothing wrong: accepted


def test_check_refuses_a_table_that_is_off_by_one(packed):
    """What sp_jpeg_entropy_batch_decode checks before it launches: a prefix column, an offset, the totals, the
    geometry record, each off by one."""
    L = lib()
    entries = [packed[nm] for nm in ("480x640 sub2", "gray", "restart rows", "17x33 sub0")]
    rc, bi, bt, ei, et = _plan(entries)
    assert rc == 0
    n = len(entries)

    def check(items=ei, tot=et, pkg=None, work=None, coef=None):
        return L.sp_jpeg_entropy_batch_check(items, n, C.byref(tot), et.pkg_bytes if pkg is None else pkg,
                                             et.work_bytes if work is None else work,
                                             bt.coef_elems if coef is None else coef)

    def edited(field, delta, k=2):
        c = (SpJpegEntropyItem * n)()
        C.memmove(c, ei, C.sizeof(ei))
        setattr(c[k], field, getattr(c[k], field) + delta)
        return c

    assert check() == 0
    for field, delta, msg in (("first_wg_sub", 1, b"first workgroups"), ("first_wg_sub", -1, b"first workgroups"),
                              ("first_wg_dc", 1, b"first workgroups"), ("pkg_off", 1, b"package"),
                              ("pkg_off", -16, b"packages of images 1 and 2 overlap"), ("work_off", 8, b"workspace"),
                              ("work_off", -16, b"workspaces of images 1 and 2 overlap"),
                              ("coef_off", -1, b"coefficients of images 1 and 2 overlap"),
                              ("dc_nchunk", 1, b"geometry"), ("total_blocks", 1, b"layout does not match")):
        assert check(items=edited(field, delta)) == -1, (field, delta)
        assert msg in L.sp_last_error(), (field, delta, L.sp_last_error())
    geom = edited("pkg_off", 0)
    geom[0].geom[3] += 1
    assert check(items=geom) == -1 and b"image 0: geometry" in L.sp_last_error()
    for field in ("wg_sub", "wg_dc"):
        tot = SpJpegEntropyTotals.from_buffer_copy(bytes(et))
        setattr(tot, field, getattr(tot, field) + 1)
        assert check(tot=tot) == -1 and b"totals" in L.sp_last_error()
    assert check(pkg=et.pkg_bytes - 16) == -1 and b"package" in L.sp_last_error()
    assert check(work=et.work_bytes - 16) == -1 and b"workspace" in L.sp_last_error()
    assert check(coef=bt.coef_elems - 1) == -1 and b"coefficients" in L.sp_last_error()
    assert L.sp_jpeg_entropy_batch_check(ei, 0, C.byref(et), et.pkg_bytes, et.work_bytes, bt.coef_elems) == -1
    assert L.sp_jpeg_entropy_batch_check(None, n, C.byref(et), et.pkg_bytes, et.work_bytes, bt.coef_elems) == -1


def _aligned(nbytes, fill):
    raw = np.full(nbytes + 16, fill, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + nbytes]


COEF_GAP, WORK_GAP, SENTINEL = 24, 48, 0x5A5A


def _emulate(entries):
    """One batch through sp_jpeg_entropy_batch_emulate with sentinel int16s between the coefficient ranges and guard
    bytes between (and around) the workspace ranges: (coefficients per image, status words)."""
    n = len(entries)
    rc, bi, bt, ei, et = _plan(entries, coef_gap=COEF_GAP)
    assert rc == 0, lib().sp_last_error()
    for k in range(n):
        ei[k].work_off += (k + 1) * WORK_GAP
    work_bytes = et.work_bytes + (n + 1) * WORK_GAP
    pkgs, work = _aligned(et.pkg_bytes, 0xEE), _aligned(work_bytes, 0xA5)
    for k, e in enumerate(entries):
        pkgs[ei[k].pkg_off:ei[k].pkg_off + e[2].size] = e[2]
    coefs = np.full(bt.coef_elems, SENTINEL, np.int16)
    status = np.zeros(n, np.int32)
    rc = lib().sp_jpeg_entropy_batch_emulate(pkgs.ctypes.data, et.pkg_bytes, ei, n, C.byref(et), work.ctypes.data,
                                             work_bytes, coefs.ctypes.data, coefs.size, status.ctypes.data)
    assert rc == 0, lib().sp_last_error()
    rest, wrest = np.ones(coefs.size, bool), np.ones(work.size, bool)
    got = []
    for k in range(n):
        a, b = ei[k].coef_off, ei[k].coef_off + ei[k].total_blocks * 64
        got.append(coefs[a:b].reshape(-1, 64))
        rest[a:b] = False
        wrest[ei[k].work_off:ei[k].work_off + ei[k].scan.work_bytes] = False
    assert rest.sum() == (n + 1) * COEF_GAP and (coefs[rest] == SENTINEL).all()
    assert wrest.sum() >= (n + 1) * WORK_GAP and (work[wrest] == 0xA5).all()
    return got, status.tolist()


@pytest.mark.parametrize("order", ["forward", "reversed"])
def test_batch_emulation_equals_the_single_image_one(packed, order):
    names = [nm for nm, _ in cases()]
    if order == "reversed":
        names = names[::-1]
    got, status = _emulate([packed[nm] for nm in names])
    for nm, co, st in zip(names, got, status):
        _, _, _, ref, ref_st = packed[nm]
        assert st == ref_st == 0, nm
        bad = np.argwhere(co != ref)
        assert bad.size == 0, f"{nm}: {len(bad)} coefficients differ, first at {bad[:3].tolist()}"


def test_mixed_batch_keeps_status_and_damage_to_their_image(packed):
    """Files with bytes after their last block and a truncated scan among good ones, a one-subsequence gray image
    directly before and after a multi-workgroup colour one: only their own status words are non-zero, and every
    image's coefficients and status are what it gives alone."""
    junk = [nm for nm in packed if "_before_" in nm]
    names = ["gray", "480x640 sub2", "gray", junk[0], "restart rows", "truncated", "1x1 sub0", junk[1], junk[2],
             "restart 1 mcu", junk[3], "shorter than a subsequence"]
    got, status = _emulate([packed[nm] for nm in names])
    assert packed["gray"][1].nsub < K_BLOCK < packed["480x640 sub2"][1].nsub and packed["480x640 sub2"][1].nsub % K_BLOCK
    for nm, co, st in zip(names, got, status):
        _, _, _, ref, ref_st = packed[nm]
        assert st == ref_st and (st != 0) == (nm in junk or nm == "truncated"), (nm, st, ref_st)
        assert np.array_equal(co, ref), nm


# ------------------------------------------------------------------------------- decode_many's routing, on the host
def _stand_in(entropy="gpu"):
    """A JpegDecoder without a device: the GPU chunk's device half is the batch emulation (its "arena" a host tensor
    that holds each image's index), the host chunk records what it was given."""
    from spotter_amd import jpeg

    class StandIn(jpeg.JpegDecoder):
        def __init__(self):
            self.entropy = entropy
            self.batch_stats = jpeg._new_batch_stats()
            self._lock, self._workers = threading.Lock(), None
            self.gpu_chunks, self.host_chunks, self.uploads = [], [], []

        def _run_gpu_entropy_chunk(self, L, pkgs, ent, etot, items, totals):
            n = len(pkgs)
            buf, work = _aligned(etot.pkg_bytes, 0), _aligned(etot.work_bytes, 0)
            for k, p in enumerate(pkgs):
                buf[ent[k].pkg_off:ent[k].pkg_off + ent[k].scan.pkg_bytes] = p[:ent[k].scan.pkg_bytes]
            coefs, status = np.zeros(totals.coef_elems, np.int16), np.zeros(n, np.int32)
            assert L.sp_jpeg_entropy_batch_emulate(buf.ctypes.data, etot.pkg_bytes, ent, n, C.byref(etot),
                                                   work.ctypes.data, etot.work_bytes, coefs.ctypes.data, coefs.size,
                                                   status.ctypes.data) == 0, L.sp_last_error()
            arena = torch.zeros(totals.rgb_bytes, dtype=torch.uint8)
            for k in range(n):
                it = items[k]
                arena[it.rgb_off:it.rgb_off + 3 * it.lay.width * it.lay.height] = k + 1
            self.gpu_chunks.append([(it.lay.width, it.lay.height) for it in items])
            return arena, status.tolist(), etot.pkg_bytes + C.sizeof(ent) + C.sizeof(items)

        def _decode_chunk(self, L, idx, bufs, lays, out, workers):
            self.host_chunks.append(list(idx))
            self.batch_stats["chunks"] += 1
            self.batch_stats["images"] += len(idx)
            for i in idx:
                out[i] = ("host", i, lays[i].width, lays[i].height)

    return StandIn()


def test_decode_many_routes_files_and_restores_the_order(packed, monkeypatch):
    from spotter_amd import jpeg

    monkeypatch.setattr(jpeg, "PACK_POOL_BYTES", 0)  # with 3 workers the scans are packed in the pool
    good = dict(cases())
    files = [good["17x33 sub1"], non_eligible()[0][1], good["gray"], tail_junk()[0][1], b"not a jpeg at all",
             good["233x177 sub2"], non_eligible()[2][1], _truncated(good["233x177 sub2"]), good["restart rows"],
             good["233x177 sub2"][:len(good["233x177 sub2"]) * 8 // 10]]  # no EOI: the packer refuses it outright
    for workers in (1, 3):
        d = _stand_in()
        out = d.decode_many(files, max_workers=workers)
        from spotter_amd.jpeg import UnsupportedJpeg

        kinds = ["gpu", "host", "gpu", "host", "refused", "gpu", "host", "host", "gpu", "host"]
        for i, (o, kind) in enumerate(zip(out, kinds)):
            if kind == "gpu":
                lay = packed[[nm for nm, b in cases() if b == files[i]][0]][0]
                assert torch.is_tensor(o) and tuple(o.shape) == (lay.height, lay.width, 3), i
                assert int(o.min()) == int(o.max()) == [k for k, j in enumerate((0, 2, 3, 5, 7, 8)) if j == i][0] + 1
            elif kind == "host":
                assert o[:2] == ("host", i), i
            else:
                assert isinstance(o, UnsupportedJpeg)
        # the eligible files formed one GPU chunk in input order, flagged ones included; the host chunk got the two
        # files that are not eligible, the two the status word sent back and the one the packer refused, in input
        # order; "host" counts the not eligible ones only (the real host chunk counts a refusal as "refused")
        assert len(d.gpu_chunks) == 1 and len(d.gpu_chunks[0]) == 6
        assert d.host_chunks == [[1, 3, 6, 7, 9]]
        st = d.batch_stats
        assert st["gpu"] == 4 and st["host"] == 2 and sum(st["fallback"].values()) == 2 and all(st["fallback"])
        assert st["calls"] == 1 and st["chunks"] == 2 and st["images"] == 9 and st["refused"] == 1
        assert st["h2d_bytes"] > 0


def test_decode_many_chunks_by_count_and_budget(packed, monkeypatch):
    from spotter_amd import jpeg

    good = dict(cases())
    small, mid = good["2x3 sub0"], good["233x177 sub2"]
    d = _stand_in()
    out = d.decode_many([small if i % 2 else good["1x1 sub2"] for i in range(SP_JPEG_BATCH_MAX + 6)], max_workers=2)
    assert [len(c) for c in d.gpu_chunks] == [SP_JPEG_BATCH_MAX, 6] and not d.host_chunks
    assert all(torch.is_tensor(o) for o in out) and d.batch_stats["chunks"] == 2
    lay, scan = packed["233x177 sub2"][:2]
    budgets = {"KEEP_ARENA": (3 * lay.width * lay.height + 255) & ~255, "KEEP_COEFS": lay.total_blocks * 64,
               "KEEP_WORK": (lay.plane_bytes + 15) & ~15}
    for name, per_image in budgets.items():
        d = _stand_in()
        monkeypatch.setattr(jpeg, name, 3 * per_image + 1)  # three such files fit, a fourth does not
        d.decode_many([mid] * 7 + [small], max_workers=1)
        assert [len(c) for c in d.gpu_chunks] == [3, 3, 2], name
        monkeypatch.undo()
    # chunks that straddle the packing windows of SP_JPEG_BATCH_MAX files are the same greedy chunks
    d = _stand_in()
    monkeypatch.setattr(jpeg, "KEEP_ARENA", 3 * budgets["KEEP_ARENA"] + 1)
    out = d.decode_many([mid] * 130, max_workers=1)
    assert [len(c) for c in d.gpu_chunks] == [3] * 43 + [1] and all(torch.is_tensor(o) for o in out)
    monkeypatch.undo()
    d = _stand_in()
    monkeypatch.setattr(jpeg, "KEEP_PKG", 2 * ((scan.pkg_bytes + 15) & ~15) + jpeg._ENT_TABLE_BYTES + 1)
    d.decode_many([mid] * 5, max_workers=1)  # two packages and the tables fit the package buffer
    assert [len(c) for c in d.gpu_chunks] == [2, 2, 1]
    monkeypatch.setattr(jpeg, "KEEP_PKG", 16)  # a file beyond the budgets runs alone
    d = _stand_in()
    d.decode_many([mid, small, mid], max_workers=1)
    assert [len(c) for c in d.gpu_chunks] == [1, 1, 1]


def test_host_chunker_chunks_by_its_three_budgets(packed, monkeypatch):
    """The host-entropy chunker's own budgets: KEEP_ARENA, KEEP_WORK, and KEEP_COEFS less the table that travels
    behind the coefficients (jpeg._TABLE_ELEMS)."""
    from spotter_amd import jpeg

    good = dict(cases())
    small, mid = good["2x3 sub0"], good["233x177 sub2"]
    lay = packed["233x177 sub2"][0]
    budgets = {"KEEP_ARENA": (3 * lay.width * lay.height + 255) & ~255, "KEEP_COEFS": lay.total_blocks * 64,
               "KEEP_WORK": (lay.plane_bytes + 15) & ~15}
    reserve = {"KEEP_ARENA": 0, "KEEP_COEFS": jpeg._TABLE_ELEMS, "KEEP_WORK": 0}
    for name, per_image in budgets.items():
        d = _stand_in(entropy="host")
        monkeypatch.setattr(jpeg, name, 3 * per_image + reserve[name] + 1)  # three such files fit, a fourth does not
        d.decode_many([mid] * 7 + [small], max_workers=1)
        assert [len(c) for c in d.host_chunks] == [3, 3, 2], name
        assert d.host_chunks == [[0, 1, 2], [3, 4, 5], [6, 7]] and not d.gpu_chunks, name
        monkeypatch.undo()
        # a file beyond the budget runs as a chunk of its own, between chunks of files that fit
        d = _stand_in(entropy="host")
        monkeypatch.setattr(jpeg, name, per_image + reserve[name] - 1)
        d.decode_many([small, small, mid, small], max_workers=1)
        assert d.host_chunks == [[0, 1], [2], [3]], name
        monkeypatch.undo()


def test_two_threads_with_different_pool_sizes_share_one_decoder(monkeypatch):
    """The pack phase uses the decoder's pool and counters under the decoder's lock: two callers that ask for
    different pool sizes (each replaces the executor) do not meet a shut-down pool or lose a count."""
    from spotter_amd import jpeg

    monkeypatch.setattr(jpeg, "PACK_POOL_BYTES", 0)
    files = [dict(cases())[nm] for nm in ("17x33 sub1", "gray", "2x3 sub0")] + [non_eligible()[0][1]]
    d, errors = _stand_in(), []

    def work(workers):
        try:
            for _ in range(12):
                out = d.decode_many(files, max_workers=workers)
                assert [torch.is_tensor(o) for o in out] == [True, True, True, False]
        except Exception as e:  # noqa: BLE001 - reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(w,)) for w in (2, 3)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert d.batch_stats["gpu"] == 72 and d.batch_stats["host"] == 24 and d.batch_stats["calls"] == 24


def test_a_host_decoder_never_packs(monkeypatch):
    d = _stand_in(entropy="host")
    monkeypatch.setattr(d, "_decode_many_gpu_entropy", None)  # calling it would raise
    out = d.decode_many([dict(cases())["gray"], non_eligible()[0][1]], max_workers=1)
    assert [o[:2] for o in out] == [("host", 0), ("host", 1)] and d.host_chunks == [[0, 1]]
    assert d.batch_stats["gpu"] == d.batch_stats["host"] == 0 and d.batch_stats["fallback"] == {}


def test_bulk_cli_and_detector_take_the_entropy_mode(tmp_path, monkeypatch):
    from spotter_amd import bulk

    seen = []

    class Det:
        def detect(self, files):
            return iter(())

    def make(args):
        seen.append(args.jpeg_entropy)
        return Det(), {}

    base = ["--model", "synthetic:r18vd", "--out", str(tmp_path / "o.jsonl"), str(tmp_path)]
    monkeypatch.delenv("SPOTTER_JPEG_ENTROPY", raising=False)
    assert bulk.main(base, make_detector=make) == 0
    assert bulk.main(["--jpeg-entropy", "gpu"] + base, make_detector=make) == 0
    monkeypatch.setenv("SPOTTER_JPEG_ENTROPY", "auto")
    assert bulk.main(base, make_detector=make) == 0
    assert seen == ["host", "gpu", "auto"]
    with pytest.raises(SystemExit):
        bulk.main(["--jpeg-entropy", "fpga"] + base, make_detector=make)
    assert bulk.BulkDetector(None, None, jpeg_entropy="gpu").jpeg_entropy == "gpu"
    assert bulk.BulkDetector(None, None).jpeg_entropy == "host"
    with pytest.raises(ValueError):
        bulk.BulkDetector(None, None, jpeg_entropy="fpga")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_batch_plan_check_and_emulation_are_sanitizer_clean(tmp_path):
    """tools/sanitize/jpeg_entropy_batch.cpp, a stand-alone ASan + UBSan program: one batch of every size from 1 to
    64 of the corrupt corpus's eligible files planned, checked and emulated in exact-size heap blocks, and single
    table rows with one field overwritten by an extreme value, which the check must refuse or the emulation must
    survive."""
    from jpeg_corpus import corpus, pack

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "jpeg_entropy_batch"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(root, "tools", "sanitize", "jpeg_entropy_batch.cpp"), "-o",
                    str(exe)], check=True, timeout=300)
    blob = tmp_path / "corpus.bin"
    blob.write_bytes(pack(corpus()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-4000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    eligible, batches, largest, flagged, rows, refused = (int(x) for x in r.stdout.split())
    assert batches == largest == SP_JPEG_BATCH_MAX  # every size up to the full table, 6 search steps included
    assert eligible > 100 and flagged > 0 and rows > 1000 and refused > rows // 2
