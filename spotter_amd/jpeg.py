"""JPEG decode in front of the processor: serve.py:96-97 decodes every image on the host with
Pillow (`Image.open(BytesIO(resp.content)).convert("RGB")`); here the Huffman entropy decode runs in the
library's host code (sp_jpeg_decode_coefs, a serial bit stream) and the per-pixel part — dequantisation,
ISLOW IDCT, fancy upsampling, YCbCr→RGB — on the GPU (sp_jpeg_to_rgb), producing the same pixels as
Pillow's libjpeg-turbo, bit for bit (tests/test_jpeg.py, tests/test_gpu_kernels.py).

`JpegDecoder.decode(data)` returns the uint8 [H, W, 3] image on the device, ready for sp_preprocess_u8;
`open_image(data)` is the drop-in for serve.py:96's `Image.open(BytesIO(image_bytes))`: a PIL RGB image (what the unchanged draw / encode tail
needs) that also carries its device copy, which SpotterImageProcessor then uses instead of uploading it
again. JPEG forms the library does not decode (CMYK, 12-bit, arithmetic coding, ...) and other image formats
keep the reference's host decode: UnsupportedJpeg is raised and open_image falls back to Pillow's Image.open for that image.
`JpegDecoder.decode_many(datas)` decodes a list of files together (host entropy decode in a thread pool, one upload,
sp_jpeg_batch_to_rgb's two launches and one status readback per chunk of up to 64 files) with decode()'s outcome per
file; spotter_amd/bulk.py builds the bulk pipeline on it. On an entropy="gpu" decoder the eligible
files of a chunk are entropy-decoded on the device in one launch chain (sp_jpeg_entropy_batch_decode).
`JpegEncoder.encode_many(srcs)` is the encode side of it: a chunk of up to 64 images in sp_jpeg_enc_batch_rgb's six
launches, one readback and one download, every file what encode() returns.

Opt-in (`JpegDecoder(device, entropy="gpu")`, or SPOTTER_JPEG_ENTROPY=gpu for the decoders open_image / image_module
create): baseline files with one interleaved scan are entropy-decoded on the GPU too (sp_jpeg_entropy_pack on the
host, sp_jpeg_entropy_decode on the device); every other file, and every file whose GPU status
word is non-zero, takes the host entropy decode, so the pixels and the exceptions are the same in both modes.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
import types

import numpy as np
import torch

from ._lib import (SP_DRAW_BATCH_MAX, SP_JPEG_BATCH_MAX, SP_JPEG_NOT_ELIGIBLE, SP_JPEG_PKG_SMALL, SP_JPEG_UNSUPPORTED,
                   SpDrawBatchItem, SpJpegBatchItem, SpJpegBatchTotals, SpJpegEncBatchItem, SpJpegEncBatchTotals,
                   SpJpegEncLayout, SpJpegEntropyItem, SpJpegEntropyTotals, SpJpegLayout, SpJpegScan, lib)
from .config import check_jpeg_entropy, jpeg_entropy_from_env


JPEG_MAX_DIMENSION = 65500  # libjpeg's jmorecfg.h limit (csrc/jpeg_host.h SP_JPEG_MAX_DIMENSION)


class UnsupportedJpeg(ValueError):
    """A JPEG form (or another format) the GPU decoder does not implement, or a malformed file: either way the
    bytes go to Pillow, i.e. to the reference's own decoder and its own errors and warnings."""


def _check_pixels(lay) -> None:
    """Pillow's decompression-bomb rule (Image._decompression_bomb_check): above Image.MAX_IMAGE_PIXELS Pillow
    warns, above twice that it raises DecompressionBombError. The GPU path takes neither: such a frame is left
    to Pillow (which then warns or raises exactly as the reference does), and nothing is allocated for it."""
    from PIL import Image

    limit = Image.MAX_IMAGE_PIXELS
    if limit is not None and max(1, lay.width) * max(1, lay.height) > limit:
        raise UnsupportedJpeg(f"{lay.width}x{lay.height} exceeds Image.MAX_IMAGE_PIXELS: left to Pillow")


# decode buffers a JpegDecoder keeps between calls; a larger image gets buffers of its own for that call only
KEEP_COEFS = 1 << 25  # int16 coefficients (64 MiB pinned + 64 MiB device): a 4K 4:4:4 frame fits
KEEP_WORK = 1 << 26   # bytes of component planes
KEEP_PKG = 1 << 26    # bytes of scan package (pinned + device) and of entropy workspace, entropy="gpu"
KEEP_ARENA = 1 << 27  # bytes of RGB a decode_many chunk may produce (its arena is allocated per chunk, not kept)
# int16 elements of the kept coefficient buffer a full decode_many table takes (it travels behind the coefficients)
_TABLE_ELEMS = (SP_JPEG_BATCH_MAX * C.sizeof(SpJpegBatchItem) + 1) // 2 + 8
# bytes both tables of a full GPU-entropy chunk take behind its packages in the package buffer
_ENT_TABLE_BYTES = SP_JPEG_BATCH_MAX * (C.sizeof(SpJpegEntropyItem) + C.sizeof(SpJpegBatchItem)) + 32
# A scan package without its segment table and stream: six Huffman tables (csrc/jpeg_entropy_core.h DevHuff, 4496
# bytes: sp_jpeg_scan.seg_off is 6 of them) and the padding; a segment entry (SegEnt) is 16 bytes. Only the size of the
# buffer the packer is first offered: a wrong guess costs a second pass (SP_JPEG_PKG_SMALL), never a wrong result.
# tests/test_jpeg_entropy_batch_host.py pins both to the packer's own offsets.
_PKG_FIXED = 6 * 4496 + 64
_SEG_BYTES = 16
# File bytes of a decode_many call from which the scans are packed in the thread pool. Packing runs at about 4 GB/s
# on one thread (32 files of 50-120 KB: 0.4 ms), so below this the pool's hand-offs cost more than they spread:
# measured on 32 such files, decode_many ran 1.6-1.75x faster packing on the calling thread.
PACK_POOL_BYTES = 1 << 24
# encode buffers a JpegEncoder keeps between encode_many chunks; a chunk closes before it would pass one of them, and
# a single image beyond one goes through encode(). The packed bit buffer is sized for the worst case (1676 bits a
# block: 2 MiB for 640x640 at 4:2:0, 64 of them 128 MiB); the download takes only the bytes the device found in use.
KEEP_ENC_WORK = 1 << 27  # bytes of encode workspace (coefficients, per-MCU counts and offsets) of a chunk
KEEP_ENC_BITS = 1 << 28  # bytes of packed bit buffer of a chunk
KEEP_ENC_PIX = 1 << 27   # bytes of host pixels (PIL sources) a chunk stages and uploads
# Downloaded segment bytes of a chunk from which sp_jpeg_enc_finish (headers, 0xFF stuffing: a memchr / memcpy pass at
# memory speed) runs in the thread pool; below it the hand-offs cost more than they spread, as with PACK_POOL_BYTES.
FINISH_POOL_BYTES = 1 << 24


def _new_batch_stats() -> dict:
    return {"calls": 0, "chunks": 0, "images": 0, "h2d_bytes": 0, "refused": 0, "flagged": 0, "gpu": 0, "host": 0,
            "fallback": {}}


def _new_enc_stats() -> dict:
    """encode_many's counters: calls, chunks, images encoded in chunks, images handed to encode() (beyond a kept-buffer
    cap), bytes uploaded (table and host pixels) and downloaded (result and segments), stream waits."""
    return {"calls": 0, "chunks": 0, "images": 0, "single": 0, "h2d_bytes": 0, "d2h_bytes": 0, "waits": 0}


def _a16(v: int) -> int:
    return (v + 15) & ~15


def default_decode_workers() -> int:
    """decode_many's default entropy-decode pool size: the CPUs this process may run on, 16 at the most."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _buf(data):
    if isinstance(data, (bytes, bytearray)):
        b = bytes(data)
        return C.cast(C.c_char_p(b), C.c_void_p), len(b), b
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8))
    return a.ctypes.data, a.size, a


def _error(rc, fn, msg=None):
    """The exception for a non-zero return code of the library's `fn`: UnsupportedJpeg for SP_JPEG_UNSUPPORTED, else
    RuntimeError("fn: <last error>"). msg: the error text as read on the thread that made the call (sp_last_error is
    thread-local); None reads it here, on the calling thread."""
    text = (lib().sp_last_error() if msg is None else msg).decode(errors="replace")
    return UnsupportedJpeg(text) if rc == SP_JPEG_UNSUPPORTED else RuntimeError(f"{fn}: {text}")


def _check(rc, fn):
    if rc:
        raise _error(rc, fn)


def _parse(L, ptr, n) -> SpJpegLayout:
    """The header pass: the layout of a file the library decodes, before anything is allocated for it. Raises
    UnsupportedJpeg for a file the parser refuses and for one beyond Pillow's pixel limit."""
    lay = SpJpegLayout()
    _check(L.sp_jpeg_decode_coefs(ptr, n, C.byref(lay), None, 0), "sp_jpeg_decode_coefs")
    _check_pixels(lay)
    return lay


def _pack(L, ptr, n, buf, alloc):
    """sp_jpeg_entropy_pack into `buf`, the buffer that is offered first (a uint8 numpy array or tensor, or None),
    and, when that is too small (SP_JPEG_PKG_SMALL: the packer has filled in the layout and the package's size), a
    second pass into alloc(layout, scan): (return code, layout, scan, the buffer that holds the package)."""
    lay, scan = SpJpegLayout(), SpJpegScan()

    def run(b):
        if b is None:
            return L.sp_jpeg_entropy_pack(ptr, n, C.byref(lay), C.byref(scan), None, 0)
        p, size = (b.data_ptr(), b.numel()) if torch.is_tensor(b) else (b.ctypes.data, b.size)
        return L.sp_jpeg_entropy_pack(ptr, n, C.byref(lay), C.byref(scan), p, size)

    rc = run(buf)
    if rc == SP_JPEG_PKG_SMALL:
        buf = alloc(lay, scan)
        rc = run(buf)
    return rc, lay, scan, buf


def _greedy(needs, caps) -> int:
    """The greedy chunk rule: how many leading entries of `needs` (one tuple of sizes per file, a size per budget in
    `caps`) form the next chunk. As many as fit every budget, SP_JPEG_BATCH_MAX at the most, and one at the least: a
    file beyond a budget runs as a chunk of its own."""
    n, tot = 0, [0] * len(caps)
    for need in needs:
        if n and (n == SP_JPEG_BATCH_MAX or any(t + x > cap for t, x, cap in zip(tot, need, caps))):
            break
        n += 1
        tot = [t + x for t, x in zip(tot, need)]
    return n


def _empty(n, dtype, device):
    """n uninitialised elements on `device`, or in pinned host memory when device is None."""
    if device is None:
        return torch.empty(n, dtype=dtype, pin_memory=True)
    return torch.empty(n, dtype=dtype, device=device)


def _grow(t, n, dtype, device=None, cap=None):
    """t when it holds n elements, else a new buffer (pinned host memory when device is None) of n elements, 1 Mi
    at the least and, where a cap is given (n is within it), `cap` at the most."""
    if t is not None and t.numel() >= n:
        return t
    n = max(n, 1 << 20)
    return _empty(n if cap is None else min(cap, n), dtype, device)


def decode_coefs(data, out: np.ndarray | None = None):
    """Host entropy decode: (layout, int16 coefficients [total_blocks, 64] natural order). out: reuse this
    int16 buffer (e.g. a pinned one) when it is large enough."""
    ptr, n, keep = _buf(data)
    L = lib()
    lay = _parse(L, ptr, n)
    need = lay.total_blocks * 64
    if out is None or out.size < need:
        out = np.empty(need, dtype=np.int16)
    _check(L.sp_jpeg_decode_coefs(ptr, n, C.byref(lay), out.ctypes.data, out.size), "sp_jpeg_decode_coefs")
    del keep
    return lay, out[:need].reshape(-1, 64)


def pack_scan(data):
    """Host half of entropy="gpu": (layout, scan, package bytes as a uint8 array), or None for a file that is not
    eligible (progressive, multi-scan, irregular restarts: it keeps the host entropy decode). Raises
    UnsupportedJpeg where the host parser refuses the file. No device call."""
    ptr, n, keep = _buf(data)

    def alloc(lay, scan):
        _check_pixels(lay)
        return np.zeros(scan.pkg_bytes, dtype=np.uint8)

    rc, lay, scan, pkg = _pack(lib(), ptr, n, None, alloc)
    del keep
    if rc == SP_JPEG_NOT_ELIGIBLE:
        return None
    _check(rc, "sp_jpeg_entropy_pack")
    return lay, scan, pkg[:scan.pkg_bytes]


def emulate_entropy(data):
    """The GPU entropy decode's passes run on the CPU in the kernels' order (sp_jpeg_entropy_emulate): (layout,
    int16 coefficients [total_blocks, 64], status word, (cross-workgroup launches in which an exit state still
    changed, most in-workgroup rounds)), or None for a file that is not eligible."""
    packed = pack_scan(data)
    if packed is None:
        return None
    lay, scan, pkg = packed
    co = np.empty(lay.total_blocks * 64, dtype=np.int16)
    status, rounds = C.c_int32(0), (C.c_int32 * 2)()
    _check(lib().sp_jpeg_entropy_emulate(pkg.ctypes.data, C.byref(scan), C.byref(lay), co.ctypes.data, co.size,
                                         C.byref(status), rounds), "sp_jpeg_entropy_emulate")
    return lay, co.reshape(-1, 64), status.value, (rounds[0], rounds[1])


def layout_dict(lay: SpJpegLayout) -> dict:
    d = {k: getattr(lay, k) for k in ("width", "height", "ncomp", "color", "progressive", "max_h", "max_v",
                                      "total_blocks", "plane_bytes")}
    for k in ("h", "v", "bw", "bh", "block_off", "plane_off"):
        d[k] = list(getattr(lay, k))
    d["quant"] = [list(lay.quant[c]) for c in range(3)]
    return d


def _plan(L, lays):
    """sp_jpeg_batch_plan over the layouts of one chunk: (layout array, table, totals)."""
    n = len(lays)
    arr, items, totals = (SpJpegLayout * n)(*lays), (SpJpegBatchItem * n)(), SpJpegBatchTotals()
    _check(L.sp_jpeg_batch_plan(arr, n, items, C.byref(totals)), "sp_jpeg_batch_plan")
    return arr, items, totals


def _chunk_need(lay):
    """What a file adds to a decode_many chunk: (int16 coefficients, plane bytes, RGB arena bytes), the budgets being
    KEEP_COEFS, KEEP_WORK and KEEP_ARENA."""
    return lay.total_blocks * 64, _a16(lay.plane_bytes), (3 * lay.width * lay.height + 255) & ~255


def _view(arena, it):
    """Image `it` (a table row) of a chunk's RGB arena, as decode() returns it."""
    H, W = it.lay.height, it.lay.width
    return arena[it.rgb_off:it.rgb_off + H * W * 3].view(H, W, 3)


_OUTSIDE = ("coefficients outside the IDCT range shared with libjpeg-turbo's SIMD code (corrupt or crafted data): "
            "left to Pillow")


class JpegDecoder:
    """Per-device decoder state: pinned staging and device buffers, grown as needed up to KEEP_COEFS / KEEP_WORK /
    KEEP_PKG and reused (one decode at a time per decoder; the lock serialises concurrent callers). A larger image
    decodes through buffers allocated for that call and released after it. The four decode forms (one file or a
    chunk, host or GPU entropy) get their buffers from one store (_take) and reach the device through one method
    (_submit), which keeps the event discipline.

    entropy: where the Huffman decode of baseline files runs. "host" (default): sp_jpeg_decode_coefs, the
    coefficients go up. "gpu" / "auto": the host only parses the headers and packs the scan (sp_jpeg_entropy_pack,
    one pass that drops the 0xFF00 stuffing); the package goes up and sp_jpeg_entropy_decode writes the coefficients
    on the device. Files that are not eligible (progressive, multi-scan, irregular restarts) and files whose GPU
    status word comes back non-zero take the host path, so every file gives the host path's pixels or exception.
    `stats` counts the paths: "gpu", "host" (not eligible), "fallback" {status word: count}, "h2d_bytes"."""

    def __init__(self, device, entropy="host"):
        self.dev = torch.device(device)
        self.entropy = check_jpeg_entropy(entropy)
        self.stats = {"gpu": 0, "host": 0, "fallback": {}, "h2d_bytes": 0}
        self.batch_stats = _new_batch_stats()  # decode_many's counters
        self._lock = threading.Lock()
        # The kept buffers by name (_take). Host entropy: the pinned int16 "coefs_host", its device copy "coefs_up"
        # (a chunk's table travels behind the coefficients) and the planes "work_up". GPU entropy: the pinned
        # "pkg_host", its device copy "pkg", the entropy workspace "ent", the coefficients the launch chain writes
        # "coefs" and the planes "work". The two paths keep separate coefficients and planes: a file that falls back
        # to the host path within one call leaves what the GPU chain wrote in place.
        self._kept: dict = {}
        self._copied = None  # event: the last H2D copy out of a kept pinned buffer is done
        self._done = None  # event: the last run's kernels are done with the kept device buffers
        # one status word per image of a chunk (decode() uses the first: sp_jpeg_to_rgb's envelope flag)
        self._status = torch.zeros(SP_JPEG_BATCH_MAX, dtype=torch.int32, device=self.dev)
        self._status_host = torch.zeros(SP_JPEG_BATCH_MAX, dtype=torch.int32, pin_memory=True)
        self._workers = None  # decode_many's entropy-decode pool

    # The names the GPU tests read the device coefficients by after a call: the store itself (`_g["coefs"]`, what the
    # GPU chain wrote) and the host path's uploaded coefficients. Read-only views of `_kept`; nothing here uses them.
    _g = property(lambda self: self._kept)
    _coefs = property(lambda self: self._kept.get("coefs_up"))

    def _take(self, need):
        """The buffers of one run. need: {name: (elements, cap, dtype, device, or None for pinned host memory)};
        returns ({name: buffer}, kept?). All sizes within their caps: the kept buffers, each grown to
        min(cap, max(elements, 1 Mi)) when too small (0 elements ask for whatever is kept, None included). Any size
        beyond its cap: buffers of this call, and the kept ones stay as they are. The pinned buffers are handed out
        once the last copy out of them is done, so the caller may fill them at once."""
        if self._copied is not None:
            self._copied.synchronize()  # the pinned buffer is free again
        if any(n > cap for n, cap, _, _ in need.values()):
            return {k: _empty(max(n, 16), dtype, device) for k, (n, _, dtype, device) in need.items()}, False
        kept = self._kept
        small = [k for k, (n, _, _, _) in need.items() if n > (kept[k].numel() if k in kept else 0)]
        if small and self._done is not None:
            # the old buffers may still be read by the previous decode on another stream: let it finish before they
            # go back to the caching allocator
            self._done.synchronize()
        for k in small:
            n, cap, dtype, device = need[k]
            kept[k] = _grow(kept.get(k), n, dtype, device, cap)
        return {k: kept.get(k) for k in need}, True

    def _submit(self, kept, src, dst, n, nstatus, launch):
        """One run on torch's current stream: copy src[:n] (a pinned buffer of _take, filled by the caller) to
        dst[:n], zero `nstatus` status words, launch(status pointer, stream) (it raises where a launch is refused),
        read the status words back and wait: the list of status words. kept: the buffers are _take's kept ones, so
        the run is fenced behind the previous one and leaves its two events for the next. The run returns, or
        raises, only after everything it enqueued is done, so the buffers never change hands with work in flight."""
        cur = torch.cuda.current_stream(self.dev)
        if kept and self._done is not None:
            cur.wait_event(self._done)  # another stream's previous decode may still read the buffers
        copied, done = torch.cuda.Event(), torch.cuda.Event()
        status = self._status[:nstatus]
        try:
            dst[:n].copy_(src[:n], non_blocking=True)
            copied.record(cur)
            status.zero_()
            launch(status.data_ptr(), cur.cuda_stream)
            self._status_host[:nstatus].copy_(status, non_blocking=True)
        finally:
            done.record(cur)
            done.synchronize()
            if kept:
                self._copied, self._done = copied, done
        return self._status_host[:nstatus].tolist()

    def decode(self, data, out: torch.Tensor | None = None) -> torch.Tensor:
        """JPEG bytes → uint8 [H, W, 3] on the device (on torch's current stream). Returns once the kernels
        have run (the IDCT's envelope flag is read back: a file outside it raises UnsupportedJpeg, for Pillow)."""
        ptr, n, keep = _buf(data)
        L = lib()
        with self._lock:
            if self.entropy != "host":
                got = self._decode_gpu_entropy(L, ptr, n, out)
                if got is not None:
                    return got
            lay = _parse(L, ptr, n)
            ncoef = lay.total_blocks * 64
            b, kept = self._take({"coefs_host": (ncoef, KEEP_COEFS, torch.int16, None),
                                  "coefs_up": (ncoef, KEEP_COEFS, torch.int16, self.dev),
                                  "work_up": (lay.plane_bytes, KEEP_WORK, torch.uint8, self.dev)})
            host = b["coefs_host"]
            _check(L.sp_jpeg_decode_coefs(ptr, n, C.byref(lay), host.data_ptr(), host.numel()), "sp_jpeg_decode_coefs")
            del keep
            out, flag = self._to_rgb(L, lay, out, kept, host, b["coefs_up"], ncoef, b["coefs_up"], b["work_up"])
            if flag:
                raise UnsupportedJpeg(_OUTSIDE)
            return out

    def _decode_gpu_entropy(self, L, ptr, n, out):
        """entropy="gpu": pack on the host into the reused pinned buffer, copy the package asynchronously, run the
        entropy kernels and sp_jpeg_to_rgb, one status readback. The image, or None when the file takes the host path
        (not eligible, or a non-zero status word); raises UnsupportedJpeg as the host parser does. Lock held."""
        def pinned(nbytes):
            return self._take({"pkg_host": (nbytes, KEEP_PKG, torch.uint8, None)})[0]["pkg_host"]

        def alloc(lay, scan):
            _check_pixels(lay)
            return pinned(scan.pkg_bytes)

        # the first pass goes into whatever pinned buffer is kept: a file that fits costs one pass
        rc, lay, scan, host = _pack(L, ptr, n, pinned(0), alloc)
        if rc == SP_JPEG_NOT_ELIGIBLE:
            self.stats["host"] += 1
            return None
        _check(rc, "sp_jpeg_entropy_pack")
        _check_pixels(lay)
        ncoef = lay.total_blocks * 64
        # (a package beyond KEEP_PKG is in a pinned buffer of this call, and "pkg" is then beyond it too)
        b, kept = self._take({"pkg": (scan.pkg_bytes, KEEP_PKG, torch.uint8, self.dev),
                              "ent": (scan.work_bytes, KEEP_PKG, torch.uint8, self.dev),
                              "coefs": (ncoef, KEEP_COEFS, torch.int16, self.dev),
                              "work": (lay.plane_bytes, KEEP_WORK, torch.uint8, self.dev)})
        out, flag = self._to_rgb(L, lay, out, kept, host, b["pkg"], scan.pkg_bytes, b["coefs"], b["work"],
                                 entropy=(scan, b["ent"]))
        self.stats["h2d_bytes"] += int(scan.pkg_bytes)
        if flag:  # the GPU result is discarded; the host path accepts the file or raises UnsupportedJpeg by its own rules
            self.stats["fallback"][flag] = self.stats["fallback"].get(flag, 0) + 1
            return None
        self.stats["gpu"] += 1
        return out

    def _to_rgb(self, L, lay, out, kept, src, dst, n, coefs, work, entropy=None):
        """The back half of decode(): (image, status word). src[:n] goes up to dst[:n]: the coefficients themselves
        (dst is coefs), or, with entropy = (scan, workspace), the scan package, from which sp_jpeg_entropy_decode
        writes coefs on the device; then sp_jpeg_to_rgb into `out` (allocated here when None)."""
        H, W = lay.height, lay.width
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.dev)
        assert out.dtype == torch.uint8 and out.is_cuda and out.shape == (H, W, 3) and out.is_contiguous()

        def launch(status, stream):
            if entropy is not None:
                scan, ent = entropy
                _check(L.sp_jpeg_entropy_decode(dst.data_ptr(), C.byref(scan), C.byref(lay), ent.data_ptr(),
                                                ent.numel(), coefs.data_ptr(), coefs.numel(), status, stream),
                       "sp_jpeg_entropy_decode")
            _check(L.sp_jpeg_to_rgb(coefs.data_ptr(), C.byref(lay), work.data_ptr(), work.numel(), out.data_ptr(),
                                    W * 3, status, stream), "sp_jpeg_to_rgb")

        return out, self._submit(kept, src, dst, n, 1, launch)[0]

    def decode_many(self, datas, max_workers=None) -> list:
        """Many JPEGs → one entry per input, in input order: the uint8 [H, W, 3] device tensor decode() returns for
        that file (a view into one arena tensor per chunk, on torch's current stream), or the UnsupportedJpeg
        decode() raises for it, returned and not raised, so one bad file does not cost the batch. Any other error
        is raised as decode() raises it.

        Every file is parsed for its layout; the accepted ones are laid out by sp_jpeg_batch_plan in chunks of at
        most SP_JPEG_BATCH_MAX files whose totals fit the kept buffers (KEEP_COEFS / KEEP_WORK / KEEP_ARENA; a file
        larger than those runs as a chunk of its own through buffers of that call). Per chunk: the host entropy
        decode of its files in a thread pool (max_workers; default min(16, CPUs this process may use)), each into
        its slice of the pinned staging buffer, one H2D copy of coefficients plus table, one sp_jpeg_batch_to_rgb
        (two launches), one readback of the status words, one event wait.

        A decoder created with entropy="gpu" / "auto" first packs the accepted files' scans, SP_JPEG_BATCH_MAX files at
        a time (sp_jpeg_entropy_pack: no Huffman decode on the host; in the pool from PACK_POOL_BYTES of input on),
        and runs the eligible ones in GPU-entropy chunks as they fill (greedy, in input order, at most SP_JPEG_BATCH_MAX files within KEEP_PKG for the packages and for the entropy
        workspace, KEEP_COEFS, KEEP_WORK, KEEP_ARENA; a file beyond them alone): packages and both tables in one
        H2D copy, sp_jpeg_entropy_batch_decode (one memset, eight launches), sp_jpeg_batch_to_rgb on the same device
        coefficients, one status readback, one event wait. Files that are not eligible and files whose status word
        comes back non-zero (any bit, the envelope's included: decode()'s rule) then go through the host chunks
        above, so every file gives the host path's pixels or its UnsupportedJpeg.
        `batch_stats` counts the calls, chunks (= launch chains), images, h2d_bytes (what was uploaded), the files
        returned as UnsupportedJpeg by the parser ("refused") and by the IDCT envelope ("flagged"), and on a
        GPU-entropy decoder the files decoded by the GPU chain ("gpu"), the ones the packer found not eligible ("host";
        a file the packer refuses outright is not counted here: the host chunk counts it as "refused") and
        the ones re-routed to the host by their status word ("fallback": {status word: count}); `stats` is not
        touched."""
        L = lib()
        bufs = [_buf(d) for d in datas]
        out: list = [None] * len(bufs)
        lays: list = [None] * len(bufs)
        for i, (ptr, n, _) in enumerate(bufs):
            try:
                lays[i] = _parse(L, ptr, n)
            except UnsupportedJpeg as e:
                out[i] = e
        workers = max_workers if max_workers is not None else default_decode_workers()
        if workers < 1:
            raise ValueError("max_workers must be at least 1")
        refused = sum(o is not None for o in out)
        if self.entropy != "host":
            # the GPU-entropy chunks first; what they decoded leaves `lays`, the rest takes the host chunks below
            self._decode_many_gpu_entropy(L, bufs, lays, out, workers)
        live = [i for i, lay in enumerate(lays) if lay is not None]
        needs = [_chunk_need(lays[i]) for i in live]
        caps = (KEEP_COEFS - _TABLE_ELEMS, KEEP_WORK, KEEP_ARENA)  # the table travels behind the coefficients
        st = self.batch_stats
        with self._lock:
            st["calls"] += 1
            st["refused"] += refused
            pos = 0
            while pos < len(live):  # greedy chunks in input order
                n = _greedy(needs[pos:pos + SP_JPEG_BATCH_MAX], caps)
                self._decode_chunk(L, live[pos:pos + n], bufs, lays, out, workers)
                pos += n
        return out

    def _decode_chunk(self, L, idx, bufs, lays, out, workers):
        """One host-entropy chunk of decode_many (lock held): out[i] for i in idx."""
        n = len(idx)
        _, items, totals = _plan(L, [lays[i] for i in idx])
        tab_off = (totals.coef_elems + 7) & ~7  # the table follows the coefficients, 16-byte aligned
        nelem = tab_off + (C.sizeof(items) + 1) // 2
        b, kept = self._take({"coefs_host": (nelem, KEEP_COEFS, torch.int16, None),
                              "coefs_up": (nelem, KEEP_COEFS, torch.int16, self.dev),
                              "work_up": (totals.work_bytes, KEEP_WORK, torch.uint8, self.dev)})
        hp = b["coefs_host"].data_ptr()

        def entropy(k):
            ptr, nb, _ = bufs[idx[k]]
            lay = SpJpegLayout()  # sp_jpeg_decode_coefs rewrites the layout: a private copy per thread
            rc = L.sp_jpeg_decode_coefs(ptr, nb, C.byref(lay), hp + 2 * items[k].coef_off,
                                        lays[idx[k]].total_blocks * 64)
            if rc == 0:
                items[k].lay.quant = lay.quant  # the tables as latched at each component's first scan
            return rc, L.sp_last_error()  # (thread-local: read on the thread that made the call)

        if workers > 1 and n > 1:
            rcs = list(self._pool(workers).map(entropy, range(n)))
        else:
            rcs = [entropy(k) for k in range(n)]
        bad = {}
        for k, (rc, msg) in enumerate(rcs):
            if rc:
                # a refused file's slice holds whatever the decoder wrote before it stopped: the kernels run over it
                # (any int16 is a valid input) and the result is dropped
                bad[k] = _error(rc, "sp_jpeg_decode_coefs", msg)
                if not isinstance(bad[k], UnsupportedJpeg):
                    raise bad[k]
        C.memmove(hp + 2 * tab_off, items, C.sizeof(items))
        arena, flags = self._batch_to_rgb(L, items, totals, kept, b["coefs_host"], b["coefs_up"], nelem, 2 * tab_off,
                                          b["coefs_up"], b["work_up"])
        st = self.batch_stats
        st["chunks"] += 1
        st["images"] += n
        st["h2d_bytes"] += 2 * nelem
        for k, i in enumerate(idx):
            if k in bad:
                st["refused"] += 1
                out[i] = bad[k]
            elif flags[k]:
                st["flagged"] += 1
                out[i] = UnsupportedJpeg(_OUTSIDE)
            else:
                out[i] = _view(arena, items[k])

    def _batch_to_rgb(self, L, items, totals, kept, src, dst, n, tab_off, coefs, work, entropy=None):
        """The back half of a chunk: (RGB arena, status word per image). src[:n] goes up to dst[:n], the table at
        byte tab_off of it: the coefficients themselves (dst is coefs), or, with entropy = (entropy table, its
        totals, its byte offset in dst, workspace), the scan packages, from which sp_jpeg_entropy_batch_decode
        writes coefs on the device; then sp_jpeg_batch_to_rgb into a new arena."""
        cnt = len(items)
        arena = torch.empty(totals.rgb_bytes, dtype=torch.uint8, device=self.dev)

        def launch(status, stream):
            if entropy is not None:
                ent, etot, ent_off, ws = entropy
                _check(L.sp_jpeg_entropy_batch_decode(dst.data_ptr(), etot.pkg_bytes, dst.data_ptr() + ent_off, ent,
                                                      cnt, C.byref(etot), ws.data_ptr(), ws.numel(), coefs.data_ptr(),
                                                      totals.coef_elems, status, stream),
                       "sp_jpeg_entropy_batch_decode")
            _check(L.sp_jpeg_batch_to_rgb(coefs.data_ptr(), totals.coef_elems, dst.data_ptr() + tab_off, items, cnt,
                                          C.byref(totals), work.data_ptr(), work.numel(), arena.data_ptr(),
                                          arena.numel(), status, stream), "sp_jpeg_batch_to_rgb")

        return arena, self._submit(kept, src, dst, n, cnt, launch)

    def _decode_many_gpu_entropy(self, L, bufs, lays, out, workers):
        """decode_many on an entropy="gpu" decoder: pack the accepted files, a window of SP_JPEG_BATCH_MAX at a time,
        and run the eligible ones in GPU-entropy chunks as the windows fill them, so at most two windows' packages are
        alive at once. out[i] is set and lays[i] cleared for every file the GPU chain decoded with status 0. Takes the
        lock itself and holds it throughout: the pool and the counters are the decoder's."""
        live = [i for i, lay in enumerate(lays) if lay is not None]

        def pack(i):
            ptr, nb, _ = bufs[i]
            lay0 = lays[i]
            nmcu = (lay0.bw[0] // max(1, lay0.h[0])) * (lay0.bh[0] // max(1, lay0.v[0]))
            # no package of this file is larger (_PKG_FIXED): one pass; were it, the packer says so and gets its size
            first = np.empty(_PKG_FIXED + _SEG_BYTES * (nmcu + 2) + nb, dtype=np.uint8)
            rc, lay, scan, pkg = _pack(L, ptr, nb, first, lambda lay, scan: np.empty(scan.pkg_bytes, dtype=np.uint8))
            return rc, L.sp_last_error(), lay, scan, pkg  # (thread-local: read on the thread that made the call)

        st = self.batch_stats
        with self._lock:
            pending, pos = [], 0  # (index, layout, scan, package) of eligible files not yet run, in input order
            while pos < len(live) or pending:
                if pos < len(live):
                    window = live[pos:pos + SP_JPEG_BATCH_MAX]
                    pos += len(window)
                    if workers > 1 and len(window) > 1 and sum(bufs[i][1] for i in window) >= PACK_POOL_BYTES:
                        results = list(self._pool(workers).map(pack, window))
                    else:
                        results = [pack(i) for i in window]
                    for i, (rc, msg, lay, scan, pkg) in zip(window, results):
                        if rc == 0:
                            pending.append((i, lay, scan, pkg))
                        elif rc == SP_JPEG_NOT_ELIGIBLE:
                            st["host"] += 1  # the host chunk decodes it
                        elif rc != SP_JPEG_UNSUPPORTED:  # (the host chunk refuses that one by the host rules)
                            raise _error(rc, "sp_jpeg_entropy_pack", msg)
                # the greedy chunk at the head of `pending`: the packages plus both tables and the entropy workspaces
                # within KEEP_PKG each, then the host chunks' three budgets
                n = _greedy([(_a16(scan.pkg_bytes), _a16(scan.work_bytes)) + _chunk_need(lay)
                             for _, lay, scan, _ in pending[:SP_JPEG_BATCH_MAX]],
                            (KEEP_PKG - _ENT_TABLE_BYTES, KEEP_PKG, KEEP_COEFS, KEEP_WORK, KEEP_ARENA))
                if n == 0 or (n == len(pending) and n < SP_JPEG_BATCH_MAX and pos < len(live)):
                    continue  # the chunk is still open and there are files left to pack
                chunk, pending = pending[:n], pending[n:]
                self._gpu_entropy_chunk(L, chunk, lays, out)

    def _gpu_entropy_chunk(self, L, chunk, lays, out):
        """One GPU-entropy chunk (lock held): plan both tables, run the device half, route the results."""
        n = len(chunk)
        larr, items, totals = _plan(L, [c[1] for c in chunk])
        ent, etot = (SpJpegEntropyItem * n)(), SpJpegEntropyTotals()
        _check(L.sp_jpeg_entropy_batch_plan((SpJpegScan * n)(*[c[2] for c in chunk]), larr, items, n, ent,
                                            C.byref(etot)), "sp_jpeg_entropy_batch_plan")
        arena, flags, h2d = self._run_gpu_entropy_chunk(L, [c[3] for c in chunk], ent, etot, items, totals)
        st = self.batch_stats
        st["chunks"] += 1
        st["h2d_bytes"] += h2d
        for k, (i, _, _, _) in enumerate(chunk):
            if flags[k]:  # the GPU result is discarded: the host chunk accepts the file or refuses it
                st["fallback"][flags[k]] = st["fallback"].get(flags[k], 0) + 1
                continue
            out[i] = _view(arena, items[k])
            lays[i] = None
            st["gpu"] += 1
            st["images"] += 1

    def _run_gpu_entropy_chunk(self, L, pkgs, ent, etot, items, totals):
        """The device half of one GPU-entropy chunk (lock held): (RGB arena, status word per image, bytes uploaded).
        Packages and both tables go into the pinned package buffer and up in one copy. (The host tests replace this
        method with the CPU emulation of the launch chain: nothing above it touches the device.)"""
        ent_off = _a16(etot.pkg_bytes)
        tab_off = _a16(ent_off + C.sizeof(ent))
        nbytes = tab_off + C.sizeof(items)
        b, kept = self._take({"pkg_host": (nbytes, KEEP_PKG, torch.uint8, None),
                              "pkg": (nbytes, KEEP_PKG, torch.uint8, self.dev),
                              "ent": (etot.work_bytes, KEEP_PKG, torch.uint8, self.dev),
                              "coefs": (totals.coef_elems, KEEP_COEFS, torch.int16, self.dev),
                              "work": (totals.work_bytes, KEEP_WORK, torch.uint8, self.dev)})
        hp = b["pkg_host"].data_ptr()
        for k, pkg in enumerate(pkgs):
            C.memmove(hp + ent[k].pkg_off, pkg.ctypes.data, ent[k].scan.pkg_bytes)
        C.memmove(hp + ent_off, ent, C.sizeof(ent))
        C.memmove(hp + tab_off, items, C.sizeof(items))
        arena, flags = self._batch_to_rgb(L, items, totals, kept, b["pkg_host"], b["pkg"], nbytes, tab_off, b["coefs"],
                                          b["work"], entropy=(ent, etot, ent_off, b["ent"]))
        return arena, flags, nbytes

    def _pool(self, workers):
        """The decoder's entropy-decode thread pool (created on first use, replaced when the size changes)."""
        import concurrent.futures as cf

        if self._workers is None or self._workers[0] != workers:
            if self._workers is not None:
                self._workers[1].shutdown(wait=True)
            self._workers = (workers, cf.ThreadPoolExecutor(max_workers=workers, thread_name_prefix="spotter-jpeg"))
        return self._workers[1]




_decoders: dict = {}
_dec_lock = threading.Lock()


class _ArrowArray(C.Structure):
    pass


_ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64),
                        ("n_buffers", C.c_int64), ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)),
                        ("children", C.POINTER(C.POINTER(_ArrowArray))), ("dictionary", C.c_void_p),
                        ("release", C.c_void_p), ("private_data", C.c_void_p)]
_capsule_ptr = C.pythonapi.PyCapsule_GetPointer
_capsule_ptr.restype = C.c_void_p
_capsule_ptr.argtypes = [C.py_object, C.c_char_p]


def pil_pixels(im):
    """(host pointer, row stride, bytes per pixel, keep-alive) of a PIL RGB image's pixels: zero-copy through
    Pillow's Arrow C-data export (RGB is stored as 4-byte RGBX pixels) when the image is one memory block, else
    a packed RGB copy (tobytes)."""
    im.load()
    W, H = im.size
    try:
        caps = im.__arrow_c_array__()
        arr = _ArrowArray.from_address(_capsule_ptr(caps[1], b"arrow_array"))
        child = arr.children[0].contents
        if arr.n_children == 1 and child.length == W * H * 4 and child.offset == 0 and arr.offset == 0:
            return child.buffers[1], W * 4, 4, caps
    except (AttributeError, ValueError, TypeError):
        pass
    b = im.tobytes()
    return C.cast(C.c_char_p(b), C.c_void_p).value, W * 3, 3, b


class JpegEncoder:
    """Per-device JPEG encoder (serve.py:139-142 `image.save(buffer, format="JPEG")`): the layout per image
    size / quality / subsampling, device workspace and bit buffer, pinned staging for the pixel upload and the
    bit download, all grown as needed and reused (one encode at a time; the lock serialises callers)."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self._lock = threading.Lock()
        self._plans: dict = {}
        self._work = self._bits = self._pix = None
        self._stage = self._down = None
        self._nbits = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._nbits_host = torch.zeros(1, dtype=torch.int64, pin_memory=True)
        # encode_many: bit counts, segment offsets and bytes used of a chunk; the finish pool; the counters
        self._res = torch.zeros(2 * SP_JPEG_BATCH_MAX + 1, dtype=torch.int64, device=self.dev)
        self._res_host = torch.zeros(2 * SP_JPEG_BATCH_MAX + 1, dtype=torch.int64, pin_memory=True)
        self._workers = None
        self.stats = _new_enc_stats()

    def plan(self, W, H, quality=-1, subsampling=-1) -> SpJpegEncLayout:
        key = (W, H, quality, subsampling)
        lay = self._plans.get(key)
        if lay is None:
            lay = SpJpegEncLayout()
            if lib().sp_jpeg_enc_plan(W, H, quality, subsampling, C.byref(lay)):
                raise ValueError(lib().sp_last_error().decode(errors="replace"))
            if len(self._plans) > 64:
                self._plans.clear()
            self._plans[key] = lay
        return lay

    def encode(self, src, quality=-1, subsampling=-1, comment: bytes | None = None) -> bytes:
        """src: a uint8 [H, W, 3] device tensor, or a PIL RGB image (its host pixels are uploaded)."""
        with self._lock:
            L = lib()
            cur = torch.cuda.current_stream(self.dev)
            if isinstance(src, torch.Tensor):
                assert src.dtype == torch.uint8 and src.is_cuda and src.dim() == 3 and src.shape[2] in (3, 4)
                assert src.stride(2) == 1 and src.stride(1) == src.shape[2]
                H, W, pb = src.shape
                ptr, stride, keep = src.data_ptr(), src.stride(0), src
            else:
                W, H = src.size
                hptr, stride, pb, keep_h = pil_pixels(src)
                n = stride * H
                self._stage = _grow(self._stage, n, torch.uint8)
                self._pix = _grow(self._pix, n, torch.uint8, self.dev)
                C.memmove(self._stage.data_ptr(), hptr, n)
                del keep_h
                self._pix[:n].copy_(self._stage[:n], non_blocking=True)
                ptr, keep = self._pix.data_ptr(), None
            lay = self.plan(W, H, quality, subsampling)
            self._work = _grow(self._work, lay.work_bytes, torch.uint8, self.dev)
            self._bits = _grow(self._bits, lay.bits_cap, torch.uint8, self.dev)
            rc = L.sp_jpeg_enc_rgb(ptr, stride, pb, C.byref(lay), self._work.data_ptr(), self._work.numel(),
                                   self._bits.data_ptr(), self._bits.numel(), self._nbits.data_ptr(), cur.cuda_stream)
            if rc:
                raise RuntimeError(f"sp_jpeg_enc_rgb: {L.sp_last_error().decode(errors='replace')}")
            self._nbits_host.copy_(self._nbits, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            ev.synchronize()
            nbits = int(self._nbits_host[0])
            nbytes = (nbits + 7) // 8
            self._down = _grow(self._down, nbytes, torch.uint8)
            self._down[:nbytes].copy_(self._bits[:nbytes], non_blocking=True)
            ev.record(cur)
            ev.synchronize()
            del keep
            com = comment or b""
            cap = L.sp_jpeg_enc_max_bytes(C.byref(lay), nbits, len(com))
            out = C.create_string_buffer(cap)
            n = C.c_int64()
            rc = L.sp_jpeg_enc_finish(C.byref(lay), self._down.data_ptr(), nbits, com, len(com), out, cap,
                                      C.byref(n))
            if rc:
                raise RuntimeError(f"sp_jpeg_enc_finish: {L.sp_last_error().decode(errors='replace')}")
            return out.raw[:n.value]

    _pool = JpegDecoder._pool  # the same thread-pool helper, over this object's _workers

    def _source(self, src, quality, subsampling):
        """One encode_many source as the chunk code needs it: the layout, the device pointer (a tensor) or the host
        pixels still to be staged (a PIL image), and what the chunk rule counts for it."""
        s = types.SimpleNamespace(src=src, ptr=None, host=None, nbytes=0, keep=None)
        if isinstance(src, DeviceRGBImage) and src._im is None:
            s.src = src = src.spotter_device_rgb  # pending draws are flushed on the current stream
        if isinstance(src, torch.Tensor):
            assert src.dtype == torch.uint8 and src.is_cuda and src.dim() == 3 and src.shape[2] in (3, 4)
            assert src.stride(2) == 1 and src.stride(1) == src.shape[2]
            H, W, s.pb = src.shape
            s.ptr, s.stride, s.keep = src.data_ptr(), src.stride(0), src
        else:
            W, H = src.size
            s.host, s.stride, s.pb, s.keep = pil_pixels(src)
            s.nbytes = s.stride * H
        s.lay = self.plan(W, H, quality, subsampling)
        s.need = ((s.lay.work_bytes + 255) & ~255, _a16(s.lay.bits_cap), (s.nbytes + 255) & ~255)
        return s

    def encode_many(self, srcs, quality=-1, subsampling=-1, comments=None, max_workers=None) -> list:
        """encode() over a list of sources at one quality / subsampling: one file per source, byte for byte what
        encode(src, quality, subsampling, comment) returns. srcs: uint8 [H, W, 3 | 4] device tensors (encode()'s stride
        rules), DeviceRGBImages (their pending draws are applied first, all of them together: flush_many) and PIL RGB
        images, mixed freely; comments: None, or one bytes / None per source.

        Per chunk (up to SP_JPEG_BATCH_MAX images, closed earlier where its workspace, packed bit capacity or staged
        host pixels would pass KEEP_ENC_WORK / KEEP_ENC_BITS / KEEP_ENC_PIX; a single image beyond one of them goes
        through encode()): the host pixels of its PIL sources and the table staged into one pinned buffer and uploaded
        with one copy, sp_jpeg_enc_batch_rgb's six launches on the current stream, one readback of the bit counts and
        segment offsets, one download of exactly the bytes in use, then sp_jpeg_enc_finish per image (in a thread pool
        of max_workers, default min(16, CPUs), from FINISH_POOL_BYTES of segment data on: ctypes releases the GIL).
        Two stream waits per chunk where encode() makes two per image. `stats` counts what was done."""
        srcs = list(srcs)
        coms = [b""] * len(srcs) if comments is None else [c or b"" for c in comments]
        if len(coms) != len(srcs):
            raise ValueError("comments must be None or hold one entry per source")
        workers = max_workers if max_workers is not None else default_decode_workers()
        if workers < 1:
            raise ValueError("max_workers must be at least 1")
        self.stats["calls"] += 1
        # the pending draws of the whole call in one launch per SP_DRAW_BATCH_MAX images, not one per image in _source
        flush_many([s for s in srcs if isinstance(s, DeviceRGBImage) and s._im is None])
        descs = [self._source(s, quality, subsampling) for s in srcs]
        caps = (KEEP_ENC_WORK, KEEP_ENC_BITS, KEEP_ENC_PIX)
        out = []
        i = 0
        while i < len(descs):
            if any(x > cap for x, cap in zip(descs[i].need, caps)):
                out.append(self.encode(descs[i].src, quality, subsampling, coms[i] or None))
                self.stats["single"] += 1
                i += 1
                continue
            n = _greedy([d.need for d in descs[i:i + SP_JPEG_BATCH_MAX]], caps)
            with self._lock:
                out += self._encode_chunk(lib(), descs[i:i + n], coms[i:i + n], workers)
            i += n
        return out

    def _encode_chunk(self, L, descs, coms, workers):
        n = len(descs)
        cur = torch.cuda.current_stream(self.dev)
        lays = (SpJpegEncLayout * n)(*[d.lay for d in descs])
        items, totals = (SpJpegEncBatchItem * n)(), SpJpegEncBatchTotals()
        _check(L.sp_jpeg_enc_batch_plan(lays, n, items, C.byref(totals)), "sp_jpeg_enc_batch_plan")
        # the upload: [host pixels of the PIL sources, each at a multiple of 256][the table]
        pix_off, tab_off = [], 0
        for d in descs:
            pix_off.append(tab_off)
            tab_off += d.need[2]
        nup = tab_off + C.sizeof(items)
        self._stage = _grow(self._stage, nup, torch.uint8)
        self._pix = _grow(self._pix, nup, torch.uint8, self.dev)
        self._work = _grow(self._work, totals.work_bytes, torch.uint8, self.dev)
        self._bits = _grow(self._bits, totals.bits_cap, torch.uint8, self.dev)
        hp, dp = self._stage.data_ptr(), self._pix.data_ptr()
        for it, d, off in zip(items, descs, pix_off):
            if d.host is not None:
                C.memmove(hp + off, d.host, d.nbytes)
                d.keep = None
            it.src = d.ptr if d.host is None else dp + off
            it.row_stride, it.pixel_bytes = d.stride, d.pb
        C.memmove(hp + tab_off, items, C.sizeof(items))
        self._pix[:nup].copy_(self._stage[:nup], non_blocking=True)
        _check(L.sp_jpeg_enc_batch_rgb(dp + tab_off, items, n, C.byref(totals), self._work.data_ptr(),
                                       self._work.numel(), self._bits.data_ptr(), self._bits.numel(),
                                       self._res.data_ptr(), cur.cuda_stream), "sp_jpeg_enc_batch_rgb")
        m = 2 * n + 1
        self._res_host[:m].copy_(self._res[:m], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cur)
        ev.synchronize()
        res = self._res_host[:m].tolist()
        nbits, seg, used = res[:n], res[n:2 * n], res[2 * n]
        self._down = _grow(self._down, used, torch.uint8)
        self._down[:used].copy_(self._bits[:used], non_blocking=True)
        ev.record(cur)
        ev.synchronize()
        for d in descs:
            d.keep = None
        base = self._down.data_ptr()

        def finish(k):
            lay, com = descs[k].lay, coms[k]
            cap = L.sp_jpeg_enc_max_bytes(C.byref(lay), nbits[k], len(com))
            buf, cnt = C.create_string_buffer(cap), C.c_int64()
            rc = L.sp_jpeg_enc_finish(C.byref(lay), base + seg[k], nbits[k], com, len(com), buf, cap, C.byref(cnt))
            # the error text is thread-local: read where the call was made
            return (rc, L.sp_last_error()) if rc else (0, C.string_at(buf, cnt.value))

        if workers > 1 and n > 1 and used >= FINISH_POOL_BYTES:
            done = list(self._pool(workers).map(finish, range(n)))
        else:
            done = [finish(k) for k in range(n)]
        for rc, val in done:
            if rc:
                raise _error(rc, "sp_jpeg_enc_finish", val)
        st = self.stats
        st["chunks"] += 1
        st["images"] += n
        st["h2d_bytes"] += nup
        st["d2h_bytes"] += 8 * m + used
        st["waits"] += 2
        return [val for _, val in done]


_encoders: dict = {}


def encoder(device=None) -> JpegEncoder:
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with _dec_lock:
        e = _encoders.get(dev)
        if e is None:
            e = _encoders[dev] = JpegEncoder(dev)
        return e


_env_entropy = None  # SPOTTER_JPEG_ENTROPY as open_image first found it (read and validated once per process)


def default_entropy() -> str:
    """The entropy mode of the decoders open_image creates: SPOTTER_JPEG_ENTROPY, read once."""
    global _env_entropy
    if _env_entropy is None:
        _env_entropy = jpeg_entropy_from_env()
    return _env_entropy


def decoder(device=None, entropy="host") -> JpegDecoder:
    """The shared decoder of a device and entropy mode (the environment is not read here)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    mode = check_jpeg_entropy(entropy)
    key = dev if mode == "host" else (dev, mode)
    with _dec_lock:
        d = _decoders.get(key)
        if d is None:
            d = _decoders[key] = JpegDecoder(dev, mode)
        return d


from PIL import Image as _PILImage  # noqa: E402  (Pillow is a dependency of the reference app)
from PIL import JpegImagePlugin as _JpegPlugin  # noqa: E402

from .draw import DrawList  # noqa: E402


class DeviceRGBImage(_PILImage.Image):
    """A PIL RGB image whose pixels live on the GPU: the uint8 [H, W, 3] device tensor `spotter_device_rgb`, which
    SpotterImageProcessor reads in place, the drop-in's ImageDraw draws on (spotter_amd/draw.py DeviceDraw records
    into `_draw_list`; flush() applies the list with one sp_draw_rgb launch before anything reads the pixels) and
    save(format="JPEG") encodes from. The host pixels are made only when Pillow itself needs them (load(): a
    device → host copy on demand; from then on the image is an ordinary loaded PIL image, drawn on by Pillow and
    uploaded by save). convert("RGB") / copy() of a not-yet-loaded image stay lazy and share the tensor until one
    of them is drawn on. `info` is the source file's, as Pillow's JpegImageFile would carry it (its "comment" is
    written back by save)."""

    def __init__(self, rgb_dev: torch.Tensor, info=None, shared=False):
        super().__init__()
        H, W, _ = rgb_dev.shape
        self._mode = "RGB"
        self._size = (int(W), int(H))
        self._dev = rgb_dev
        self._owns = not shared  # a shared tensor is cloned before the first draw reaches it
        self._draw_list = DrawList(W, H)
        if info:
            self.info = dict(info)

    @property
    def spotter_device_rgb(self) -> torch.Tensor:
        """The device pixels with every recorded draw applied."""
        self.flush()
        return self._dev

    def flush(self):
        """Apply the recorded draw operations on the current stream: one packed table (operations, tile bins, mask
        bytes) in the device's pinned staging buffer, one H2D copy, one sp_draw_rgb launch."""
        lst = self._draw_list
        if not len(lst):
            return
        t = self._drawable()
        _draw_stage(t.device).run(lst, t)
        lst.clear()

    def _drawable(self) -> torch.Tensor:
        """The tensor a draw may write in place: the image's own packed-RGB tensor, or a clone of a shared or
        differently laid out one, which the image owns from here on."""
        t = self._dev
        if not self._owns or t.stride(2) != 1 or t.stride(1) != 3 or t.stride(0) < 3 * t.shape[1]:
            t = self._dev = t.clone(memory_format=torch.contiguous_format)  # device to device
            self._owns = True
        return t

    def _lazy_copy(self):
        t = self.spotter_device_rgb  # pending draws are applied first (by the owner in place, else to a clone)
        self._owns = False  # from here on neither image owns the tensor
        return DeviceRGBImage(t, info=self.info, shared=True)

    def load(self):
        if self._im is None and getattr(self, "_dev", None) is not None:
            # the host copy as RGBX rows (X = 255): Pillow's own 4-byte pixel layout, which frombytes unpacks with
            # a straight 4-byte copy (0.48 against 0.98 ms for packed RGB through a bytes object)
            t = self.spotter_device_rgb
            H, W, _ = t.shape
            x4 = torch.full((H, W, 4), 255, dtype=torch.uint8, device=t.device)
            x4[..., :3].copy_(t)
            host = torch.empty((H, W, 4), dtype=torch.uint8, pin_memory=True)
            host.copy_(x4, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(t.device))
            done.synchronize()
            self.im = _PILImage.frombytes("RGB", self._size, memoryview(host.numpy()).cast("B"), "raw", "RGBX").im
        return super().load()

    def convert(self, mode=None, *args, **kwargs):
        if mode in (None, "RGB") and not args and not kwargs and self._im is None:
            return self._lazy_copy()
        return super().convert(mode, *args, **kwargs)

    def copy(self):
        if self._im is None:
            return self._lazy_copy()
        return super().copy()

    def save(self, fp, format=None, **params):
        """serve.py:140 `image.save(buffer, format="JPEG")`: encoded on the GPU, the bytes Pillow writes. An image
        whose pixels never reached the host (drawn on through the drop-in's ImageDraw or not at all) encodes from
        its device tensor, recorded draws applied first; once loaded (drawn on by Pillow), its host pixels are
        uploaded. Other formats, file names and options go to Pillow's own save."""
        opts = _gpu_jpeg_options(self, fp, format, params)
        if opts is None:
            return super().save(fp, format, **params)
        src = self.spotter_device_rgb if self._im is None else self
        fp.write(encoder(self._dev.device).encode(src, *opts))


class _DrawStage:
    """Per-device staging of DeviceRGBImage.flush: a pinned host buffer the draw table is packed into and its
    device copy, grown as needed and reused like JpegEncoder's (one flush at a time; the lock serialises callers)."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self._lock = threading.Lock()
        self._stage = self._table = None
        self._copied = None  # event: the last H2D copy out of the pinned buffer is done
        self._done = None    # event: the last launch is done with the device table
        # run_many's counters: launches, images in them, bytes uploaded, host waits for an event that had not passed
        self.stats = {"batch_launches": 0, "batch_images": 0, "batch_h2d_bytes": 0, "batch_waits": 0}

    def _wait(self, event):
        if event is not None and not event.query():
            self.stats["batch_waits"] += 1
            event.synchronize()

    def _alloc(self, n):
        """New staging of at least n bytes: (pinned host buffer, device buffer)."""
        return _grow(None, n, torch.uint8), _grow(None, n, torch.uint8, self.dev)

    def pack_batch(self, pairs):
        """The batch buffer of run_many in the pinned staging buffer (lock held, the buffer free):
        [each list's packed table, as sp_draw_pack writes it, back to back at multiples of 16][the sp_draw_batch_item
        rows, planned]. Returns (rows, the buffer as a uint8 array over the staging buffer, the rows' offset)."""
        L = lib()
        items = (SpDrawBatchItem * len(pairs))()
        rows = C.sizeof(items)

        def pack_all():
            cap = 0 if self._stage is None else self._stage.numel()
            base = self._stage.data_ptr() if cap else 0
            off, fits = 0, True
            for it, (lst, _) in zip(items, pairs):
                room = cap - rows - off
                need = lst.pack(base + off, room) if fits and room > 0 else lst.pack()
                fits = fits and need <= room
                it.table_off, it.table_bytes = off, need  # (a table's size is a multiple of 16)
                off += need
            return off, fits

        end, fits = pack_all()
        if not fits:
            self._wait(self._done)  # the old device table goes back to the caching allocator
            self._stage, self._table = self._alloc(end + rows)
            end, fits = pack_all()
            assert fits
        for it, (_, t) in zip(items, pairs):
            it.rgb, it.height, it.width, it.row_stride = t.data_ptr(), t.shape[0], t.shape[1], t.stride(0)
        hp = self._stage.data_ptr()
        if L.sp_draw_batch_plan(items, len(pairs), hp, end) < 0:
            raise RuntimeError(f"sp_draw_batch_plan: {L.sp_last_error().decode(errors='replace')}")
        C.memmove(hp + end, items, rows)
        return items, self._stage[:end + rows].numpy(), end

    def run_many(self, pairs):
        """The draw lists of up to SP_DRAW_BATCH_MAX images, pairs of (non-empty DrawList, its drawable tensor), in one
        launch on the current stream: pack_batch's buffer, one H2D copy, one sp_draw_batch_rgb. The staging buffers
        and their two events are run()'s, so single and batched flushes on any streams keep one order."""
        with self._lock:
            L = lib()
            cur = torch.cuda.current_stream(self.dev)
            self._wait(self._copied)  # the pinned buffer is free again
            items, buf, end = self.pack_batch(pairs)
            n, nbytes = len(pairs), len(buf)
            hp, dp = self._stage.data_ptr(), self._table.data_ptr()
            if self._done is not None:
                cur.wait_event(self._done)  # another stream's previous launch may still read the device table
            self._table[:nbytes].copy_(self._stage[:nbytes], non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record(cur)
            rc = L.sp_draw_batch_rgb(dp + end, items, n, hp, dp, end, cur.cuda_stream)
            if rc:
                raise RuntimeError(f"sp_draw_batch_rgb: {L.sp_last_error().decode(errors='replace')}")
            self._done = torch.cuda.Event()
            self._done.record(cur)
            st = self.stats
            st["batch_launches"] += 1
            st["batch_images"] += n
            st["batch_h2d_bytes"] += nbytes

    def run(self, lst, rgb: torch.Tensor):
        with self._lock:
            L = lib()
            cur = torch.cuda.current_stream(self.dev)
            if self._copied is not None:
                self._copied.synchronize()  # the pinned buffer is free again
            cap = 0 if self._stage is None else self._stage.numel()
            need = lst.pack(self._stage.data_ptr() if cap else None, cap)
            if need > cap:
                if self._done is not None:
                    self._done.synchronize()  # the old device table goes back to the caching allocator
                self._stage = _grow(None, need, torch.uint8)
                self._table = _grow(None, need, torch.uint8, self.dev)
                need = lst.pack(self._stage.data_ptr(), self._stage.numel())
            if self._done is not None:
                cur.wait_event(self._done)  # another stream's previous launch may still read the device table
            self._table[:need].copy_(self._stage[:need], non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record(cur)
            H, W, _ = rgb.shape
            rc = L.sp_draw_rgb(rgb.data_ptr(), H, W, rgb.stride(0), self._stage.data_ptr(), self._table.data_ptr(),
                               need, cur.cuda_stream)
            if rc:
                raise RuntimeError(f"sp_draw_rgb: {L.sp_last_error().decode(errors='replace')}")
            self._done = torch.cuda.Event()
            self._done.record(cur)


_stages: dict = {}


def _draw_stage(device) -> _DrawStage:
    dev = torch.device(device)
    with _dec_lock:
        s = _stages.get(dev)
        if s is None:
            s = _stages[dev] = _DrawStage(dev)
        return s


def flush_many(images) -> None:
    """DeviceRGBImage.flush over any number of images of one device, on the current stream: the pending draw lists of
    up to SP_DRAW_BATCH_MAX images go up in one copy and are applied by one sp_draw_batch_rgb launch (a group per
    SP_DRAW_BATCH_MAX images with draws; a single image takes the same path). Images with nothing recorded are left
    out and not touched; an image listed twice is flushed once. Per image the ownership rule is flush()'s (a shared
    or not packed-RGB tensor is cloned first), and the pixels are flush()'s, bit for bit."""
    todo, seen = [], set()
    for im in images:
        if len(im._draw_list) and id(im) not in seen:
            seen.add(id(im))
            todo.append(im)
    if not todo:
        return
    dev = todo[0]._dev.device
    if any(im._dev.device != dev for im in todo):
        raise ValueError("flush_many: the images are on more than one device")
    stage = _draw_stage(dev)
    for i in range(0, len(todo), SP_DRAW_BATCH_MAX):
        group = todo[i:i + SP_DRAW_BATCH_MAX]
        stage.run_many([(im._draw_list, im._drawable()) for im in group])
        for im in group:
            im._draw_list.clear()


_SUBSAMPLING = {-1: -1, 0: 0, 1: 1, 2: 2, "4:4:4": 0, "4:2:2": 1, "4:2:0": 2, "4:1:1": 2}


def _gpu_jpeg_options(im, fp, format, params):
    """(quality, subsampling, comment) when Pillow's JPEG save of `im` with these arguments is what the GPU
    encoder writes (JpegImagePlugin._save: baseline, standard tables, no dpi / EXIF / ICC / XMP / extra,
    comment from im.info), else None."""
    if format is None or str(format).upper() not in ("JPEG", "JPG") or not hasattr(fp, "write"):
        return None
    if im.mode != "RGB" or set(params) - {"quality", "subsampling"}:
        return None
    if max(im.size) > JPEG_MAX_DIMENSION:  # libjpeg raises JERR_IMAGE_TOO_BIG: Pillow's save raises it
        return None
    q = params.get("quality", -1)
    sub = params.get("subsampling", -1)
    if type(q) is not int or not (q == -1 or 1 <= q <= 100):
        return None
    if not isinstance(sub, (int, str)) or sub not in _SUBSAMPLING:
        return None
    comment = im.info.get("comment")
    if comment is not None and (not isinstance(comment, bytes) or len(comment) > 65533):
        return None
    # (dpi, EXIF, ICC and XMP come from the save() arguments only, never from im.info: any of them → Pillow)
    return q, _SUBSAMPLING[sub], comment


def _device_image(im, data, device=None, entropy="host"):
    """A file Pillow has opened (its header parse, identification rules and decompression-bomb check have run,
    raising whatever the reference raises) → its GPU-decoded DeviceRGBImage, or None to keep Pillow's image:
    other formats and modes, MPO, and every JPEG the library leaves to the host decoder."""
    if type(im) is not _JpegPlugin.JpegImageFile or im.mode != "RGB":
        return None
    try:
        dec = decoder(device) if entropy == "host" else decoder(device, entropy)
        return DeviceRGBImage(dec.decode(data), info=im.info)
    except UnsupportedJpeg:
        return None


def open_image(data, device=None, entropy=None):
    """serve.py:96's `Image.open(BytesIO(image_bytes))` for raw bytes: a DeviceRGBImage for the JPEGs the
    library decodes (pixels identical to Pillow's), Pillow's own image otherwise. Pillow parses the header
    first, so a file Pillow refuses raises exactly what the reference raises. entropy: "host" / "gpu" / "auto",
    None: SPOTTER_JPEG_ENTROPY as first read (default_entropy)."""
    import io

    b = bytes(data)
    im = _PILImage.open(io.BytesIO(b))
    dev = _device_image(im, b, device, default_entropy() if entropy is None else entropy)
    if dev is None:
        return im
    im.close()
    return dev


class _ImageModule(types.ModuleType):
    """`PIL.Image` as serve.py sees it after the drop-in: every attribute is Pillow's,
    except `open`, which decodes JPEGs on the GPU (open_image's rule) when handed an in-memory file, as
    serve.py:96 does. Bound at module scope, so AmenitiesDetector's body stays the reference's, byte for byte."""

    def __init__(self, device=None):
        super().__init__("PIL.Image", _PILImage.__doc__)
        self._spotter_device = device
        # latched here, once: a bad SPOTTER_JPEG_ENTROPY fails the drop-in's import, later changes are not seen
        self._spotter_entropy = jpeg_entropy_from_env()

    def __getattr__(self, name):
        return getattr(_PILImage, name)

    def open(self, fp, mode="r", formats=None):
        import io

        im = _PILImage.open(fp, mode, formats)
        if mode == "r" and isinstance(fp, io.BytesIO):
            dev = _device_image(im, fp.getvalue(), self._spotter_device, self._spotter_entropy)
            if dev is not None:
                im.close()
                return dev
        return im


def image_module(device=None) -> types.ModuleType:
    """The `Image` global the drop-in binds in serve.py (spotter_amd/dropin.py)."""
    return _ImageModule(device)
