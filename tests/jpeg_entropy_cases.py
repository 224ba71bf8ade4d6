"""Inputs of the GPU entropy decode tests (tests/test_jpeg_entropy_host.py on the CPU emulation,
tests/test_gpu_jpeg_entropy.py on the kernels): baseline JPEGs built with Pillow, in the style of
tests/test_gpu_jpeg.py::_cases.

cases(): the non-degenerate inputs — every size at which the decode takes another path (a stream shorter than
one subsequence; one workgroup; several workgroups, so the cross-workgroup rounds run), each subsampling, gray,
restart segments of one MCU row and of one MCU, quality-100 noise (16-bit codes followed by long magnitudes
that straddle subsequence ends), and a baseline re-encode of the reference fixture. resistant(): frames whose
streams are periodic, so a wrongly started decoder can stay out of step for ever; the tests assert nothing
about which path those take.
"""
from __future__ import annotations

import functools
import io
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "test_pic.jpg")
SIZES = [(1, 1), (2, 3), (17, 33), (233, 177), (480, 640)]


def jpeg(img, mode="RGB", **kw) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(img).convert(mode).save(b, "JPEG", **kw)
    return b.getvalue()


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    from PIL import Image

    from spotter_amd.synthetic import synthetic_image

    out = []
    for (h, w) in SIZES:
        img = synthetic_image(h * 7 + w, h, w) if min(h, w) >= 2 else np.full((h, w, 3), 77, np.uint8)
        for sub in (0, 1, 2):
            out.append((f"{h}x{w} sub{sub}", jpeg(img, quality=90, subsampling=sub)))
    out.append(("gray", jpeg(synthetic_image(3, 45, 61), mode="L", quality=85)))
    out.append(("gray 233x177", jpeg(synthetic_image(4, 233, 177), mode="L", quality=90)))
    out.append(("restart rows", jpeg(synthetic_image(5, 123, 77), quality=80, restart_marker_rows=1, subsampling=2)))
    out.append(("restart 1 mcu", jpeg(synthetic_image(6, 67, 90), quality=85, restart_marker_blocks=1, subsampling=1)))
    out.append(("restart 1 mcu gray", jpeg(synthetic_image(7, 40, 50), mode="L", quality=85, restart_marker_blocks=1)))
    noise = np.random.default_rng(0).integers(0, 256, (96, 80, 3), dtype=np.uint8)
    out.append(("noise q100", jpeg(noise, quality=100, subsampling=0)))
    out.append(("noise q100 420", jpeg(noise, quality=100, subsampling=2)))
    short = jpeg(np.full((8, 8, 3), 130, np.uint8), quality=50, subsampling=0)
    out.append(("shorter than a subsequence", short))
    pic = np.asarray(Image.open(GOLDEN).convert("RGB"))
    out.append(("test_pic baseline", jpeg(pic, quality=75, subsampling=2)))
    out.append(("test_pic baseline 444", jpeg(pic, quality=75, subsampling=0)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def resistant() -> tuple:
    out = []
    for v in (0, 128, 255):
        out.append((f"flat {v}", jpeg(np.full((96, 160, 3), v, np.uint8), quality=75)))
    x = np.arange(256)
    stripes = np.where((x // 4) % 2 == 0, 40, 210).astype(np.uint8)  # period 8 pixels: every block the same
    out.append(("stripes", jpeg(np.broadcast_to(stripes[None, :, None], (128, 256, 3)).copy(), quality=90)))
    out.append(("stripes 444", jpeg(np.broadcast_to(stripes[None, :, None], (128, 256, 3)).copy(), quality=90,
                                    subsampling=0)))
    out.append(("black 640x480", jpeg(np.zeros((480, 640, 3), np.uint8), quality=75)))
    return tuple(out)


def _segment(data: bytes, marker: int) -> tuple:
    """(offset of the 0xFF, total length) of the first `marker` segment of the header."""
    p = 2
    while data[p + 1] != marker:
        p += 2 + int.from_bytes(data[p + 2:p + 4], "big")
    return p, 2 + int.from_bytes(data[p + 2:p + 4], "big")


def multi_scan_baseline(h=37, w=52, quality=85) -> bytes:
    """A sequential (SOF0) file with three non-interleaved scans, put together by hand: the three planes of an image
    are encoded by Pillow as gray files (same size, quality and standard tables, so a gray file's scan is exactly a
    non-interleaved scan of a 1x1-sampled component), and the file is the first one's header with a 3-component
    SOF0, followed by the three scans under SOS headers that name component 1, 2, 3."""
    from spotter_amd.synthetic import synthetic_image

    img = synthetic_image(23, h, w)
    grays = [jpeg(np.ascontiguousarray(img[..., c]), mode="L", quality=quality) for c in range(3)]
    g = grays[0]
    sof, sof_len = _segment(g, 0xC0)
    sos, sos_len = _segment(g, 0xDA)
    assert g[sof + 9] == 1 and sos_len == 10  # one component; SOS: FF DA 00 08 01 id tables 00 3F 00
    frame = b"\xff\xc0" + (17).to_bytes(2, "big") + g[sof + 4:sof + 9] + b"\x03" + b"".join(
        bytes([cid, 0x11, g[sof + 12]]) for cid in (1, 2, 3))
    out = g[:sof] + frame + g[sof + sof_len:sos]
    for cid, f in zip((1, 2, 3), grays):
        s, n = _segment(f, 0xDA)
        out += f[s:s + 5] + bytes([cid]) + f[s + 6:s + n] + f[s + n:-2]  # SOS header, then the data up to EOI
    return out + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def non_eligible() -> tuple:
    from spotter_amd.synthetic import synthetic_image

    img = synthetic_image(21, 120, 200)
    return (("progressive", jpeg(img, quality=85, progressive=True)),
            ("progressive 444", jpeg(img, quality=85, progressive=True, subsampling=0)),
            ("baseline, three non-interleaved scans", multi_scan_baseline()),
            ("test_pic", open(GOLDEN, "rb").read()))


@functools.lru_cache(maxsize=None)
def tail_junk() -> tuple:
    """Eligible files with N extra bytes after the last block of a segment: before EOI, and before a restart
    marker. The host decoder refuses them as extraneous data where it sees them, so the GPU path must not come
    back with status 0 there (a block begun in those bytes and not finished leaves no other trace than k != 0)."""
    from spotter_amd.synthetic import synthetic_image

    bases = [("gray 24x24", jpeg(synthetic_image(31, 24, 24), mode="L", quality=85)),
             ("gray 24x40", jpeg(synthetic_image(32, 24, 40), mode="L", quality=70)),
             ("rgb 40x56", jpeg(synthetic_image(33, 40, 56), quality=75)),
             ("rgb 444 17x33", jpeg(synthetic_image(34, 17, 33), quality=90, subsampling=0)),
             ("rgb restart 40x56", jpeg(synthetic_image(35, 40, 56), quality=80, restart_marker_blocks=2))]
    out = []
    for name, d in bases:
        spots = [("eoi", len(d) - 2)]
        if "restart" in name:
            rst = [i for i in range(len(d) - 1) if d[i] == 0xFF and 0xD0 <= d[i + 1] <= 0xD7]
            spots += [("rst0", rst[0]), (f"rst{len(rst) // 2}", rst[len(rst) // 2])]
        for where, at in spots:
            for n in (1, 2, 3, 4, 8, 13, 16, 24, 32, 48):
                for val in (0x00, 0x11, 0x55, 0xAA, 0xFF):
                    fill = (b"\xff\x00" if val == 0xFF else bytes([val])) * n
                    out.append((f"{name}:{n}x{val:02x}_before_{where}", d[:at] + fill + d[at:]))
    return tuple(out)
