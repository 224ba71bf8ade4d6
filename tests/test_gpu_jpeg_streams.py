"""GPU: the JPEG decode kernels on hand-built streams (tests/jpeg_stream_writer.py), the files Pillow's encoder never
writes: csrc/jpeg.hip's h1v2 chroma branch, chroma components with different factors in one frame, the
no-conversion colour path (color == 2), MCUs of 7-10 blocks in the entropy decode's Geom / block_index, huff_sym's
slow path under tables other than Annex K's, table ids 2 and 3, 16-bit quantisation tables.

For every case, through JpegDecoder(dev) and JpegDecoder(dev, entropy="gpu"): the pixels are Pillow's bit for bit;
the coefficients on the device are the blocks the file was written from; under entropy="gpu" the GPU path ran (stats)
with no fallback. tests/test_jpeg_streams_host.py asserts on the CPU, for the same lists, the conditions that make
this demand fair (Pillow loads the file, the blocks are inside the IDCT envelope, the CPU emulation of the entropy
decode ends with status 0)."""
import io
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from PIL import Image  # noqa: E402

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_stream_writer as jw  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def decoders(dev):
    from spotter_amd.jpeg import JpegDecoder

    return JpegDecoder(dev), JpegDecoder(dev, entropy="gpu")


def _ids(cases):
    return [c.name for c in cases]


def _same(got, ref, name):
    g = got.cpu().numpy()
    assert g.shape == ref.shape and g.dtype == np.uint8, (name, g.shape, ref.shape)
    bad = np.argwhere(g != ref)
    assert bad.size == 0, f"{name}: {len(bad)} samples differ, first at {bad[:3].tolist()}"


def _same_coefs(dev_coefs, case, path):
    co = dev_coefs[:case.coefs.size].cpu().numpy().reshape(-1, 64)
    bad = np.argwhere(co != case.coefs)
    assert bad.size == 0, f"{case.name} ({path}): {len(bad)} coefficients differ, first at {bad[:3].tolist()}"


def _check(case, decoders):
    from spotter_amd.jpeg import decode_coefs

    host, gpu = decoders
    ref = jw.pillow_pixels(case.data)
    lay, _ = decode_coefs(case.data)
    assert lay.color == case.color and lay.total_blocks * 64 == case.coefs.size
    _same(host.decode(case.data), ref, case.name + " (host entropy)")
    _same_coefs(host._coefs, case, "host entropy")
    before = gpu.stats["gpu"], sum(gpu.stats["fallback"].values()), gpu.stats["host"]
    _same(gpu.decode(case.data), ref, case.name + " (gpu entropy)")
    after = gpu.stats["gpu"], sum(gpu.stats["fallback"].values()), gpu.stats["host"]
    if case.demand_gpu:
        assert after == (before[0] + 1, before[1], before[2]), (case.name, gpu.stats)
        _same_coefs(gpu._g["coefs"], case, "gpu entropy")
    else:  # a periodic stream: Pillow's pixels by whichever path, as test_gpu_jpeg_entropy.py's resistant frames
        assert after[0] + after[1] == before[0] + before[1] + 1 and after[2] == before[2], (case.name, gpu.stats)


@pytest.mark.parametrize("case", jw.sampling_cases(), ids=_ids(jw.sampling_cases()))
def test_sampling_layouts(case, decoders):
    """4:4:0 (h1v2), mixed chroma factors, 8- to 10-block MCUs, luma 4x1 and 1x4, gray declaring 2x2; 3x5 (one MCU,
    chroma at most 2 wide: the box branch), exact MCU multiples, ragged right and bottom edges."""
    _check(case, decoders)


@pytest.mark.parametrize("case", jw.colour_cases(), ids=_ids(jw.colour_cases()))
def test_colour_rules(case, decoders):
    """Adobe transform 0 / 1, R,G,B ids with and without JFIF, JFIF over Adobe 0, ids 0,1,2: layout.color (asserted
    in _check) and the pixels, at 4:4:4, 4:2:0, 4:4:0."""
    _check(case, decoders)


@pytest.mark.parametrize("case", jw.table_cases(), ids=_ids(jw.table_cases()))
def test_tables(case, decoders):
    _check(case, decoders)


@pytest.mark.parametrize("case", jw.extreme_cases(), ids=_ids(jw.extreme_cases()))
def test_coefficient_extremes(case, decoders):
    _check(case, decoders)


@pytest.mark.parametrize("case", jw.workgroup_cases(), ids=_ids(jw.workgroup_cases()))
def test_several_workgroups(case, decoders):
    _check(case, decoders)


def test_16_bit_table_outside_the_envelope_is_left_to_pillow(dev):
    """Dequantised values past the range shared with libjpeg-turbo's SIMD IDCT: UnsupportedJpeg by either entropy
    path (the GPU one decodes the stream, sees the IDCT's flag and hands over to the host path, which raises)."""
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg

    case = jw.outside_envelope_case()
    with pytest.raises(UnsupportedJpeg, match="IDCT range"):
        JpegDecoder(dev).decode(case.data)
    d = JpegDecoder(dev, entropy="gpu")
    with pytest.raises(UnsupportedJpeg, match="IDCT range"):
        d.decode(case.data)
    assert d.stats["gpu"] == 0 and d.stats["fallback"] == {1: 1}
    _same_coefs(d._g["coefs"], case, "gpu entropy")


def test_refused_files_raise_by_either_path(dev):
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg

    for d in (JpegDecoder(dev), JpegDecoder(dev, entropy="gpu")):
        for name, data in jw.refused_cases() + (("luma 4x1 chroma 1x1", jw.luma_4x1_chroma_1x1()),):
            with pytest.raises(UnsupportedJpeg):
                d.decode(data)
        assert d.stats["gpu"] == d.stats["host"] == 0 and not d.stats["fallback"], d.stats


def test_drop_in_keeps_pillows_image_for_luma_4x1_chroma_1x1(dev):
    from spotter_amd import jpeg

    data = jw.luma_4x1_chroma_1x1()
    im = jpeg.image_module(dev).open(io.BytesIO(data))
    assert type(im) is type(Image.open(io.BytesIO(data)))
    assert np.array_equal(np.asarray(im.convert("RGB")), jw.pillow_pixels(data))


def _batch_files():
    """One decode_many chunk: blocks per MCU 1 / 3 / 4 / 5 / 6 / 8 / 9 / 10, both colour rules, Annex K / reversed /
    optimal / ids-2-3 tables, gray, restart files, a multi-workgroup scan next to one-MCU files, a 12-block refusal,
    a file outside the envelope and a progressive Pillow file."""
    from jpeg_entropy_cases import jpeg

    from spotter_amd.synthetic import synthetic_image

    by_name = {c.name: c for c in jw.all_cases()}
    names = ["440 70x41", "y2x2 cb2x1 cr1x2 37x29", "y2x2 cb2x2 cr1x1 70x41", "y4x1 2x1 2x1 3x5", "y1x4 1x2 1x2 37x29",
             "y2x1 cb1x1 cr2x1 16x16", "gray 2x2 37x29", "adobe 0 420 53x37", "RGB ids 444 3x5", "RGB ids jfif 440 53x37",
             "cb, cr on tables 2/3 and 3/2", "16-bit dqt", "optimal tables", "reversed AC lengths",
             "AC 1023, DC -1024/1023, ri=3", "10-block MCU, ri=1", "dense 96x80, optimal tables", "440 3x5"]
    files = [(n, by_name[n].data) for n in names]
    eligible = len(files)
    files.insert(3, jw.refused_cases()[0])
    files.insert(9, ("progressive", jpeg(synthetic_image(21, 40, 56), quality=85, progressive=True)))
    files.insert(14, (jw.outside_envelope_case().name, jw.outside_envelope_case().data))
    return files, eligible


def test_mixed_batch_equals_decode(dev, decoders):
    """decode_many over one chunk that mixes the files above, in both orders (a per-image index that leaks across
    images shows when its neighbours change): every entry is decode()'s pixels (Pillow's) or its UnsupportedJpeg, and
    batch_stats counts every eligible file as decoded by the GPU chain."""
    from spotter_amd._lib import SP_JPEG_BATCH_MAX
    from spotter_amd.jpeg import JpegDecoder, UnsupportedJpeg

    files, eligible = _batch_files()
    assert 12 <= len(files) <= SP_JPEG_BATCH_MAX
    want = []
    for name, data in files:
        try:
            px = decoders[0].decode(data).cpu().numpy()
            assert np.array_equal(px, np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))), name
            want.append(px)
        except UnsupportedJpeg:
            want.append(None)
    assert sum(w is None for w in want) == 2
    for entropy in ("host", "gpu"):
        d = JpegDecoder(dev, entropy=entropy)
        for rep, order in enumerate((list(range(len(files))), list(range(len(files)))[::-1])):
            got = d.decode_many([files[i][1] for i in order], max_workers=2)
            assert len(got) == len(files)
            for g, i in zip(got, order):
                if want[i] is None:
                    assert isinstance(g, UnsupportedJpeg), (files[i][0], entropy)
                else:
                    assert torch.is_tensor(g), (files[i][0], entropy, g)
                    _same(g, want[i], f"{files[i][0]} ({entropy}, order {rep})")
            st = d.batch_stats
            assert st["calls"] == rep + 1 and st["refused"] == st["flagged"] == rep + 1, st
            if entropy == "gpu":
                assert st["gpu"] == (rep + 1) * eligible and st["host"] == rep + 1, st
                assert st["fallback"] == {1: rep + 1}, st  # the file outside the envelope, flagged by the IDCT
                assert st["chunks"] == 2 * (rep + 1), st   # one GPU-entropy chunk, one host chunk
            else:
                assert st["gpu"] == st["host"] == 0 and st["chunks"] == rep + 1, st
