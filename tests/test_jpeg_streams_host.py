"""CPU: the JPEG decode path on hand-built streams (tests/jpeg_stream_writer.py), no device call.

Every other JPEG in the suite was written by Pillow: 4:4:4 / 4:2:2 / 4:2:0, the Annex K Huffman tables under ids 0
and 1, 8-bit quantisation tables, component ids 1, 2, 3 under JFIF. The writer takes coefficient blocks and emits
the file, so here the blocks are the ground truth of the entropy decode, and the files reach what the parser and the
kernels accept beyond Pillow's encoder: 4:4:0, chroma components with different factors, luma 4x1 and 1x4, MCUs of 8
to 10 blocks, table ids 2 and 3, optimal and length-reversed Huffman tables, 16-bit quantisation tables, Adobe and
R,G,B colour rules, category-10 AC and category-11 DC magnitudes, blocks that end at coefficient 63.

1. The writer itself: at Pillow's three samplings, fed oracle.jpeg_enc_np's blocks, its scan is that encoder's.
2. For every case: Pillow loads it without a warning; sp_jpeg_decode_coefs returns the written blocks;
   oracle.jpeg_np.to_rgb of them is Pillow's pixels; the blocks are inside the IDCT envelope; the CPU emulation of the
   GPU entropy decode ends with status 0 and the written blocks. These are the conditions under which
   tests/test_gpu_jpeg_streams.py demands the GPU path for the same files.
3. Refusals: files Pillow's load raises on are UnsupportedJpeg from the decoder and from the packer (MCUs of 12
   blocks, scans naming the components out of frame order, an all-ones Huffman code); multi-scan files that name
   their components in an order Pillow takes keep decoding.
"""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_stream_writer as jw  # noqa: E402


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("subsampling", [0, 1, 2])
@pytest.mark.parametrize("size", [(1, 1), (17, 33), (48, 64)])
def test_writer_reproduces_the_reference_encoder(size, subsampling):
    """Blocks from oracle.jpeg_enc_np.coefficient_blocks, Annex K tables, JFIF: the entropy-coded bytes equal
    oracle.jpeg_enc_np.encode's (pinned to Pillow's own output in tests/test_jpeg_enc.py), and so does the file up to
    the order of its header segments."""
    from oracle.jpeg_enc_np import coefficient_blocks, encode

    from spotter_amd.synthetic import synthetic_image

    h, w = size
    img = synthetic_image(3 * h + w, h, w) if min(h, w) >= 2 else np.full((h, w, 3), 77, np.uint8)
    blocks, qt = coefficient_blocks(img, -1, subsampling)
    comps = [(b, bh, bv, min(c, 1), min(c, 1), min(c, 1), c + 1) for c, (b, bh, bv) in enumerate(blocks)]
    mine = jw.write(w, h, comps, {0: qt[0].tolist(), 1: qt[1].tolist()}, jw.STD, app=(jw.JFIF,))
    ref = encode(img, -1, subsampling)
    assert jw.scan_bytes(mine) == jw.scan_bytes(ref)
    assert mine == ref  # DQT, SOF0, DHT, SOS in jcmarker.c's order, as the writer emits them
    assert np.array_equal(jw.pillow_pixels(mine), np.asarray(Image.open(io.BytesIO(ref)).convert("RGB")))


def test_optimal_tables_are_valid_and_shorter():
    """gen_optimal_table: at most 16 bits, Kraft sum below 1 (the all-ones code stays free), every used symbol
    coded, and the scan is shorter than under the Annex K tables."""
    c = {x.name: x for x in jw.table_cases()}
    opt, std = c["optimal tables"], c["cb, cr on tables 2/3 and 3/2"]
    rng = np.random.default_rng(13)
    g = jw.random_blocks(rng, 53, 37, jw.S420)
    tabs = jw.optimal_tables(53, 37, jw.components(g, jw.S420))
    assert sorted(tabs) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    for bits, vals in tabs.values():
        assert len(bits) == 16 and sum(bits) == len(vals) == len(set(vals))
        assert sum(n * 2.0 ** -ln for ln, n in enumerate(bits, 1)) < 1.0
    assert len(opt.data) < len(std.data)
    # a skewed histogram that the unlimited code would give 20-bit lengths: limited to 16
    bits, vals = jw.gen_optimal_table([2 ** max(0, 24 - k) if k < 24 else 0 for k in range(256)])
    assert sum(bits) == 24 and max(ln for ln, n in enumerate(bits, 1) if n) == 16
    assert sum(n * 2.0 ** -ln for ln, n in enumerate(bits, 1)) < 1.0
    rb, rv = jw.reversed_lengths(jw.AC_LUM)
    assert rb == jw.AC_LUM[0] and sorted(rv) == sorted(jw.AC_LUM[1])
    from oracle.jpeg_enc_np import _derive

    assert _derive((rb, rv))[0x01][1] >= 12 and _derive((rb, rv))[0x00][1] >= 12  # the frequent symbols: long codes


@pytest.mark.parametrize("case", jw.all_cases(), ids=_ids(jw.all_cases()))
def test_case_meets_the_conditions_of_the_gpu_tests(case):
    from oracle.jpeg_np import simd_envelope_ok, to_rgb

    from spotter_amd.jpeg import decode_coefs, emulate_entropy, layout_dict

    ref = jw.pillow_pixels(case.data)  # warnings are errors there
    lay, co = decode_coefs(case.data)
    L = layout_dict(lay)
    assert L["color"] == case.color
    bad = np.argwhere(co != case.coefs)
    assert co.shape == case.coefs.shape and bad.size == 0, f"{len(bad)} coefficients differ, first at {bad[:3].tolist()}"
    assert simd_envelope_ok(co, L)
    got = to_rgb(co, L)
    assert got.shape == ref.shape and np.array_equal(got, ref)
    em = emulate_entropy(case.data)
    assert em is not None and em[2] == 0, em and em[2:]
    assert np.array_equal(em[1], case.coefs)


def test_case_lists_hold_what_they_are_meant_to():
    """Blocks per MCU from 1 to 10, table ids 2 and 3 in use, both colour rules, category-11 DC differences and
    category-10 AC values, restart segments of one MCU, and scans of more than two workgroups of subsequences."""
    from spotter_amd.jpeg import pack_scan

    scans = {c.name: pack_scan(c.data)[1] for c in jw.all_cases()}
    assert {s.bpm for s in scans.values()} >= {1, 3, 4, 5, 6, 8, 9, 10}
    assert scans["10-block MCU, ri=1"].bpm == 10 and scans["10-block MCU, ri=1"].nseg == scans["10-block MCU, ri=1"].nmcu > 1
    assert scans["restart interval above the MCU count"].nseg == 1
    assert scans["AC 1023, DC -1024/1023, ri=3"].nseg > 1
    for c in jw.workgroup_cases():
        assert scans[c.name].nsub > 2 * 256 and scans[c.name].stream_bits > 2 * 256 * 256, (c.name, scans[c.name].nsub)
    for c in jw.sampling_cases():
        if c.name.endswith("3x5"):
            assert scans[c.name].nmcu == 1
    assert {c.color for c in jw.colour_cases()} == {1, 2} and len(jw.colour_cases()) == 36
    assert len(jw.sampling_cases()) == 32
    ext = {c.name: c for c in jw.extreme_cases()}
    e = ext["AC 1023, DC -1024/1023"]
    assert e.coefs[:, 0].min() == -1024 and e.coefs[:, 0].max() == 1023 and abs(e.coefs[:, 1:]).max() == 1023
    assert np.abs(np.diff(e.blocks[1][0, :, 0])).max() == 2047  # a category-11 difference within a chroma row
    assert all(np.count_nonzero(b[1:]) == 1 and b[63] for b in ext["only coefficient 63"].coefs)
    assert all(np.count_nonzero(b[1:]) == 63 for b in ext["all 63 AC non-zero"].coefs)


def test_16_bit_table_outside_the_envelope_is_flagged():
    """The one case deliberately outside the envelope: the stream decodes to the written blocks, the dequantised
    values leave the range shared with libjpeg-turbo's SIMD IDCT, so the decoder must leave the file to Pillow
    (tests/test_gpu_jpeg_streams.py asserts UnsupportedJpeg from JpegDecoder.decode)."""
    from oracle.jpeg_np import simd_envelope_ok

    from spotter_amd.jpeg import decode_coefs, layout_dict

    case = jw.outside_envelope_case()
    jw.pillow_pixels(case.data)
    lay, co = decode_coefs(case.data)
    assert np.array_equal(co, case.coefs) and max(lay.quant[0]) == 1000
    assert not simd_envelope_ok(co, layout_dict(lay))


@pytest.mark.parametrize("name,data", jw.refused_cases(), ids=[n for n, _ in jw.refused_cases()])
def test_files_pillow_refuses_are_refused(name, data):
    from spotter_amd.jpeg import UnsupportedJpeg, decode_coefs, pack_scan

    with pytest.raises(Exception):  # noqa: B017, PT011 - whatever Pillow raises: the file is Pillow's to refuse
        jw.pillow_pixels(data)
    with pytest.raises(UnsupportedJpeg):
        decode_coefs(data)
    with pytest.raises(UnsupportedJpeg):
        pack_scan(data)


@pytest.mark.parametrize("case", jw.subset_scan_cases(), ids=_ids(jw.subset_scan_cases()))
def test_scans_in_an_order_pillow_takes_keep_decoding(case):
    """The other side of the scan-order rule: sequential files of several scans whose components are named as
    libjpeg accepts them (2,1 then 0 among them) decode to the written blocks and Pillow's pixels."""
    from oracle.jpeg_np import to_rgb

    from spotter_amd.jpeg import decode_coefs, layout_dict, pack_scan

    ref = jw.pillow_pixels(case.data)
    lay, co = decode_coefs(case.data)
    assert np.array_equal(co, case.coefs)
    assert np.array_equal(to_rgb(co, layout_dict(lay)), ref)
    assert pack_scan(case.data) is None  # more than one scan: not eligible for the GPU entropy decode


def test_luma_4x1_over_chroma_1x1_is_declined_by_design(monkeypatch):
    """Chroma four times below luma: Pillow decodes it, the parser does not implement the ratio and says so, and the
    drop-in's open then returns Pillow's own image (here with a decoder that only parses: no device)."""
    from spotter_amd import jpeg
    from spotter_amd.jpeg import UnsupportedJpeg, decode_coefs, pack_scan

    data = jw.luma_4x1_chroma_1x1()
    jw.pillow_pixels(data)
    with pytest.raises(UnsupportedJpeg, match="ratio"):
        decode_coefs(data)
    with pytest.raises(UnsupportedJpeg, match="ratio"):
        pack_scan(data)

    class ParseOnly:
        def decode(self, d):
            decode_coefs(d)
            raise AssertionError("the parser took the file")

    monkeypatch.setattr(jpeg, "decoder", lambda *a, **k: ParseOnly())
    im = jpeg.image_module().open(io.BytesIO(data))
    assert type(im) is type(Image.open(io.BytesIO(data))) and im.mode == "RGB"
    assert np.array_equal(np.asarray(im.convert("RGB")), jw.pillow_pixels(data))
