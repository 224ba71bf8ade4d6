"""CPU: the case lists of tests/jpeg_idct_cases.py, no device call. These are the conditions under which
tests/test_gpu_jpeg_stages.py may demand, bit for bit, the status words, the IDCT planes and the pixels of
oracle.jpeg_np from the kernels of csrc/jpeg.hip:

1. every class of envelope block is there in full and each block trips exactly the conditions of its label (recomputed
   here from oracle.jpeg_np._islow_1d), the boundary classes sit exactly at 511 / 512 / -512 / -513, and
   oracle.jpeg_np.simd_envelope_ok, the mirror of the kernel's flag, says any(label);
2. Pillow loads every file with warnings as errors and sp_jpeg_decode_coefs returns the written blocks;
3. oracle.jpeg_np.to_rgb is Pillow's pixels for every case that is not flagged, and for the flagged blocks exactly
   at 512 and -513 Pillow's pixels are not the C-semantics ones: the flag is what keeps wrong pixels from being served;
4. no three-table frame, edge-grid case or colour frame is outside the envelope;
5. the layout facts the GPU tests lean on: component boundaries inside a workgroup of 32 blocks, a frame of fewer
   than 32 blocks, chroma widths and heights of 1, 2 and 3 in every upsampling form, all 65 536 value pairs in the
   colour frames' planes.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_idct_cases as jc  # noqa: E402
import jpeg_stream_writer as jw  # noqa: E402


def _decoded(case):
    """(layout dict, coefficients) of the host decode, the coefficients checked against the written blocks."""
    from spotter_amd.jpeg import decode_coefs, layout_dict

    lay, co = decode_coefs(case.data)
    bad = np.argwhere(co != case.coefs)
    assert co.shape == case.coefs.shape and bad.size == 0, \
        f"{case.name}: {len(bad)} coefficients differ, first at {bad[:3].tolist()}"
    return layout_dict(lay), co


def _inside_and_pillows(case):
    """Pillow loads the file (warnings are errors), the host decoder returns the written blocks, they are inside
    the envelope, and the oracle's pixels are Pillow's."""
    from oracle.jpeg_np import simd_envelope_ok, to_rgb

    ref = jw.pillow_pixels(case.data)
    L, co = _decoded(case)
    assert L["color"] == case.color, case.name
    assert simd_envelope_ok(co, L), case.name
    got = to_rgb(co, L)
    assert got.shape == ref.shape and np.array_equal(got, ref), case.name
    return L, co


# ------------------------------------------------------------------------------------------------ envelope blocks
def test_every_envelope_class_is_full_and_sits_where_its_name_says():
    by = {}
    for b in jc.envelope_blocks():
        by.setdefault(b.cls, []).append(b)
    for cls in jc._CLASSES:
        assert len(by[cls]) == (jc._NPLAIN if cls == "inside" else jc._N), (cls, len(by.get(cls, ())))
    assert len(by["16-bit table"]) == 5
    none = (False, False, False, False)
    for b in by["inside, max 511"]:
        assert b.label == none and b.hi == 511
    for b in by["high alone, max 512"]:
        assert b.label == (False, False, True, False) and b.hi == 512 and b.lo >= -512
    for b in by["inside, min -512"]:
        assert b.label == none and b.lo == -512
    for b in by["low alone, min -513"]:
        assert b.label == (False, False, False, True) and b.lo == -513 and b.hi <= 511
    for b in by["both pass-2 bounds"]:
        assert b.label == (False, False, True, True)
    for b in by["pass 1 with pass 2"]:
        assert not b.label[0] and b.label[1] and (b.label[2] or b.label[3])
    for b in by["inside, pass 1 >= 16000"]:
        assert b.label == none and 16000 <= b.p1 <= jc.ENV16
    for b in by["inside"]:
        assert b.label == none
    # the DC-only blocks under a table of 8: pass 1 is 32 * DC, every sample is DC
    dc = {v: by[f"DC {v} under table 8"][0] for v in (511, 512, -512, -513)}
    assert dc[511].label == none and (dc[511].p1, dc[511].hi, dc[511].lo) == (16352, 511, 511)
    assert dc[512].label == (False, True, True, False) and dc[512].p1 == 16384
    assert dc[-512].label == (False, True, False, False) and (dc[-512].p1, dc[-512].lo) == (16384, -512)  # pass 1 alone
    assert dc[-513].label == (False, True, False, True)
    for b in by["16-bit table"]:
        assert b.label[0] and b.quant.max() > 255
    # the plain inside blocks fill the sample range: every pass-2 value of [-512, 511] occurs among them
    from oracle.jpeg_np import CB, P1, _islow_1d

    blocks = np.stack([b.coefs[0].astype(np.int64) * b.quant for b in by["inside"] + by["inside, max 511"]
                       + by["inside, min -512"]]).reshape(-1, 8, 8)
    ws = _islow_1d(np.swapaxes(blocks, 1, 2), CB - P1)
    out = _islow_1d(np.swapaxes(ws, 1, 2), CB + P1 + 3)
    assert np.array_equal(np.unique(out), np.arange(-512, 512))
    # all four conditions occur, alone where they can (below) and together
    assert {b.label for b in jc.envelope_blocks()} >= {none, (False, False, True, False), (False, False, False, True),
                                                       (False, True, False, False), (False, False, True, True)}
    assert all(b.quant.max() <= 255 for b in jc.envelope_blocks() if b.cls != "16-bit table")


def test_interleaving_puts_flagged_blocks_into_every_call_of_64():
    order = jc.interleaved(jc.envelope_blocks())
    assert sorted(b.name for b in order) == sorted(b.name for b in jc.envelope_blocks())
    for i in range(0, len(order), 64):
        flags = [b.flagged for b in order[i:i + 64]]
        assert 4 <= sum(flags) <= len(flags) - 4, (i, sum(flags))
        # inside blocks with a flagged neighbour on either side, flagged ones between inside ones
        assert any(flags[k] and not flags[k - 1] and not flags[k + 1] for k in range(1, len(flags) - 1)), i


@pytest.mark.parametrize("cls", list(jc._CLASSES) + ["DC", "16-bit table"])
def test_envelope_blocks_decode_and_carry_their_label(cls):
    """Per block: Pillow loads the file, the host decoder returns the block and its table, simd_envelope_ok (the
    mirror of the kernel's flag) is `not flagged`, an inside block's oracle pixels are Pillow's. For the flagged blocks
    whose largest sample is exactly 512, or smallest exactly -513, Pillow's pixels differ from the C-semantics ones:
    512 wraps to -512 (black) under & 1023 where the SIMD packs saturate to white, and -513 to 511."""
    from oracle.jpeg_np import simd_envelope_ok, to_rgb

    blocks = [b for b in jc.envelope_blocks() if b.cls == cls or (cls == "DC" and b.cls.startswith("DC "))]
    assert blocks
    for b in blocks:
        ref = jw.pillow_pixels(b.data)
        L, co = _decoded(b)
        assert L["total_blocks"] == 1 and L["quant"][0] == b.quant.tolist(), b.name
        assert simd_envelope_ok(co, L) == (not b.flagged), b.name
        got = to_rgb(co, L)
        if not b.flagged:
            assert np.array_equal(got, ref), b.name
        elif cls in ("high alone, max 512", "low alone, min -513"):
            assert not np.array_equal(got, ref), b.name


def test_the_dequantised_bound_never_trips_without_pass_2():
    """The issue asks for a block under a 16-bit table that trips only the dequantised and pass-1 bounds. None
    exists. The two passes together are 8 times an orthonormal transform, so 64 samples within [-512, 511] bound the
    sum of squares of the dequantised coefficients by 64 * (8 * 512)^2 / 64, each coefficient by 8 * 512 = 4096
    (plus the integer IDCT's rounding): far below 2^14. A seeded search agrees: blocks of one to four coefficients
    dequantised to 16384..65535 in magnitude, the rest small, all trip a pass-2 bound."""
    rng = np.random.default_rng(25)
    n = 20000
    blocks = rng.integers(-3, 4, (n, 64))
    quant = np.ones((n, 64), np.int64)
    for _ in range(4):
        pos = rng.integers(0, 64, n)
        on = rng.random(n) < 0.6
        on[0] = True
        quant[np.arange(n)[on], pos[on]] = rng.integers(16384, 65536, on.sum())
        blocks[np.arange(n)[on], pos[on]] = rng.choice([-1, 1], on.sum())
    lab, deq, _, _, _ = jc.envelope_terms(blocks, quant)
    tripped = lab[:, 0]
    assert tripped.sum() > n // 2 and (lab[tripped, 2] | lab[tripped, 3]).all()
    # and over the search that feeds the classes: whenever pass 2 is inside, the dequantised values are within 4096
    # and a rounding margin
    b, q = jc._search_round(np.random.default_rng(26), 16384)
    lab, deq, p1, hi, lo = jc.envelope_terms(b, q)
    inside2 = ~(lab[:, 2] | lab[:, 3])
    assert inside2.sum() > 1000 and deq[inside2].max() <= 4096 + 8
    # pass 1 alone: only the DC -512 block's kind, a row whose pass-1 DC term is -16384 .. -16400 (the values pass 2
    # still rounds to -512: (-16400 * 8192 + 2^17) >> 18 = -512) and whose samples are all -512
    alone = lab[:, 1] & inside2
    assert alone.any() and (lo[alone] == -512).all() and (p1[alone] >= 16384).all() and (p1[alone] <= 16400).all()


# ------------------------------------------------------------------------------------------------ frames
@pytest.mark.parametrize("case", jc.three_table_frames(), ids=[c.name for c in jc.three_table_frames()])
def test_three_table_frames(case):
    """Three different tables reach the layout, the blocks are dense, and the block counts put both component
    boundaries inside a workgroup of 32 blocks with a partial last workgroup."""
    L, co = _inside_and_pillows(case)
    assert L["quant"][0] == jw.Q1 and L["quant"][1] == jc.Q3 and L["quant"][2] == jc.QGRADED
    assert L["block_off"][1] % 32 and L["block_off"][2] % 32 and L["total_blocks"] % 32
    assert (np.count_nonzero(co, axis=1) >= 32).all()
    # reading Cb's table for Cr, or Y's for either, changes the planes: the tables differ where the blocks are not 0
    from oracle.jpeg_np import planes

    swapped = dict(L, quant=[L["quant"][0], L["quant"][1], L["quant"][1]])
    assert not np.array_equal(planes(co, swapped)[2], planes(co, L)[2])


def test_three_table_frames_cover_the_layouts():
    from spotter_amd.jpeg import decode_coefs

    lays = [decode_coefs(c.data)[0] for c in jc.three_table_frames()]
    assert {(tuple(l.h), tuple(l.v)) for l in lays} == {((1, 1, 1), (1, 1, 1)), ((2, 1, 1), (2, 1, 1)),
                                                        ((2, 2, 1), (2, 1, 2))}
    assert min(l.total_blocks for l in lays) < 32 < max(l.total_blocks for l in lays)
    # a workgroup that holds blocks of all three components, and frames of several workgroups
    assert any(l.block_off[2] < 32 for l in lays) and sum(l.total_blocks > 64 for l in lays) >= 2


@pytest.mark.parametrize("layout", [lab for lab, _ in jc.EDGE_LAYOUTS])
def test_edge_grid(layout):
    cases = [c for c in jc.edge_grid() if c.layout == layout]
    assert len(cases) == len(jc.EDGE_SIZES) ** 2
    for c in cases:
        _inside_and_pillows(c)


def test_edge_grid_reaches_every_chroma_width_and_height():
    """dw and dh of 1, 2 and 3 (box replication at dw <= 2, the single-row case dh == 1, the first fancy widths) in
    each of h2v1, h1v2 and h2v2, and widths at which a 4-pixel group of the batch colour kernel spans rows."""
    from spotter_amd.jpeg import decode_coefs

    seen = {}
    for c in jc.edge_grid():
        lay = decode_coefs(c.data)[0]
        for k in (1, 2):
            rh, rv = lay.max_h // lay.h[k], lay.max_v // lay.v[k]
            dw = -(-lay.width * lay.h[k] // lay.max_h)
            dh = -(-lay.height * lay.v[k] // lay.max_v)
            seen.setdefault((rh, rv), set()).add((dw, dh))
    assert set(seen) == {(1, 1), (2, 1), (1, 2), (2, 2)}
    for form in ((2, 1), (1, 2), (2, 2)):
        assert {(dw, dh) for dw in (1, 2, 3) for dh in (1, 2, 3)} <= seen[form], form
    assert len(jc.edge_grid()) == 810 and {1, 2, 3, 5} <= set(jc.EDGE_SIZES)


@pytest.mark.parametrize("case", jc.colour_frames(), ids=[c.name for c in jc.colour_frames()])
def test_colour_frames_hold_every_pair(case):
    """The ramp planes come back from the integer IDCT exactly, so the frame's planes hold all 65 536 pairs of its
    two ramp components; the third plane is noise over the whole range."""
    from oracle.jpeg_np import planes

    L, co = _inside_and_pillows(case)
    pl = planes(co, L)
    cx, cy = case.pair
    ramp = np.arange(256, dtype=np.uint8)
    assert np.array_equal(pl[cx], np.broadcast_to(ramp[None, :], (256, 256)))
    assert np.array_equal(pl[cy], np.broadcast_to(ramp[:, None], (256, 256)))
    pairs = np.unique(pl[cx].astype(np.int64) * 256 + pl[cy])
    assert pairs.size == 65536
    third = pl[3 - cx - cy]
    assert third.min() == 0 and third.max() == 255 and np.unique(third).size == 256


def test_colour_frames_cover_the_three_pairs():
    assert sorted(c.pair for c in jc.colour_frames()) == [(0, 1), (0, 2), (1, 2)]
