"""CPU: the premises of tests/test_gpu_jpeg_enc_stages.py, so that a pass there means something.

For every case of tests/jpeg_enc_cases.py the numpy oracle writes Pillow's bytes; the "runs" images give exactly the
blocks they were built for; over the whole table, and for the luma AND the chroma Huffman tables, the entropy walk's
special paths are reached (1, 2 and 3 ZRL codes in a block, a block without EOB, AC sizes 1..10, DC-difference sizes
0..11, every run length 0..15, an MCU shorter than 16 bits), and some raw stream holds a 0xFF byte; no block codes to
more bits than the bound behind sp_jpeg_enc_plan's bits_cap; the oracle's per-stage views (scan_order_blocks,
mcu_bit_counts) agree with entropy_bits and with the library's own decode of the oracle's file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_enc_cases as ec  # noqa: E402

from oracle import jpeg_enc_np as J  # noqa: E402

MAX_BITS_PER_BLOCK = 22 + 63 * 26 + 16  # jpeg_host.h kMaxBitsPerBlock, the bound behind bits_cap


def _family_ids():
    """Small families as one test each, the larger images one test per case."""
    out = [(f, None) for f in ("geometry", "runs", "saturation", "flat")]
    return out + [("mcu_counts", c[0]) for c in ec.mcu_count_cases()]


def _cases_of(family, cid):
    return [ec.case_by_id(cid)] if cid else list(ec.FAMILIES[family]())


@pytest.mark.parametrize("family,cid", _family_ids(), ids=[c or f for f, c in _family_ids()])
def test_oracle_writes_pillows_bytes_and_stages_agree(family, cid):
    """encode == Pillow; sum(mcu_bit_counts) == nbits; every block within the bits_cap bound; scan_order_blocks has
    the MCU-interleaved shape."""
    for case in _cases_of(family, cid):
        name, rgb, q, sub = case
        ref = ec.reference(name)
        assert J.encode(rgb, q, sub) == ref.pillow, name
        assert int(ref.mcu_bits.sum()) == ref.nbits, name
        assert len(ref.raw) == (ref.nbits + 7) // 8, name
        hs, vs = J.SAMPLING[sub]
        H, W, _ = rgb.shape
        assert ref.nmcu == -(-W // (8 * hs)) * -(-H // (8 * vs)) and ref.bpm == hs * vs + 2, name
        assert ref.blocks.shape == (ref.nmcu * ref.bpm, 64) and ref.blocks.dtype == np.int16, name
        assert ref.mcu_bits.max() <= ref.bpm * MAX_BITS_PER_BLOCK, name
        per_block = [sum(s for _, s in codes) for _, _, (codes, *_r) in J._walk_scan(ref.comps)]
        assert len(per_block) == ref.nmcu * ref.bpm and max(per_block) <= MAX_BITS_PER_BLOCK, (name, max(per_block))


def test_mcu_bit_counts_restate_the_stream():
    """Independently of the shared walk: cutting the raw stream at the cumulative counts and decoding each piece
    with the Annex K tables returns that MCU's blocks (one case per subsampling with dense content)."""
    for name in ("geo 17x25 s0", "geo 25x17 s1", "geo 24x25 s2", "runs colour 444"):
        ref = ec.reference(name)
        bits = np.unpackbits(np.frombuffer(ref.raw, np.uint8))[:ref.nbits]
        dec = [{(code, ln): sym for sym, (code, ln) in J._derive(t).items()}
               for t in (J.DC_LUM, J.AC_LUM, J.DC_CHR, J.AC_CHR)]
        ny = ref.bpm - 2
        last = [0, 0, 0]
        pos = 0

        def sym(table):
            nonlocal pos
            code = 0
            for ln in range(1, 17):
                code = (code << 1) | int(bits[pos])
                pos += 1
                if (code, ln) in table:
                    return table[(code, ln)]
            raise AssertionError("no code")

        def mag(n):
            nonlocal pos
            if n == 0:
                return 0
            v = int("".join(map(str, bits[pos:pos + n])), 2)
            pos += n
            return v if v >> (n - 1) else v - (1 << n) + 1

        for m in range(ref.nmcu):
            assert pos == ref.offsets[m], (name, m)
            for j in range(ref.bpm):
                c = 0 if j < ny else j - ny + 1
                blk = np.zeros(64, np.int64)
                last[c] += mag(sym(dec[0 if c == 0 else 2]))
                blk[0] = last[c]
                k = 1
                while k < 64:
                    s = sym(dec[1 if c == 0 else 3])
                    if s == 0:
                        break
                    k += s >> 4
                    if s & 15:
                        blk[k] = mag(s & 15)
                    k += 1
                assert np.array_equal(blk, ref.blocks[m * ref.bpm + j]), (name, m, j)
        assert pos == ref.nbits


def test_runs_images_give_their_targets():
    """The oracle's luma blocks of the gray images equal the targets (Cb = Cr = 0 throughout); the colour image's
    Cb / Cr blocks equal theirs."""
    t = ec.run_targets()
    for name in ("runs gray 444", "runs gray 420"):
        comps = ec.reference(name).comps
        assert np.array_equal(comps[0][0][:4, :12], t), name
        assert not comps[1][0].any() and not comps[2][0].any(), name
    tcb, tcr = ec.colour_run_targets()
    for name in ("runs colour 444", "runs colour 420"):
        comps = ec.reference(name).comps
        assert np.array_equal(comps[1][0][:6, :12], tcb), name
        assert np.array_equal(comps[2][0][:6, :12], tcr), name


def _merged_histogram(cases):
    tot = {k: {"ac": set(), "dc": set(), "zrl": set(), "no_eob": False} for k in ("luma", "chroma")}
    lo, hi = 1 << 30, 0
    for c in cases:
        h = J.symbol_histogram(ec.reference(c[0]).comps)
        for k in tot:
            tot[k]["ac"] |= h[k]["ac"]
            tot[k]["dc"] |= h[k]["dc"]
            tot[k]["zrl"] |= h[k]["zrl"]
            tot[k]["no_eob"] |= h[k]["no_eob"]
            assert h[k]["max_zrl"] == max(h[k]["zrl"], default=0)
        lo, hi = min(lo, h["mcu_bits"][0]), max(hi, h["mcu_bits"][1])
    return tot, (lo, hi)


def test_table_reaches_every_class_in_both_huffman_tables():
    cases = ec.all_cases()
    tot, (lo, hi) = _merged_histogram(cases)
    for k in ("luma", "chroma"):
        t = tot[k]
        assert {1, 2, 3} <= t["zrl"], (k, t["zrl"])
        assert t["no_eob"], k
        assert {s for _, s in t["ac"]} >= set(range(1, 11)), (k, sorted({s for _, s in t["ac"]}))
        assert t["dc"] >= set(range(12)), (k, sorted(t["dc"]))
        assert {r for r, _ in t["ac"]} >= set(range(16)), (k, sorted({r for r, _ in t["ac"]}))
    assert lo < 16, lo  # every MCU holds both tables' codes
    assert any(b"\xff" in ec.reference(c[0]).raw for c in cases)


def test_plan_bounds_every_case_and_restates_the_layout():
    """sp_jpeg_enc_plan: bits_cap * 8 >= nbits for every case; work_bytes is the layout the stage tests read."""
    from spotter_amd._lib import SpJpegEncLayout, load

    L = load()
    for name, rgb, q, sub in ec.all_cases():
        ref = ec.reference(name)
        lay = SpJpegEncLayout()
        H, W, _ = rgb.shape
        assert L.sp_jpeg_enc_plan(W, H, q, sub, C.byref(lay)) == 0, name
        nmcu = lay.mcux * lay.mcuy
        coef_off = -(-(8 + 12 * nmcu) // 256) * 256
        assert lay.work_bytes == coef_off + lay.total_blocks * 128, name
        assert lay.bits_cap * 8 >= lay.total_blocks * MAX_BITS_PER_BLOCK, name
        assert (nmcu, lay.bpm) == (ref.nmcu, ref.bpm) and lay.bits_cap * 8 >= ref.nbits, name


def _decoded_in_scan_order(data, ref):
    """The library's host entropy decode of a baseline file, rearranged from component planes (natural order) to the
    scan's order (zig-zag)."""
    from spotter_amd.jpeg import decode_coefs

    lay, co = decode_coefs(data)
    hs, vs = J.SAMPLING[ref.sub]
    per = []
    for c in range(3):
        h, v = (hs, vs) if c == 0 else (1, 1)
        bw, bh = lay.bw[c], lay.bh[c]
        pl = co[lay.block_off[c]:lay.block_off[c] + bw * bh].reshape(bh, bw, 64)
        mcuy, mcux = bh // v, bw // h
        per.append(pl.reshape(mcuy, v, mcux, h, 64).transpose(0, 2, 1, 3, 4).reshape(mcuy * mcux, v * h, 64))
    return np.concatenate(per, axis=1)[..., J.NATURAL].reshape(-1, 64)


@pytest.mark.parametrize("family", ["geometry", "runs", "saturation", "flat"])
def test_decoding_the_oracles_file_returns_scan_order_blocks(family):
    for name, rgb, q, sub in ec.FAMILIES[family]():
        ref = ec.reference(name)
        got = _decoded_in_scan_order(ref.pillow, ref)  # == the oracle's file, asserted above
        assert got.shape == ref.blocks.shape and np.array_equal(got, ref.blocks), name


def test_decoding_the_oracles_file_returns_scan_order_blocks_many_mcus():
    for name in ("mcus 257 x1", "mcus 1025 x5", "mcus 1025 x5 420"):
        ref = ec.reference(name)
        assert np.array_equal(_decoded_in_scan_order(ref.pillow, ref), ref.blocks), name
