"""A baseline JPEG stream writer for the decoder tests, numpy only: it takes quantised coefficient blocks and emits
the file, so the blocks themselves are the exact reference of every entropy decode (host decoder, CPU emulation, GPU
kernels) and nothing about the file is limited to what Pillow's encoder writes: any sampling factors, any Huffman
tables under ids 0-3, 8- or 16-bit quantisation tables, any component ids and APPn segments, restart intervals, any
scan order. tests/test_jpeg_streams_host.py pins the writer (Pillow's three samplings: the scan bytes are
oracle.jpeg_enc_np.encode's) and every case list below on the CPU; tests/test_gpu_jpeg_streams.py runs the same
lists through the kernels.

A component is (blocks int [mcuy*v, mcux*h, 64] natural order, h, v, tq, td, ta, component_id), mcux / mcuy counted
with the frame's largest factors. A frame of one component is never subsampled (jdinput.c): its blocks are
[ceil(H/8), ceil(W/8), 64] whatever factors its SOF declares.
"""
from __future__ import annotations

import functools
import io
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.jpeg_enc_np import AC_CHR, AC_LUM, DC_CHR, DC_LUM, NATURAL, _BitWriter, _derive  # noqa: E402

JFIF = b"\xff\xe0\x00\x10JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00"
STD = {(0, 0): DC_LUM, (1, 0): AC_LUM, (0, 1): DC_CHR, (1, 1): AC_CHR}
ONE_SYMBOL = ([1] + [0] * 15, [0])  # the symbol 0 (DC difference 0 / EOB) as the 1-bit code "0"


def adobe(transform: int) -> bytes:
    """The Adobe APP14 segment (version 100, flags 0) with the given colour transform byte."""
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


def _grid(width, height, comps):
    """(per-component (h, v) of the MCU walk, mcux, mcuy)."""
    hv = [(c[1], c[2]) for c in comps] if len(comps) > 1 else [(1, 1)]
    maxh, maxv = max(h for h, _ in hv), max(v for _, v in hv)
    return hv, -(-width // (8 * maxh)), -(-height // (8 * maxv)), maxh, maxv


def _scans(comps, scan_order):
    """scan_order → a list of scans, each a list of component indices (None: one scan, frame order)."""
    if scan_order is None:
        return [list(range(len(comps)))]
    if scan_order and isinstance(scan_order[0], (list, tuple)):
        return [list(s) for s in scan_order]
    return [list(scan_order)]


def _block_symbols(b, c, pred):
    """One block as (class, component, symbol, value bits, bit count) events: jchuff.c encode_one_block."""
    diff = int(b[0]) - pred
    t, t2 = (-diff, diff - 1) if diff < 0 else (diff, diff)
    nb = t.bit_length()
    yield 0, c, nb, t2, nb
    r = 0
    for k in range(1, 64):
        x = int(b[NATURAL[k]])
        if x == 0:
            r += 1
            continue
        while r > 15:
            yield 1, c, 0xF0, 0, 0
            r -= 16
        t, t2 = (-x, x - 1) if x < 0 else (x, x)
        nb = t.bit_length()
        yield 1, c, (r << 4) + nb, t2, nb
        r = 0
    if r > 0:
        yield 1, c, 0x00, 0, 0


def _scan_symbols(width, height, comps, scan, restart_interval):
    """The events of one scan in stream order (the MCU walk of oracle.jpeg_enc_np.entropy_bits, plus restarts: a
    (2, n, ...) event before MCU k * restart_interval, predictors reset). A scan of one component is not
    interleaved: one block per MCU over the blocks that hold image data (jdinput.c per_scan_setup)."""
    hv, mcux, mcuy, maxh, maxv = _grid(width, height, comps)
    pred = [0] * len(comps)
    if len(scan) == 1:
        c = scan[0]
        cols, rows = -(-width * hv[c][0] // (8 * maxh)), -(-height * hv[c][1] // (8 * maxv))
        walk = [[(c, y, x)] for y in range(rows) for x in range(cols)]
    else:
        walk = [[(c, my * hv[c][1] + yy, mx * hv[c][0] + xx)
                 for c in scan for yy in range(hv[c][1]) for xx in range(hv[c][0])]
                for my in range(mcuy) for mx in range(mcux)]
    for n, mcu in enumerate(walk):
        if restart_interval and n and n % restart_interval == 0:
            yield 2, (n // restart_interval - 1) % 8, 0, 0, 0
            pred = [0] * len(comps)
        for c, by, bx in mcu:
            b = comps[c][0][by, bx]
            yield from _block_symbols(b, c, pred[c])
            pred[c] = int(b[0])


def write(width, height, comps, qtables, huff, *, restart_interval=0, scan_order=None, app=()) -> bytes:
    """The bytes of a baseline (SOF0) JPEG: SOI, `app` segments, DQT per table (16-bit when a value exceeds 255),
    SOF0, DHT per table, DRI when restart_interval, then one interleaved scan of all components in `scan_order`
    (component indices; default frame order), EOI. scan_order may also be a list of such lists: one scan each, a
    scan of a single component being non-interleaved. qtables: {id: 64 values, natural order}; huff:
    {(class, id): (bits[16], vals)}."""
    nc = len(comps)
    o = bytearray(b"\xff\xd8")
    for seg in app:
        o += seg
    for i, t in qtables.items():
        if max(t) > 255:
            o += b"\xff\xdb\x00\x83" + bytes([0x10 | i]) + b"".join(int(t[NATURAL[k]]).to_bytes(2, "big") for k in range(64))
        else:
            o += b"\xff\xdb\x00\x43" + bytes([i]) + bytes(int(t[NATURAL[k]]) for k in range(64))
    o += b"\xff\xc0" + (8 + 3 * nc).to_bytes(2, "big") + b"\x08" + height.to_bytes(2, "big") + width.to_bytes(2, "big")
    o += bytes([nc])
    for _, h, v, tq, _, _, cid in comps:
        o += bytes([cid, (h << 4) | v, tq])
    for (tc, th), (bits, vals) in huff.items():
        o += b"\xff\xc4" + (3 + 16 + len(vals)).to_bytes(2, "big") + bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)
    if restart_interval:
        o += b"\xff\xdd\x00\x04" + restart_interval.to_bytes(2, "big")
    codes = {k: _derive(t) for k, t in huff.items()}
    for scan in _scans(comps, scan_order):
        o += b"\xff\xda" + (6 + 2 * len(scan)).to_bytes(2, "big") + bytes([len(scan)])
        for c in scan:
            o += bytes([comps[c][6], (comps[c][4] << 4) | comps[c][5]])
        o += b"\x00\x3f\x00"
        w = _BitWriter(True)
        for kind, c, sym, val, nb in _scan_symbols(width, height, comps, scan, restart_interval):
            if kind == 2:  # flush, RSTn; the predictors were reset by the walk
                w.flush()
                w.out += bytes([0xFF, 0xD0 + c])
                continue
            w.put(*codes[(kind, comps[c][4 + kind])][sym])
            if nb:
                w.put(val, nb)
        w.flush()
        o += w.out
    return bytes(o) + b"\xff\xd9"


def scan_bytes(data: bytes) -> bytes:
    """The entropy-coded bytes of a single-scan file: after the SOS header, up to EOI."""
    p = data.index(b"\xff\xda")
    return data[p + 2 + int.from_bytes(data[p + 2:p + 4], "big"):-2]


def gen_optimal_table(freq) -> tuple:
    """jchuff.c jpeg_gen_optimal_table: (bits[16], vals) of a Huffman code for the symbols with a non-zero count,
    no code longer than 16 bits and, through the reserved pseudo-symbol 256, none all ones."""
    freq = [int(f) for f in freq] + [1]
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1 = c2 = -1
        v = 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        v = 1 << 62
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for s in codesize:
        if s:
            assert s <= 32
            bits[s] += 1
    for i in range(32, 16, -1):  # the length limit of the standard's figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1  # the pseudo-symbol's code, the longest one, is never assigned
    vals = [j for n in range(1, 33) for j in range(256) if codesize[j] == n]
    return bits[1:17], vals


def optimal_tables(width, height, comps, *, restart_interval=0, scan_order=None) -> dict:
    """{(class, id): table} for the table ids `comps` name: gen_optimal_table over the symbols the scan emits."""
    hist = {}
    for scan in _scans(comps, scan_order):
        for kind, c, sym, _, _ in _scan_symbols(width, height, comps, scan, restart_interval):
            if kind < 2:
                hist.setdefault((kind, comps[c][4 + kind]), [0] * 256)[sym] += 1
    return {k: gen_optimal_table(f) for k, f in sorted(hist.items())}


def reversed_lengths(table) -> tuple:
    """The same multiset of code lengths with the symbol order reversed: the frequent symbols of an Annex K table
    get its 12-16-bit codes."""
    bits, vals = table
    lens = [ln for ln, n in enumerate(bits, 1) for _ in range(n)]
    pairs = sorted(zip(lens, list(vals)[::-1]))
    return list(bits), [s for _, s in pairs]


def random_blocks(rng, width, height, samp, amp=30, dens=0.3, dc=60) -> list:
    """Sparse random blocks for the sampling list [(h, v)]: AC uniform in [-amp, amp] with probability `dens`,
    DC uniform in [-dc, dc]."""
    hv = samp if len(samp) > 1 else [(1, 1)]
    maxh, maxv = max(h for h, _ in hv), max(v for _, v in hv)
    mcux, mcuy = -(-width // (8 * maxh)), -(-height // (8 * maxv))
    out = []
    for h, v in hv:
        shape = (mcuy * v, mcux * h, 64)
        b = rng.integers(-amp, amp + 1, shape) * (rng.random(shape) < dens)
        b[..., 0] = rng.integers(-dc, dc + 1, shape[:2])
        out.append(b.astype(np.int64))
    return out


def components(blocks, samp, tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1), ids=(1, 2, 3)) -> list:
    return [(blocks[c], samp[c][0], samp[c][1], tq[c], td[c], ta[c], ids[c]) for c in range(len(blocks))]


def expected_coefs(blocks) -> np.ndarray:
    """What decode_coefs must return: the components' blocks in frame order."""
    return np.concatenate([b.reshape(-1, 64) for b in blocks]).astype(np.int16)


class Case:
    """One written file: name, bytes, the blocks it was written from, the colour rule its headers select
    (sp_jpeg_layout.color) and whether the test may demand the GPU entropy path for it (False only for the
    sync-resistant all-zero frame)."""

    def __init__(self, name, data, blocks, color=1, demand_gpu=True):
        self.name, self.data, self.blocks, self.color, self.demand_gpu = name, data, blocks, color, demand_gpu
        self.coefs = expected_coefs(blocks)
        self.coefs.setflags(write=False)

    def __repr__(self):
        return f"Case({self.name!r})"


Q4 = [4] * 64  # flat and small: random sparse blocks of amplitude 30 stay inside the IDCT envelope
Q1 = [1] * 64
S420, S444, S440 = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3, [(1, 2), (1, 1), (1, 1)]

LAYOUTS = (("440", S440), ("y2x2 cb2x1 cr1x2", [(2, 2), (2, 1), (1, 2)]), ("y2x2 cb2x2 cr1x1", [(2, 2), (2, 2), (1, 1)]),
           ("y2x2 cb1x1 cr2x2", [(2, 2), (1, 1), (2, 2)]), ("y4x1 2x1 2x1", [(4, 1), (2, 1), (2, 1)]),
           ("y1x4 1x2 1x2", [(1, 4), (1, 2), (1, 2)]), ("y2x1 cb1x1 cr2x1", [(2, 1), (1, 1), (2, 1)]),
           ("gray 2x2", [(2, 2)]))
SIZES = ((3, 5), (16, 16), (37, 29), (70, 41))  # (width, height)


def _simple(name, rng, W, H, samp, **kw):
    g = random_blocks(rng, W, H, samp)
    n = len(samp)
    comps = components(g, samp, tq=(0, 1, 1)[:n], td=(0, 1, 1)[:n], ta=(0, 1, 1)[:n], ids=(1, 2, 3)[:n])
    q = {0: Q4, 1: Q4} if n == 3 else {0: Q4}
    huff = STD if n == 3 else {(0, 0): DC_LUM, (1, 0): AC_LUM}
    return Case(name, write(W, H, comps, q, huff, app=(JFIF,), **kw), g, color=1 if n == 3 else 0)


@functools.lru_cache(maxsize=None)
def sampling_cases() -> tuple:
    rng = np.random.default_rng(11)
    return tuple(_simple(f"{lab} {W}x{H}", rng, W, H, samp) for lab, samp in LAYOUTS for W, H in SIZES)


@functools.lru_cache(maxsize=None)
def colour_cases() -> tuple:
    rng = np.random.default_rng(12)
    rules = (("adobe 0", (adobe(0),), (1, 2, 3), 2), ("adobe 1", (adobe(1),), (1, 2, 3), 1),
             ("RGB ids", (), (82, 71, 66), 2), ("RGB ids jfif", (JFIF,), (82, 71, 66), 1),
             ("jfif adobe 0", (JFIF, adobe(0)), (1, 2, 3), 1), ("ids 0 1 2", (), (0, 1, 2), 1))
    out = []
    for slab, samp in (("444", S444), ("420", S420), ("440", S440)):
        for W, H in ((53, 37), (3, 5)):
            for lab, app, ids, color in rules:
                g = random_blocks(rng, W, H, samp)
                data = write(W, H, components(g, samp, ids=ids), {0: Q4, 1: Q4}, STD, app=app)
                out.append(Case(f"{lab} {slab} {W}x{H}", data, g, color=color))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def table_cases() -> tuple:
    rng = np.random.default_rng(13)
    W, H, samp = 53, 37, S420
    g = random_blocks(rng, W, H, samp)
    q = {0: Q4, 1: Q4}
    out = []
    dht = {(0, 0): DC_LUM, (1, 0): AC_LUM, (0, 2): DC_CHR, (1, 3): AC_CHR, (0, 3): DC_LUM, (1, 2): AC_LUM}
    out.append(Case("cb, cr on tables 2/3 and 3/2", write(W, H, components(g, samp, td=(0, 2, 3), ta=(0, 3, 2)), q, dht,
                                                          app=(JFIF,)), g))
    out.append(Case("quantisation ids 3 and 2", write(W, H, components(g, samp, tq=(3, 2, 2)), {3: Q4, 2: Q4}, STD,
                                                      app=(JFIF,)), g))
    # 16-bit values on three coefficients, the blocks' values there kept small: a sample is at most about
    # (6 * 300 / 8) + (2 * 256 + 400) / 4 = 453 plus the sparse rest, inside the envelope's [-512, 511]
    q16 = [1] * 64
    q16[0], q16[1], q16[63] = 300, 256, 400
    g16 = [x.copy() for x in g]
    for x in g16:
        x[..., 0], x[..., 1], x[..., 63] = np.clip(x[..., 0], -6, 6), np.clip(x[..., 1], -2, 2), np.clip(x[..., 63], -1, 1)
    out.append(Case("16-bit dqt", write(W, H, components(g16, samp), {0: q16, 1: q16}, STD, app=(JFIF,)), g16))
    comps = components(g, samp)
    out.append(Case("optimal tables", write(W, H, comps, q, optimal_tables(W, H, comps), app=(JFIF,)), g))
    rev = dict(STD)
    rev[(1, 0)], rev[(1, 1)] = reversed_lengths(AC_LUM), reversed_lengths(AC_CHR)
    out.append(Case("reversed AC lengths", write(W, H, comps, q, rev, app=(JFIF,)), g))
    gz = [np.zeros_like(x) for x in g]
    one = {k: ONE_SYMBOL for k in STD}
    out.append(Case("one-symbol 1-bit tables, all-zero frame", write(W, H, components(gz, samp), q, one, app=(JFIF,)),
                    gz, demand_gpu=False))
    return tuple(out)


def _extreme_blocks(rng, W, H, samp):
    g = [np.zeros_like(x) for x in random_blocks(rng, W, H, samp)]
    for x in g:
        x[..., 63] = rng.choice([-3, -2, -1, 1, 2, 3], x.shape[:2])   # 62 zeros: three ZRLs, then 0x0n, no EOB
        x[::2, ::2, 1:] = rng.choice([-2, -1, 1, 2], x[::2, ::2, 1:].shape)  # all 63 AC coefficients non-zero
        x[1::2, 1::2, 63] = 0
        x[1::2, 1::2, 5], x[1::2, 1::2, 7] = 1023, -1023              # category-10 AC
        x[..., 0] = np.where((np.add.outer(np.arange(x.shape[0]), np.arange(x.shape[1]))) % 2 == 0, -1024, 1023)
    return g


@functools.lru_cache(maxsize=None)
def extreme_cases() -> tuple:
    """Quantisation all ones. The +-1023 blocks hold two AC coefficients only and the dense blocks +-2, so every
    block stays inside the envelope while the DC differences reach category 11 (+-2047)."""
    rng = np.random.default_rng(14)
    W, H, samp = 53, 37, S420
    q = {0: Q1, 1: Q1}
    out = []
    g63 = [np.zeros_like(x) for x in random_blocks(rng, W, H, samp)]
    for x in g63:
        x[..., 63] = rng.choice([-3, -2, -1, 1, 2, 3], x.shape[:2])
        x[..., 0] = rng.integers(-60, 61, x.shape[:2])
    out.append(Case("only coefficient 63", write(W, H, components(g63, samp), q, STD, app=(JFIF,)), g63))
    gfull = random_blocks(rng, W, H, samp, amp=0)
    for x in gfull:
        x[..., 1:] = rng.choice([-2, -1, 1, 2], x[..., 1:].shape)
    out.append(Case("all 63 AC non-zero", write(W, H, components(gfull, samp), q, STD, app=(JFIF,)), gfull))
    ge = _extreme_blocks(rng, W, H, samp)
    out.append(Case("AC 1023, DC -1024/1023", write(W, H, components(ge, samp), q, STD, app=(JFIF,)), ge))
    out.append(Case("AC 1023, DC -1024/1023, ri=3", write(W, H, components(ge, samp), q, STD, app=(JFIF,),
                                                          restart_interval=3), ge))
    g = random_blocks(rng, W, H, samp)
    out.append(Case("restart interval above the MCU count", write(W, H, components(g, samp), {0: Q4, 1: Q4}, STD,
                                                                  app=(JFIF,), restart_interval=1000), g))
    s10 = [(2, 2), (2, 2), (2, 1)]
    g10 = random_blocks(rng, W, H, s10)
    out.append(Case("10-block MCU, ri=1", write(W, H, components(g10, s10), {0: Q4, 1: Q4}, STD, app=(JFIF,),
                                                restart_interval=1), g10))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def workgroup_cases() -> tuple:
    """96x80 4:4:4, three AC coefficients in four non-zero, up to +-120: scans of more than two workgroups of
    subsequences (2 * 256 * 256 bits; tests/test_jpeg_streams_host.py asserts it from the packer's count). Not all
    63: a stream of blocks without an EOB gives a decoder that started inside a block nothing to find the block
    grid by, so across workgroups it stays unsynchronised past the round budget and the file falls back to the
    host, by design (at this size: status kStUnsync on the CPU emulation)."""
    rng = np.random.default_rng(15)
    W, H, samp = 96, 80, S444
    g = random_blocks(rng, W, H, samp, amp=0)
    for x in g:
        s = x[..., 1:].shape
        x[..., 1:] = rng.integers(1, 121, s) * rng.choice([-1, 1], s) * (rng.random(s) < 0.75)
    comps = components(g, samp)
    q = {0: Q1, 1: Q1}
    rev = dict(STD)
    rev[(1, 0)], rev[(1, 1)] = reversed_lengths(AC_LUM), reversed_lengths(AC_CHR)
    return (Case("dense 96x80, reversed AC lengths", write(W, H, comps, q, rev, app=(JFIF,)), g),
            Case("dense 96x80, optimal tables", write(W, H, comps, q, optimal_tables(W, H, comps), app=(JFIF,)), g))


@functools.lru_cache(maxsize=None)
def outside_envelope_case() -> Case:
    """16-bit quantisation values that take the dequantised coefficients past +-(2^14 - 1): Pillow's SIMD IDCT and
    the C-semantics one part there, so the file belongs to Pillow."""
    rng = np.random.default_rng(16)
    W, H, samp = 53, 37, S420
    g = random_blocks(rng, W, H, samp)
    q16 = [1000] * 64
    return Case("16-bit dqt outside the envelope", write(W, H, components(g, samp), {0: q16, 1: Q4}, STD, app=(JFIF,)), g)


SCAN_ORDERS = ([2, 0, 1], [1, 2, 0], [0, 2, 1], [1, 0, 2], [2, 1, 0])


@functools.lru_cache(maxsize=None)
def refused_cases() -> tuple:
    """(name, bytes) of files Pillow refuses (libjpeg errors), so the parser must too: interleaved MCUs of more than
    D_MAX_BLOCKS_IN_MCU = 10 blocks, scans that name the frame's components out of order (jdmarker.c get_sos takes
    the i-th scan component only from frame positions i and up), a Huffman table whose code is all ones."""
    rng = np.random.default_rng(17)
    W, H = 53, 37
    q = {0: Q4, 1: Q4}
    out = []
    for lab, samp in (("y4x2 2x1 2x1", [(4, 2), (2, 1), (2, 1)]), ("three at 2x2", [(2, 2)] * 3)):
        g = random_blocks(rng, W, H, samp)
        out.append((f"12-block MCU {lab}", write(W, H, components(g, samp), q, STD, app=(JFIF,))))
    for slab, samp in (("420", S420), ("444", S444)):
        g = random_blocks(rng, W, H, samp)
        for order in SCAN_ORDERS:
            out.append((f"scan order {order} {slab}", write(W, H, components(g, samp), q, STD, app=(JFIF,),
                                                            scan_order=order)))
        # two scans, the first out of order: components 2 and 0 interleaved, then component 1 alone
        out.append((f"scans [2, 0] then [1] {slab}", write(W, H, components(g, samp), q, STD, app=(JFIF,),
                                                          scan_order=[[2, 0], [1]])))
    gz = [np.zeros_like(x) for x in random_blocks(rng, W, H, S420)]
    two = {k: ([2] + [0] * 15, [0, 1]) for k in STD}
    out.append(("two 1-bit codes", write(W, H, components(gz, S420), q, two, app=(JFIF,))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def subset_scan_cases() -> tuple:
    """Multi-scan sequential files Pillow decodes (each scan names its components in frame order), so the parser
    must go on taking them: Case entries, for the host decoder only (more than one scan is not GPU-eligible). A
    component scanned alone has only its blocks with image data coded, so the others are written as zeros."""
    rng = np.random.default_rng(18)
    W, H = 53, 37
    out = []
    for slab, samp in (("420", S420), ("444", S444)):
        g = random_blocks(rng, W, H, samp)
        for c, (h, v) in enumerate(samp):
            g[c][-(-H * v // (8 * samp[0][1])):] = 0
            g[c][:, -(-W * h // (8 * samp[0][0])):] = 0
        for scans in ([[0, 1], [2]], [[1, 2], [0]], [[0, 2], [1]], [[2], [0, 1]], [[2], [1], [0]], [[2, 1], [0]]):
            out.append(Case(f"scans {scans} {slab}", write(W, H, components(g, samp), {0: Q4, 1: Q4}, STD, app=(JFIF,),
                                                           scan_order=scans), g))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def luma_4x1_chroma_1x1() -> bytes:
    """Chroma four times below luma: Pillow decodes it, the parser declines it by design (ratio above 2)."""
    rng = np.random.default_rng(19)
    samp = [(4, 1), (1, 1), (1, 1)]
    g = random_blocks(rng, 53, 37, samp)
    return write(53, 37, components(g, samp), {0: Q4, 1: Q4}, STD, app=(JFIF,))


def all_cases() -> tuple:
    return sampling_cases() + colour_cases() + table_cases() + extreme_cases() + workgroup_cases()


def pillow_pixels(data: bytes) -> np.ndarray:
    """Pillow's convert("RGB") of the file, warnings turned into errors."""
    import warnings

    from PIL import Image

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(data))
        im.load()
        return np.asarray(im.convert("RGB"))
