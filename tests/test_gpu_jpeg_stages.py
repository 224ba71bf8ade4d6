"""GPU: the JPEG decode kernels of csrc/jpeg.hip stage by stage (jpeg_idct_kernel, jpeg_color_kernel and their batch
forms), over the case lists of tests/jpeg_idct_cases.py. Every comparison is bit for bit; no tolerance appears.

Stage 1, the IDCT: sp_jpeg_to_rgb and sp_jpeg_batch_to_rgb write the component planes into a caller-owned `work`
buffer, which is read back after the call and compared with oracle.jpeg_np.planes, MCU-padding blocks and blocks
outside the envelope included (the kernel's & 1023 wrap is the oracle's), between guard bytes. The per-image status
word must be exactly the block's label: 1 for a block that trips any of the four envelope conditions, among them
blocks whose largest pass-2 value is 512 or smallest -513 and nothing else, 0 for blocks at 511 and -512, also beside
flagged neighbours in one launch.

Stage 2, upsampling and colour: with the planes pinned, the pixels of the edge grid (every first / last row and
column rule, the box replication, dh == 1, all four rounding biases under full-range noise) and of the colour-domain
frames (every (Cb, Cr), (Y, Cb), (Y, Cr) pair) against oracle.jpeg_np.to_rgb, through JpegDecoder.decode (one thread
per pixel), decode_many (4-pixel groups, packed dword stores) and direct batch calls with rgb_stride = 3 W + 5 (the
bytewise path, groups that wrap rows).

tests/test_jpeg_idct_cases.py asserts on the CPU what makes these demands fair: the labels, Pillow's agreement with
the oracle on every case that is not flagged, and that no frame case is outside the envelope."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(__file__))
import jpeg_idct_cases as jc  # noqa: E402

from spotter_amd._lib import SP_JPEG_BATCH_MAX, SpJpegBatchItem, SpJpegBatchTotals, SpJpegLayout, lib  # noqa: E402

WORK_FILL, RGB_FILL, GUARD = 0x5A, 0xA5, 256


@pytest.fixture(scope="module")
def dev():
    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    return torch.device("cuda", 0)


_REF = {}


def _ref(case):
    """(layout, coefficients, oracle planes, oracle pixels) of a case: computed once, read by every test."""
    if case.name not in _REF:
        from oracle.jpeg_np import planes, to_rgb

        from spotter_amd.jpeg import decode_coefs, layout_dict

        lay, co = decode_coefs(case.data)
        assert np.array_equal(co, case.coefs), case.name
        L = layout_dict(lay)
        pl, px = planes(co, L), to_rgb(co, L)
        for a in pl + [px]:
            a.setflags(write=False)
        _REF[case.name] = (lay, co, pl, px)
    return _REF[case.name]


def _first(bad):
    return bad[:3].tolist()


def _same(got, want, name):
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    assert g.shape == want.shape and g.dtype == np.uint8, (name, g.shape, want.shape)
    bad = np.argwhere(g != want)
    assert bad.size == 0, (f"{name}: {len(bad)} samples differ, first at (y, x, channel) {_first(bad)}: "
                           f"{[int(g[tuple(b)]) for b in bad[:3]]} for {[int(want[tuple(b)]) for b in bad[:3]]}")


def _check_planes(work, base, lay, planes, name, rest):
    """The component planes of one image inside the host copy of `work`, at byte `base`: each equal to the oracle's,
    whole block grid. Clears their bytes in the mask `rest`."""
    for c in range(lay.ncomp):
        h, w = lay.bh[c] * 8, lay.bw[c] * 8
        a = base + lay.plane_off[c]
        got = work[a:a + h * w].reshape(h, w)
        bad = np.argwhere(got != planes[c])
        assert bad.size == 0, (f"{name}: component {c}: {len(bad)} IDCT samples differ, first at (row, column) "
                               f"{_first(bad)} (block {bad[0][0] // 8 * lay.bw[c] + bad[0][1] // 8} of the component): "
                               f"{int(got[tuple(bad[0])])} for {int(planes[c][tuple(bad[0])])}")
        rest[a:a + h * w] = False


def _check_rows(rgb, off, stride, px, name, rest):
    H, W = px.shape[:2]
    for y in range(H):
        a = off + y * stride
        row = rgb[a:a + 3 * W]
        if not np.array_equal(row, px[y].reshape(-1)):
            _same(row.reshape(W, 3)[None], px[y][None], f"{name} row {y}")
        rest[a:a + 3 * W] = False


def _batch_call(dev, cases, pad=0):
    """One sp_jpeg_batch_to_rgb over `cases` (at most 64) with a table built here: gaps between the plane sets and
    between the images, rows of 3 W + pad bytes, both arenas pre-filled. Checks the planes, the pixels of the cases
    that are inside the envelope (of all, where the oracle's C semantics are pinned: gray blocks) and that nothing else
    was written; returns the status words."""
    n = len(cases)
    assert 1 <= n <= SP_JPEG_BATCH_MAX
    refs = [_ref(c) for c in cases]
    items, tot = (SpJpegBatchItem * n)(), SpJpegBatchTotals()
    assert lib().sp_jpeg_batch_plan((SpJpegLayout * n)(*[r[0] for r in refs]), n, items, C.byref(tot)) == 0, \
        lib().sp_last_error()
    rgb_off = work_off = GUARD
    for k, it in enumerate(items):
        assert bytes(it.lay.quant) == bytes(refs[k][0].quant)
        it.rgb_stride = 3 * it.lay.width + pad
        it.rgb_off, it.work_off = rgb_off, work_off
        rgb_off += (it.rgb_stride * it.lay.height + 3 + 36) & ~3  # (4-byte aligned, a gap of at least 36 bytes)
        work_off += ((it.lay.plane_bytes + 15) & ~15) + 48
    rgb = torch.full((rgb_off + GUARD,), RGB_FILL, dtype=torch.uint8, device=dev)
    work = torch.full((work_off + GUARD,), WORK_FILL, dtype=torch.uint8, device=dev)
    status = torch.zeros(n + 2, dtype=torch.int32, device=dev)
    status[0] = status[n + 1] = 0x7E7E7E7E
    coefs = torch.from_numpy(np.concatenate([r[1].reshape(-1) for r in refs])).to(dev)
    table = torch.from_numpy(np.frombuffer(bytes(items), dtype=np.uint8).copy()).to(dev)
    rc = lib().sp_jpeg_batch_to_rgb(coefs.data_ptr(), coefs.numel(), table.data_ptr(), items, n, C.byref(tot),
                                    work.data_ptr(), work.numel(), rgb.data_ptr(), rgb.numel(),
                                    status.data_ptr() + 4, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert st[0] == st[n + 1] == 0x7E7E7E7E
    got, pl = rgb.cpu().numpy(), work.cpu().numpy()
    rest, wrest = np.ones(got.size, bool), np.ones(pl.size, bool)
    for it, c, (lay, _, planes, px) in zip(items, cases, refs):
        _check_planes(pl, it.work_off, lay, planes, c.name, wrest)
        _check_rows(got, it.rgb_off, it.rgb_stride, px, c.name, rest)
    assert (got[rest] == RGB_FILL).all(), "bytes outside the images' rows were written"
    assert (pl[wrest] == WORK_FILL).all(), "bytes of work outside the planes were written"
    return st[1:n + 1]


def _single_calls(dev, cases):
    """sp_jpeg_to_rgb for each case, each with its own slots of one work arena, one RGB arena and one status array
    (guards between the slots), all launched before one synchronisation. Checks as _batch_call; returns the status
    words."""
    refs = [_ref(c) for c in cases]
    slots, rgb_off, work_off = [], GUARD, GUARD
    for lay, _, _, px in refs:
        slots.append((rgb_off, work_off))
        rgb_off += (px.size + 255 + GUARD) & ~255
        work_off += ((lay.plane_bytes + 15) & ~15) + 48
    rgb = torch.full((rgb_off + GUARD,), RGB_FILL, dtype=torch.uint8, device=dev)
    work = torch.full((work_off + GUARD,), WORK_FILL, dtype=torch.uint8, device=dev)
    status = torch.full((2 * len(cases) + 1,), 0x7E7E7E7E, dtype=torch.int32, device=dev)
    status[1::2] = 0
    stream = torch.cuda.current_stream().cuda_stream
    keep = []
    for k, ((lay, co, _, _), (ro, wo)) in enumerate(zip(refs, slots)):
        coefs = torch.from_numpy(co.reshape(-1)).to(dev)
        keep.append(coefs)
        rc = lib().sp_jpeg_to_rgb(coefs.data_ptr(), C.byref(lay), work.data_ptr() + wo, lay.plane_bytes,
                                  rgb.data_ptr() + ro, 3 * lay.width, status.data_ptr() + 4 * (2 * k + 1), stream)
        assert rc == 0, lib().sp_last_error()
    torch.cuda.synchronize()
    st = status.cpu().tolist()
    assert all(x == 0x7E7E7E7E for x in st[0::2])
    got, pl = rgb.cpu().numpy(), work.cpu().numpy()
    rest, wrest = np.ones(got.size, bool), np.ones(pl.size, bool)
    for c, (lay, _, planes, px), (ro, wo) in zip(cases, refs, slots):
        _check_planes(pl, wo, lay, planes, c.name, wrest)
        _check_rows(got, ro, 3 * lay.width, px, c.name, rest)
    assert (got[rest] == RGB_FILL).all(), "bytes outside the images' rows were written"
    assert (pl[wrest] == WORK_FILL).all(), "bytes of work outside the planes were written"
    return st[1::2]


def _chunks(cases):
    return [cases[i:i + SP_JPEG_BATCH_MAX] for i in range(0, len(cases), SP_JPEG_BATCH_MAX)]


def _assert_status(got, blocks, form):
    wrong = [(b.name, s, dict(zip(jc.CONDITIONS, b.label)), {"pass 2": (int(b.lo), int(b.hi)), "pass 1": int(b.p1)})
             for b, s in zip(blocks, got) if s != int(b.flagged)]
    assert not wrong, f"{form}: {len(wrong)} status words differ from the label, first (name, status, label): {wrong[:3]}"


# ------------------------------------------------------------------------------------------------ stage 1
def test_batch_status_is_the_label_of_each_block(dev):
    """The envelope blocks as 64 one-block images per launch, flagged ones spread among inside ones: status[i] is 1
    exactly for the flagged blocks (blocks at 512 and at -513 alone among them), 0 for the blocks at 511 and -512
    and for every inside block beside a flagged neighbour; the IDCT plane of every block, flagged or not, is the
    oracle's."""
    order = jc.interleaved(jc.envelope_blocks())
    for chunk in _chunks(order):
        _assert_status(_batch_call(dev, chunk), chunk, "sp_jpeg_batch_to_rgb")


def _single_subset():
    by = {}
    for b in jc.envelope_blocks():
        by.setdefault(b.cls, []).append(b)
    return [b for cls, bs in by.items() for b in bs[:12 if cls == "inside" else 6]]


def test_single_image_status_is_the_label_of_each_block(dev):
    """The single-image kernel on six blocks of every class (all of the DC-only and 16-bit-table ones)."""
    blocks = _single_subset()
    assert {b.cls for b in blocks} == {b.cls for b in jc.envelope_blocks()}
    _assert_status(_single_calls(dev, blocks), blocks, "sp_jpeg_to_rgb")


def test_three_table_planes_batch(dev):
    """Y, Cb and Cr dequantised each by its own table, component boundaries inside a workgroup of 32 blocks, a last
    partial workgroup, a frame of 6 blocks: every plane is the oracle's, padding blocks included."""
    frames = list(jc.three_table_frames())
    assert _batch_call(dev, frames) == [0] * len(frames)
    assert _batch_call(dev, frames[::-1], pad=5) == [0] * len(frames)


def test_three_table_planes_single(dev):
    frames = list(jc.three_table_frames())
    assert _single_calls(dev, frames) == [0] * len(frames)


def test_three_table_frames_through_gpu_entropy(dev):
    """The quantisation tables as the scan packer latches them: JpegDecoder(entropy="gpu"), one file at a time and as
    one chunk; the GPU chain decodes every frame, and decode() leaves the oracle's planes in the decoder's work."""
    from spotter_amd.jpeg import JpegDecoder

    frames = jc.three_table_frames()
    d = JpegDecoder(dev, entropy="gpu")
    for c in frames:
        lay, _, planes, px = _ref(c)
        _same(d.decode(c.data), px, c.name + " (decode, gpu entropy)")
        work = d._g["work"][:lay.plane_bytes].cpu().numpy()
        _check_planes(work, 0, lay, planes, c.name + " (decode, gpu entropy)", np.ones(work.size, bool))
    assert d.stats["gpu"] == len(frames) and not d.stats["fallback"] and d.stats["host"] == 0, d.stats
    got = d.decode_many([c.data for c in frames])
    for g, c in zip(got, frames):
        assert torch.is_tensor(g), (c.name, g)
        _same(g, _ref(c)[3], c.name + " (decode_many, gpu entropy)")
    assert d.batch_stats["gpu"] == len(frames) and not d.batch_stats["fallback"], d.batch_stats


# ------------------------------------------------------------------------------------------------ stage 2
def _decode_and_decode_many(dev, cases):
    from spotter_amd.jpeg import JpegDecoder

    d = JpegDecoder(dev)
    for c in cases:
        _same(d.decode(c.data), _ref(c)[3], c.name + " (decode)")
    got = d.decode_many([c.data for c in cases])
    assert len(got) == len(cases) and d.batch_stats["chunks"] == -(-len(cases) // SP_JPEG_BATCH_MAX)
    for g, c in zip(got, cases):
        assert torch.is_tensor(g), (c.name, g)
        _same(g, _ref(c)[3], c.name + " (decode_many)")


@pytest.mark.parametrize("layout", [lab for lab, _ in jc.EDGE_LAYOUTS])
def test_edge_grid_pixels(dev, layout):
    """81 sizes of one sampling layout through the single-image kernels and the batch kernels (64 per launch chain,
    packed rows: the dword stores, 4-pixel groups that span up to four rows at W = 1)."""
    _decode_and_decode_many(dev, [c for c in jc.edge_grid() if c.layout == layout])


@pytest.mark.parametrize("layout", [lab for lab, _ in jc.EDGE_LAYOUTS])
def test_edge_grid_pixels_strided_rows(dev, layout):
    """The same through direct batch calls with rgb_stride = 3 W + 5: the bytewise path, a row wrap inside a 4-pixel
    group, the 5 bytes after every row and the gaps between images untouched."""
    for chunk in _chunks([c for c in jc.edge_grid() if c.layout == layout]):
        assert _batch_call(dev, chunk, pad=5) == [0] * len(chunk)


def test_colour_domain(dev):
    """Every (Cb, Cr) pair under noise luma, every (Y, Cb) and (Y, Cr) pair under noise in the third: the colour
    constants over their whole domain, both clamps, by all three store paths."""
    frames = list(jc.colour_frames())
    _decode_and_decode_many(dev, frames)
    assert _batch_call(dev, frames, pad=5) == [0, 0, 0]
