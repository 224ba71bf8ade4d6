"""GPU: the cross-process batcher's native half and one end-to-end run.

sp_copy_segments against an exact host copy (int32 views, so NaN payloads and -0.0 count) over the lengths,
alignments and segment counts at which its vector / scalar split and its block-to-segment table can go wrong,
between device memory and registered host memory in both directions; sp_host_register / sp_host_unregister on
anonymous page-aligned memory and on a POSIX shared-memory block; then three client processes and one owner
process with a real R18vd engine."""
import ctypes as C
import json
import mmap
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_model import BOX_TOL_PX, SCORE_TOL  # noqa: E402

GUARD = 0x5A5A5A5A
ELEMS = [4099, 0, 1, 3, 4, 5, 63, 64, 65, 4096, 8195]  # 4096 = one workgroup's share: exactly one, one + 3, two + 3
OFFSETS = [0, 4, 8, 12]  # bytes from 16-byte alignment


def _cases():
    """Every (elems, src offset, dst offset); the launch sizes below cut this list into n = 1, 2, the maximum, rest."""
    return [(e, so, do) for e in ELEMS for so in OFFSETS for do in OFFSETS]


def _plan(cases):
    """Element positions of every case's source and destination in two flat int32 buffers: each on its own 16-byte
    aligned base plus its offset, at least four guard words between neighbours."""
    src_pos, dst_pos, s, d = [], [], 8, 8
    for e, so, do in cases:
        src_pos.append(s + so // 4)
        dst_pos.append(d + do // 4)
        s += (e + so // 4 + 4 + 3) // 4 * 4 + 4
        d += (e + do // 4 + 4 + 3) // 4 * 4 + 4
    return src_pos, dst_pos, s + 8, d + 8


def _bits(n, seed):
    """Random 32-bit patterns with quiet and signalling NaNs of several payloads, infinities and -0.0 sown in."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    special = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001],
                       dtype=np.uint32).view(np.int32)
    a[rng.integers(0, n, size=n // 5)] = special[rng.integers(0, len(special), size=n // 5)]
    return a


class HostBuf:
    """Anonymous page-aligned host memory, registered for the device."""

    def __init__(self, n_words):
        from spotter_amd import ops

        self.mm = mmap.mmap(-1, (4 * n_words + 4095) // 4096 * 4096)
        self.np = np.frombuffer(self.mm, dtype=np.int32, count=n_words)
        self.addr = self.np.ctypes.data
        self.dev = ops.host_register(self.addr, len(self.mm))

    def close(self):
        from spotter_amd import ops

        ops.host_unregister(self.addr)
        self.np = None
        self.mm.close()


@pytest.mark.parametrize("kind", ["device to device", "registered host to device", "device to registered host"])
def test_copy_segments_is_bit_exact(kind):
    from spotter_amd import _lib, ops

    cases = _cases()
    src_pos, dst_pos, n_src, n_dst = _plan(cases)
    src_np = _bits(n_src, 5)
    exp = np.full(n_dst, GUARD, dtype=np.uint32).view(np.int32)
    for (e, _, _), s, d in zip(cases, src_pos, dst_pos):
        assert s + e <= n_src and d + e <= n_dst
        exp[d:d + e] = src_np[s:s + e]
    bufs = []
    try:
        if kind.startswith("registered host"):
            hs = HostBuf(n_src)
            bufs.append(hs)
            hs.np[:] = src_np
            src_ptr = hs.dev
        else:
            src_t = torch.from_numpy(src_np).cuda()
            src_ptr = src_t.data_ptr()
        if kind.endswith("registered host"):
            hd = HostBuf(n_dst)
            bufs.append(hd)
            hd.np[:] = np.int32(GUARD)
            dst_ptr, read = hd.dev, lambda: hd.np.copy()
        else:
            dst_t = torch.full((n_dst,), GUARD, dtype=torch.int32, device="cuda")
            dst_ptr, read = dst_t.data_ptr(), lambda: dst_t.cpu().numpy()
        assert src_ptr % 16 == 0 and dst_ptr % 16 == 0
        segs = [(src_ptr + 4 * s, dst_ptr + 4 * d, e) for (e, _, _), s, d in zip(cases, src_pos, dst_pos)]
        # n = 1, n = 2, the maximum (mixed lengths and alignments in one launch), then the rest
        i, sizes = 0, [1, 2] + [_lib.SP_COPY_MAX_SEGMENTS] * len(segs)
        launches = []
        for n in sizes:
            if i >= len(segs):
                break
            launches.append(segs[i:i + n])
            i += n
        assert [len(l) for l in launches[:3]] == [1, 2, 64] and sum(len(l) for l in launches) == len(segs)
        torch.cuda.synchronize()
        for l in launches:
            ops.copy_segments(l)
        torch.cuda.synchronize()
        got = read()
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f"{bad.size} words differ, first at {bad[:8]}"
    finally:
        torch.cuda.synchronize()
        for b in bufs:
            b.close()


def test_copy_segments_n1_and_n2_with_differently_misaligned_ends():
    """n = 1 and n = 2 again, with source and destination at different offsets, so every word moves singly."""
    from spotter_amd import ops

    src = torch.from_numpy(_bits(3 * 5000, 9)).cuda()
    for n in (1, 2):
        dst = torch.full((3 * 5000,), GUARD, dtype=torch.int32, device="cuda")
        exp = np.full(3 * 5000, GUARD, dtype=np.uint32).view(np.int32)
        segs = []
        for k in range(n):
            s, d, e = 5000 * k + 1, 5000 * k + 3 - 2 * k, 4099 + k
            segs.append((src.data_ptr() + 4 * s, dst.data_ptr() + 4 * d, e))
            exp[d:d + e] = src.cpu().numpy()[s:s + e]
        ops.copy_segments(segs)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), exp)


def test_refused_descriptors_return_minus_one_and_change_nothing():
    from spotter_amd import _lib, ops

    L = _lib.lib()
    src = torch.from_numpy(_bits(256, 3)).cuda()
    dst = torch.full((256,), GUARD, dtype=torch.int32, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()
    st = torch.cuda.current_stream().cuda_stream

    def desc(n, segs):
        x = _lib.SpCopySegmentsDesc(n=n)
        for i, (a, b, e) in enumerate(segs):
            x.seg[i].src, x.seg[i].dst, x.seg[i].elems = a, b, e
        return C.byref(x)

    good = (s, d, 64)
    refused = [
        (None, "null descriptor"),
        (desc(0, [good]), "n 0 outside [1, 64]"),
        (desc(65, [good]), "n 65 outside [1, 64]"),
        (desc(2, [good, (s, d + 512, -1)]), "elems -1 < 0"),
        (desc(2, [good, (None, d + 512, 8)]), "null pointer"),
        (desc(2, [good, (s, None, 8)]), "null pointer"),
        (desc(2, [good, (s + 2, d + 512, 8)]), "4-byte aligned"),
    ]
    for dsc, text in refused:
        assert L.sp_copy_segments(dsc, st) == -1
        assert text in L.sp_last_error().decode(), (text, L.sp_last_error())
    torch.cuda.synchronize()
    assert (dst.cpu().numpy().view(np.uint32) == GUARD).all()  # not even the good first segment of a refused call
    ops.copy_segments([(s, d, 0), (None, None, 0), (s, d + 64, 4)])  # empty segments are legal and skipped
    torch.cuda.synchronize()
    got = dst.cpu().numpy()
    assert np.array_equal(got[16:20], src.cpu().numpy()[:4]) and (got[:16].view(np.uint32) == GUARD).all()


def test_host_register_refusals_and_reregistration():
    from spotter_amd import _lib, ops

    L = _lib.lib()
    err = lambda: L.sp_last_error().decode()
    mm = mmap.mmap(-1, 4 * 4096)
    arr = np.frombuffer(mm, dtype=np.int32)
    addr = arr.ctypes.data
    dev = C.c_void_p()
    try:
        assert L.sp_host_register(None, 4096, C.byref(dev)) != 0 and "null pointer" in err()
        assert L.sp_host_register(addr, 0, C.byref(dev)) != 0 and "<= 0" in err()
        assert L.sp_host_register(addr, -8, C.byref(dev)) != 0 and "<= 0" in err()
        assert L.sp_host_register(addr + 64, 4096, C.byref(dev)) != 0 and "not aligned" in err()
        assert L.sp_host_unregister(addr) != 0 and "not registered" in err()
        src = torch.from_numpy(_bits(1024, 4)).cuda()
        for round_ in range(2):  # register, use, unregister; then the same again
            arr[:] = 0
            d = ops.host_register(addr, len(mm))
            assert L.sp_host_register(addr, len(mm), C.byref(dev)) != 0 and "overlaps" in err()  # double register
            assert L.sp_host_register(addr + 4096, 4096, C.byref(dev)) != 0 and "overlaps" in err()
            ops.copy_segments([(src.data_ptr(), d + 4 * 7, 1000)])
            torch.cuda.synchronize()
            assert np.array_equal(arr[7:1007], src.cpu().numpy()[:1000]) and not arr[:7].any() and not arr[1007:].any()
            ops.host_unregister(addr)
            assert L.sp_host_unregister(addr) != 0 and "not registered" in err()
    finally:
        arr = None
        mm.close()


def test_posix_shared_memory_registers_and_is_seen_by_both_mappings():
    """What the batcher does: a multiprocessing.shared_memory block, registered, written by the copy kernel through
    one mapping and read through a second mapping of the same name."""
    from multiprocessing import shared_memory

    from spotter_amd import ops
    shm = shared_memory.SharedMemory(create=True, size=8 * 4096)
    other = shared_memory.SharedMemory(name=shm.name)
    a = np.frombuffer(shm.buf, dtype=np.int32)
    b = np.frombuffer(other.buf, dtype=np.int32)
    try:
        a[:] = 0
        src = torch.from_numpy(_bits(4099, 6)).cuda()
        back = torch.zeros(4099, dtype=torch.int32, device="cuda")
        d = ops.host_register(a.ctypes.data, shm.size)
        try:
            ops.copy_segments([(src.data_ptr(), d + 4 * 5, 4099)])
            torch.cuda.synchronize()
            assert np.array_equal(b[5:5 + 4099], src.cpu().numpy()) and not b[:5].any()
            ops.copy_segments([(d + 4 * 5, back.data_ptr(), 4099)])
            torch.cuda.synchronize()
            assert torch.equal(back, src)
        finally:
            ops.host_unregister(a.ctypes.data)
    finally:
        a = b = None
        other.close()
        shm.close()
        shm.unlink()


# One client process: two images through the processor and the model with batching="shared"; saves the sigmoid
# scores and the post-processed detections (threshold 0: every one of the top 300).
CHILD = r"""
import json, os, sys
a = json.loads(sys.argv[1])
sys.path.insert(0, a["root"])
import numpy as np, torch
from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
from spotter_amd.synthetic import synthetic_image
m = SpotterForObjectDetection.from_pretrained("synthetic:r18vd", batching="shared")
m._shared_opts = dict(timeout_s=60.0)
proc = SpotterImageProcessor()
xs = [proc(images=synthetic_image(s)) for s in a["seeds"]]
m._shared_client().connect(3 * 640 * 640, on_gpu=True)
print("READY", flush=True)
sys.stdin.readline()
res = {}
for i, x in enumerate(xs):
    with torch.no_grad():
        out = m(**x)
    det = proc.post_process_object_detection(out, target_sizes=torch.tensor([[640, 640]]), threshold=0.0)[0]
    res[f"sig{i}"] = torch.sigmoid(out.logits[0]).cpu().numpy()
    for k in ("scores", "labels", "boxes"):
        res[f"{k}{i}"] = det[k].numpy()
assert m._engine is None and m._batcher is None
m._shared.close()
np.savez(a["out"], **res)
print("DONE engine_is_none", flush=True)
"""


def _match(got, ref):
    """Every post-processed detection has a partner of its own: same label, score within SCORE_TOL, box within
    BOX_TOL_PX. One within SCORE_TOL of the other side's lowest kept score may lack one (the top-300 cut)."""
    used = set()
    for side_a, side_b in ((ref, got), (got, ref)):
        cut = side_b["scores"].min()
        used.clear()
        for s, l, b in zip(side_a["scores"], side_a["labels"], side_a["boxes"]):
            cand = [j for j in np.flatnonzero((side_b["labels"] == l) & (np.abs(side_b["scores"] - s) <= SCORE_TOL))
                    if j not in used and np.abs(side_b["boxes"][j] - b).max() <= BOX_TOL_PX]
            if cand:
                used.add(min(cand, key=lambda j: np.abs(side_b["boxes"][j] - b).max()))
            else:
                assert s <= cut + SCORE_TOL, f"no partner for label {l} score {s:.5f} box {b}"


def test_three_client_processes_share_one_owner_engine(tmp_path):
    from multiprocessing.connection import Client

    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.config import PRESETS
    from spotter_amd.synthetic import synthetic_image

    sockdir = __import__("tempfile").mkdtemp(prefix="spb")
    sock = os.path.join(sockdir, "o.sock")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env["SPOTTER_BATCH_SOCKET"] = sock
    env.pop("SPOTTER_BATCHING", None)
    seeds = [[400 + 2 * i, 401 + 2 * i] for i in range(3)]
    procs, timers = [], []

    def start(cmd, limit, **kw):
        p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT, **kw)
        t = threading.Timer(limit, p.kill)  # every child has its own time limit
        t.start()
        procs.append(p)
        timers.append(t)
        return p

    def line(p, want, who):
        got = p.stdout.readline()
        assert got.startswith(want), f"{who} ended before {want} (rc {p.poll()}): nothing further is started"
        return got

    try:
        owner = start([sys.executable, "-m", "spotter_amd.shared_batch", "--device", "0", "--socket", sock, "--model",
                       "synthetic:r18vd", "--precision", "fp32", "--max-wait-ms", "50", "--idle-exit-s", "60"],
                      150, stdin=subprocess.DEVNULL)
        assert line(owner, "READY", "the owner").split()[1] == str(owner.pid)
        kids = []
        for i in range(3):
            arg = json.dumps({"root": ROOT, "seeds": seeds[i], "out": str(tmp_path / f"c{i}.npz")})
            kids.append(start([sys.executable, "-c", CHILD, arg], 150, stdin=subprocess.PIPE))
        # the bs1 references, in this process, while the clients start (test_request_microbatching_matches_single_calls)
        ref_model = SpotterForObjectDetection(PRESETS["r18vd"], use_graphs=False)
        proc = SpotterImageProcessor()
        ref = {}
        for s in sum(seeds, []):
            with torch.no_grad():
                out = ref_model(**proc(images=synthetic_image(s)))
            det = proc.post_process_object_detection(out, target_sizes=torch.tensor([[640, 640]]), threshold=0.0)[0]
            ref[s] = (torch.sigmoid(out.logits[0]).cpu().numpy(), {k: det[k].numpy() for k in det})
        for i, k in enumerate(kids):
            line(k, "READY", f"client {i}")
        for k in kids:  # released together
            k.stdin.write("go\n")
            k.stdin.flush()
        for i, k in enumerate(kids):
            out, _ = k.communicate(timeout=150)
            assert k.returncode == 0 and "DONE engine_is_none" in out, f"client {i} failed (rc {k.returncode})"
        with Client(sock, family="AF_UNIX") as c:
            c.send(("stats",))
            assert c.poll(30)
            st = c.recv()[1]
    finally:
        for t in timers:
            t.cancel()
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait(timeout=30)
            p.stdout.close()
        __import__("shutil").rmtree(sockdir, ignore_errors=True)
    assert st["images"] == 6 and st["batches"] < st["images"], st
    for i in range(3):
        z = np.load(tmp_path / f"c{i}.npz")
        for j, s in enumerate(seeds[i]):
            sig, det = ref[s]
            np.testing.assert_allclose(np.sort(z[f"sig{j}"].max(-1)), np.sort(sig.max(-1)), rtol=0, atol=SCORE_TOL)
            _match({k: z[f"{k}{j}"] for k in ("scores", "labels", "boxes")}, det)
