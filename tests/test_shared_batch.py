"""CPU: batching across replica processes (spotter_amd/shared_batch.py) with a stub owner, whose forward is a
numpy function of each image (stub_forward) and whose gather / scatter are numpy copies: the protocol, the collector
rule, start-up under the lock, and what happens when either side dies. Also the argument checks of the new C-ABI
entry points, which refuse before any device call. Every child process runs under a timeout."""
import ctypes as C
import json
import os
import pickle
import shutil
import signal
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
H = W = 8


def image(client: int, call: int) -> np.ndarray:
    """A distinct [1, 3, H, W] image per (client, call): means 0.1 apart, so no two share their stub rows."""
    rng = np.random.default_rng(1000 * client + call)
    return (rng.uniform(0, 0.01, (1, 3, H, W)) + 0.1 * (10 * client + call)).astype(np.float32)


def expected(img: np.ndarray):
    from spotter_amd.shared_batch import stub_forward

    return stub_forward(img, 300, 80)


def check_rows(out, img):
    lg, bx = expected(img)
    np.testing.assert_allclose(out.logits.numpy(), lg, rtol=0, atol=1e-6)
    np.testing.assert_allclose(out.pred_boxes.numpy(), bx, rtol=0, atol=1e-6)


@pytest.fixture
def sockdir():
    d = tempfile.mkdtemp(prefix="spb")  # short: an AF_UNIX path holds ~100 bytes
    yield d
    shutil.rmtree(d, ignore_errors=True)


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    env.pop("SPOTTER_BATCHING", None)
    return env


class OwnerProc:
    def __init__(self, sock, *extra):
        self.sock = sock
        self.p = subprocess.Popen([sys.executable, "-m", "spotter_amd.shared_batch", "--stub", "--socket", sock,
                                   "--model", "synthetic:r18vd", "--precision", "fp32", *extra],
                                  stdout=subprocess.PIPE, stdin=subprocess.DEVNULL, text=True, env=_env(), cwd=ROOT)
        self.ready = self.p.stdout.readline().strip()

    def stats(self):
        from multiprocessing.connection import Client

        with Client(self.sock, family="AF_UNIX") as c:
            c.send(("stats",))
            assert c.poll(10)
            return c.recv()[1]

    def stop(self):
        if self.p.poll() is None:
            self.p.kill()
        self.p.wait(timeout=10)
        self.p.stdout.close()


@pytest.fixture
def owner(sockdir):
    made = []

    def start(*extra):
        o = OwnerProc(os.path.join(sockdir, "o.sock"), *extra)
        made.append(o)
        assert o.ready == f"READY {o.p.pid}", o.ready  # the READY line carries the owner's pid
        return o

    yield start
    for o in made:
        o.stop()


@pytest.fixture
def models(sockdir, monkeypatch):
    """In-process clients of the socket in sockdir; closed afterwards, and any owner they started is killed."""
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRESETS

    monkeypatch.setenv("SPOTTER_BATCH_SOCKET", os.path.join(sockdir, "o.sock"))
    made = []

    def make(cfg=None, **kw):
        opts = dict(stub=True, idle_exit_s=5.0, timeout_s=20.0, start_timeout_s=60.0)
        opts.update(kw.pop("opts", {}))
        m = SpotterForObjectDetection(cfg or PRESETS["r18vd"], batching="shared", **kw)
        m._shared_opts = opts
        made.append(m)
        return m

    yield make
    pids = {m._shared.owner_pid for m in made if m._shared is not None and m._shared.owner_pid}
    for m in made:
        if m._shared is not None:
            m._shared.close()
    for pid in pids:
        try:
            os.kill(pid, signal.SIGKILL)
        except ProcessLookupError:
            pass


def call(m, img):
    with torch.no_grad():
        return m(pixel_values=torch.from_numpy(img))


# What a child client process runs: connect and warm up, report READY, wait for the go line, make its calls, save
# every call's rows, close its slot, report DONE.
CHILD = r"""
import json, os, sys
import numpy as np, torch
a = json.loads(sys.argv[1])
sys.path.insert(0, a["root"]); sys.path.insert(0, os.path.join(a["root"], "tests"))
from test_shared_batch import image
from spotter_amd import SpotterForObjectDetection
m = SpotterForObjectDetection.from_pretrained("synthetic:r18vd", batching="shared")
m._shared_opts = dict(stub=True, idle_exit_s=5.0, timeout_s=30.0, start_timeout_s=60.0)
if a["warm"] == "call":
    m(pixel_values=torch.from_numpy(image(a["client"], 99)))
elif a["warm"] == "hello":
    m._shared_client().connect(image(0, 0).size)
print("READY", (m._shared.owner_pid if m._shared else 0) or 0, flush=True)
sys.stdin.readline()
lg, bx = [], []
for j in range(a["calls"]):
    out = m(pixel_values=torch.from_numpy(image(a["client"], j)))
    lg.append(out.logits.numpy()); bx.append(out.pred_boxes.numpy())
pid = m._shared.owner_pid
assert m._engine is None
m._shared.close()
np.savez(a["out"], logits=np.concatenate(lg), boxes=np.concatenate(bx))
print("DONE", pid, flush=True)
"""


class ChildClient:
    def __init__(self, sockdir, client, calls, warm="call"):
        self.client, self.calls = client, calls
        self.out = os.path.join(sockdir, f"out{client}.npz")
        env = _env()
        env["SPOTTER_BATCH_SOCKET"] = os.path.join(sockdir, "o.sock")
        arg = json.dumps({"root": ROOT, "client": client, "calls": calls, "out": self.out, "warm": warm})
        self.p = subprocess.Popen([sys.executable, "-c", CHILD, arg], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, env=env, cwd=ROOT)
        self.timer = threading.Timer(CHILD_TIMEOUT, self.p.kill)  # the child's own time limit
        self.timer.start()

    def wait_ready(self):
        line = self.p.stdout.readline()
        assert line.startswith("READY"), f"client {self.client} died before READY (rc {self.p.poll()})"
        return int(line.split()[1])

    def go(self):
        self.p.stdin.write("go\n")
        self.p.stdin.flush()

    def finish(self):
        """The owner pid the child saw; its rows are checked against its own images."""
        out, _ = self.p.communicate(timeout=CHILD_TIMEOUT)
        self.timer.cancel()
        done = [l for l in out.splitlines() if l.startswith("DONE")]
        assert self.p.returncode == 0 and done, f"client {self.client} failed (rc {self.p.returncode})"
        z = np.load(self.out)
        for j in range(self.calls):
            lg, bx = expected(image(self.client, j))
            np.testing.assert_allclose(z["logits"][j:j + 1], lg, rtol=0, atol=1e-6)
            np.testing.assert_allclose(z["boxes"][j:j + 1], bx, rtol=0, atol=1e-6)
        return int(done[0].split()[1])

    def kill(self):
        self.timer.cancel()
        if self.p.poll() is None:
            self.p.kill()
        self.p.wait(timeout=10)
        for f in (self.p.stdin, self.p.stdout):
            f.close()


def _until(cond, what, limit=20.0):
    end = time.monotonic() + limit
    while not cond():
        assert time.monotonic() < end, f"timed out waiting for {what}"
        time.sleep(0.005)


def _owners_of(sock):
    """Pids of the live owner processes serving `sock`, from their command lines."""
    found = []
    for d in os.listdir("/proc"):
        if d.isdigit():
            try:
                argv = open(f"/proc/{d}/cmdline", "rb").read().split(b"\0")
            except OSError:
                continue
            if b"spotter_amd.shared_batch" in argv and sock.encode() in argv:
                found.append(int(d))
    return sorted(found)


def test_six_processes_are_coalesced_and_each_gets_its_own_rows(sockdir, owner):
    o = owner("--max-wait-ms", "50", "--idle-exit-s", "30")
    kids = [ChildClient(sockdir, i, 5) for i in range(6)]
    try:
        for k in kids:
            k.wait_ready()
        for k in kids:
            k.go()
        pids = {k.finish() for k in kids}
        st = o.stats()
    finally:
        for k in kids:
            k.kill()
    assert pids == {o.p.pid}
    assert st["images"] == 36, st  # 6 warm-up calls + 30
    assert st["batches"] < st["images"] and st["max_batch"] > 1, st


def test_a_lone_client_is_dispatched_at_once(owner, models):
    owner("--max-wait-ms", "500")
    m = models()
    check_rows(call(m, image(0, 0)), image(0, 0))  # connects
    t0 = time.perf_counter()
    out = call(m, image(0, 1))
    dt = time.perf_counter() - t0
    check_rows(out, image(0, 1))
    assert dt < 0.25, f"a lone client's call took {dt * 1e3:.0f} ms with max_wait_ms=500"
    assert m._engine is None


def test_a_mismatched_hello_is_refused_by_field(owner, models):
    from spotter_amd.config import PRESETS

    o = owner()
    with pytest.raises(ValueError, match="precision differs"):
        call(models(precision="bf16"), image(0, 0))
    with pytest.raises(ValueError, match=r"config\.num_queries differs"):
        call(models(cfg=PRESETS["r18vd"].replace(num_queries=100)), image(0, 0))
    check_rows(call(models(), image(0, 2)), image(0, 2))  # the owner still serves a matching client
    assert o.stats()["images"] == 1


def test_a_failing_forward_reaches_every_client_of_the_batch_and_the_next_succeeds(owner, models):
    from spotter_amd.shared_batch import STUB_FAIL_VALUE

    # a submit is held until both connected clients have one waiting: each round below is one batch of two
    o = owner("--max-wait-ms", "20000")
    ms = [models(), models()]
    for m in ms:
        m._shared_client().connect(image(0, 0).size)

    def both(imgs):
        got = [None, None]

        def run(i):
            try:
                got[i] = call(ms[i], imgs[i])
            except Exception as e:
                got[i] = e

        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join(30)
        return got

    bad = image(0, 0)
    bad.reshape(-1)[0] = STUB_FAIL_VALUE
    got = both([bad, image(1, 0)])
    assert all(isinstance(g, RuntimeError) and "stub forward failure" in str(g) for g in got), got
    assert o.stats()["batches"] == 0  # the failed batch is not counted
    got = both([image(0, 1), image(1, 1)])
    check_rows(got[0], image(0, 1))
    check_rows(got[1], image(1, 1))
    st = o.stats()
    assert (st["batches"], st["images"], st["max_batch"]) == (1, 2, 2), st


def test_owner_killed_fails_the_pending_call_and_the_next_call_starts_a_new_owner(sockdir, models):
    from multiprocessing.connection import Client

    a, b = models(opts=dict(idle_exit_s=20.0)), models()
    b._shared_opts = dict(a._shared_opts)
    a.max_wait_ms = b.max_wait_ms = 10000.0  # the owner a's first call starts holds a batch for its idle clients
    check_rows(call(a, image(0, 0)), image(0, 0))  # no owner yet: this call starts one
    first = a._shared.owner_pid
    b._shared_client().connect(image(0, 0).size)
    assert b._shared.owner_pid == first
    got = []

    def pending():
        t0 = time.perf_counter()
        try:
            got.append(call(b, image(1, 1)))
        except Exception as e:
            got.append(e)
        got.append(time.perf_counter() - t0)

    t = threading.Thread(target=pending)
    t.start()

    def waiting():
        with Client(os.path.join(sockdir, "o.sock"), family="AF_UNIX") as c:
            c.send(("stats",))
            return c.poll(10) and c.recv()[1]["waiting"] == 1

    _until(waiting, "b's submit to be held for a")
    os.kill(first, signal.SIGKILL)
    t.join(30)
    assert isinstance(got[0], RuntimeError) and "went away" in str(got[0]), got
    assert got[1] < b._shared.timeout_s
    a._shared.close()
    check_rows(call(b, image(1, 2)), image(1, 2))  # reconnects: nobody listens, so it starts a new owner
    assert b._shared.owner_pid not in (None, first)


def test_a_killed_client_does_not_disturb_the_others(sockdir, owner):
    o = owner("--max-wait-ms", "10000", "--idle-exit-s", "30")
    victim = ChildClient(sockdir, 7, 1, warm="hello")
    kids = [ChildClient(sockdir, i, 3, warm="hello") for i in range(2)]
    try:
        for k in [victim] + kids:
            k.wait_ready()
        victim.go()  # its submit is held for the two idle clients
        _until(lambda: o.stats()["waiting"] == 1, "the victim's submit")
        victim.kill()
        _until(lambda: o.stats()["clients"] == 2, "the owner to drop the victim")
        for k in kids:
            k.go()
        for k in kids:
            k.finish()
        st = o.stats()
    finally:
        for k in [victim] + kids:
            k.kill()
    assert st["images"] == 6 and st["waiting"] == 0, st  # 2 x 3 calls; the victim's submit was discarded


def test_two_simultaneous_first_callers_start_exactly_one_owner(sockdir):
    kids = [ChildClient(sockdir, i, 2, warm="none") for i in range(2)]
    pids = set()
    try:
        for k in kids:
            k.wait_ready()
        for k in kids:
            k.go()
        pids = {k.finish() for k in kids}
        assert len(pids) == 1, pids
        assert _owners_of(os.path.join(sockdir, "o.sock")) == sorted(pids)
    finally:
        for k in kids:
            k.kill()
        for pid in pids:
            try:
                os.kill(pid, signal.SIGKILL)
            except ProcessLookupError:
                pass


def test_the_owner_exits_when_idle(sockdir, owner):
    o = owner("--idle-exit-s", "0.3")
    assert o.p.wait(timeout=20) == 0
    assert not os.path.exists(o.sock)  # and takes its socket with it


def test_batching_comes_from_the_environment_only_when_not_given(monkeypatch):
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRESETS

    monkeypatch.delenv("SPOTTER_BATCHING", raising=False)
    assert SpotterForObjectDetection.from_pretrained("synthetic:r18vd").batching is False
    for env, want in (("off", False), ("threads", True), ("shared", "shared")):
        monkeypatch.setenv("SPOTTER_BATCHING", env)
        assert SpotterForObjectDetection.from_pretrained("synthetic:r18vd").batching is want
    assert SpotterForObjectDetection.from_pretrained("synthetic:r18vd", batching=False).batching is False
    monkeypatch.setenv("SPOTTER_BATCHING", "bogus")
    with pytest.raises(ValueError, match="SPOTTER_BATCHING"):
        SpotterForObjectDetection.from_pretrained("synthetic:r18vd")
    assert SpotterForObjectDetection(PRESETS["r18vd"]).batching is False  # the constructor reads no environment
    with pytest.raises(ValueError, match="batching"):
        SpotterForObjectDetection(PRESETS["r18vd"], batching="bogus")
    assert SpotterForObjectDetection(PRESETS["r18vd"], batching="threads").batching is True


def test_a_pickled_shared_model_holds_no_connection_and_no_engine(owner, models):
    owner()
    m = models()
    check_rows(call(m, image(3, 0)), image(3, 0))
    assert m._shared is not None and m._shared._conn is not None
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.batching == "shared" and m2._shared is None and m2._engine is None and m._engine is None
    check_rows(call(m2, image(3, 1)), image(3, 1))  # and connects on its own
    m2._shared.close()


def test_copy_and_register_refuse_bad_arguments_before_any_device_call():
    from spotter_amd import _lib

    L = _lib.load()
    err = lambda: L.sp_last_error().decode()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)

    def desc(n, segs=()):
        d = _lib.SpCopySegmentsDesc(n=n)
        for i, (s, t, e) in enumerate(segs):
            d.seg[i].src, d.seg[i].dst, d.seg[i].elems = s, t, e
        return C.byref(d)

    assert L.sp_copy_segments(None, None) == -1 and "null descriptor" in err()
    for n in (0, -1, _lib.SP_COPY_MAX_SEGMENTS + 1):
        assert L.sp_copy_segments(desc(n), None) == -1 and f"n {n} outside [1, 64]" in err()
    assert L.sp_copy_segments(desc(2, [(p, p + 128, 4), (p, p + 128, -1)]), None) == -1 and "elems -1 < 0" in err()
    assert L.sp_copy_segments(desc(1, [(None, p, 4)]), None) == -1 and "null pointer" in err()
    assert L.sp_copy_segments(desc(1, [(p, None, 4)]), None) == -1 and "null pointer" in err()
    assert L.sp_copy_segments(desc(1, [(p + 2, p + 128, 4)]), None) == -1 and "4-byte aligned" in err()
    assert L.sp_copy_segments(desc(1, [(p, p + 128, 1 << 44)]), None) == -1 and "workgroups" in err()
    assert L.sp_copy_segments(desc(2, [(None, None, 0), (p, None, 0)]), None) == 0  # all empty: nothing to launch
    dev = C.c_void_p()
    assert L.sp_host_register(None, 4096, C.byref(dev)) == -1 and "null pointer" in err()
    assert L.sp_host_register(4096 * 16, 4096, None) == -1 and "null dev_ptr" in err()
    for nbytes in (0, -4096):
        assert L.sp_host_register(4096 * 16, nbytes, C.byref(dev)) == -1 and "<= 0" in err()
    assert L.sp_host_register(4096 * 16 + 64, 4096, C.byref(dev)) == -1 and "not aligned" in err()
    assert L.sp_host_unregister(None) == -1 and "null pointer" in err()
    assert L.sp_host_unregister(4096 * 16) == -1 and "not registered" in err()
    assert dev.value is None


def test_default_socket_names_the_physical_gpu(monkeypatch):
    from spotter_amd.shared_batch import default_socket

    for var in ("SPOTTER_BATCH_SOCKET", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    assert default_socket(3) == "/tmp/spotter-batch-gpu3.sock"
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "5")  # a Ray replica: its one GPU is index 0
    assert default_socket(0) == "/tmp/spotter-batch-gpu5.sock"
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "6,7")
    assert default_socket(1) == "/tmp/spotter-batch-gpu7.sock"
    monkeypatch.setenv("SPOTTER_BATCH_SOCKET", "/run/x.sock")
    assert default_socket(1) == "/run/x.sock"


def test_a_malformed_message_is_answered_and_the_owner_keeps_serving(owner, models):
    from multiprocessing.connection import Client

    o = owner()
    with Client(o.sock, family="AF_UNIX") as c:
        for msg in (("hello",), ("submit", 1), ("hello", {"config": "{}"}), "what", ("submit", 1, ("a", "b"))):
            c.send(msg)
            assert c.poll(10)
            assert c.recv()[0] in ("error", "refused", "done")
    check_rows(call(models(), image(4, 0)), image(4, 0))
