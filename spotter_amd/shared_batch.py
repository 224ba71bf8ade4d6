"""Batching across the replica PROCESSES that share one GPU.

The deployment runs several single-caller replica processes per MI355X, so spotter_amd.batching.MicroBatcher
(threads of one process) never has two calls to merge. Here one OWNER process per GPU holds the only Engine; the
replicas hand it their `pixel_values` through host shared memory, it coalesces whatever is waiting into one
forward and hands every replica its own rows back.

    python -m spotter_amd.shared_batch --device N --socket PATH --model NAME --precision P
                                       [--max-batch 16] [--max-wait-ms 2] [--idle-exit-s 60]

Slot: each client owns one multiprocessing.shared_memory block, an input area of 3·H·W floats and an output area
of Q·C + Q·4 floats (slot_layout). Both sides pin it with sp_host_register, so the owner's two sp_copy_segments
launches per batch (gather the B slot images into the contiguous [B,3,H,W] input; scatter every image's logits and
boxes into its slot) read and write the slots directly.

Messages (multiprocessing.connection over an AF_UNIX socket, all tiny):
    ("hello", {config, precision, batch_invariant, digest, shm, in_elems})  -> ("ok", {pid, stub}) | ("refused", field, text)
    ("submit", seq, (H, W))                                -> ("done", seq, error or None)
    ("stats",)                                             -> ("stats", {batches, images, max_batch, clients})

Collector rule: after the first submit the owner takes further same-shape submits until max_batch, or until every
connected client has a submit waiting, or max_wait_ms after the first; so a lone client is dispatched at once.
All signalling is on the host: no kernel waits on a flag.

Start-up: the first caller that finds no live owner on the socket takes an flock on PATH.lock, starts the owner as a
fresh child interpreter (subprocess.Popen, never exec), waits for its "READY <pid>" line and releases the lock;
concurrent first callers wait on the lock and then connect. The owner exits after idle_exit_s without a client.
"""
from __future__ import annotations

import argparse
import atexit
import hashlib
import json
import os
import sys
import threading
import time
import weakref
from multiprocessing import resource_tracker, shared_memory
from multiprocessing.connection import Client, Listener, wait

import numpy as np

PAGE = 4096
BATCHING_ENV = "SPOTTER_BATCHING"
SOCKET_ENV = "SPOTTER_BATCH_SOCKET"
MAX_BATCH_LIMIT = 32  # one scatter launch carries 2 segments per image (SP_COPY_MAX_SEGMENTS = 64)
STUB_FAIL_VALUE = -12345.0  # stub forward: an image whose first value is this makes the forward raise


def check_batching(value):
    """The constructor's `batching`: False / "off", True / "threads" (MicroBatcher), "shared" → False, True, "shared"."""
    if value is None or value is False or value == "off":
        return False
    if value is True or value == "threads":
        return True
    if value == "shared":
        return "shared"
    raise ValueError(f"batching {value!r} (e.g. from {BATCHING_ENV}) must be one of False, True, 'off', 'threads', "
                     "'shared'")


def batching_from_env():
    """SPOTTER_BATCHING (off | threads | shared) as a `batching` argument; unset → False."""
    v = os.environ.get(BATCHING_ENV)
    if v is None:
        return False
    if v not in ("off", "threads", "shared"):
        raise ValueError(f"{BATCHING_ENV}={v!r} must be one of ['off', 'shared', 'threads']")
    return check_batching(v)


def default_socket(device_index: int) -> str:
    """SPOTTER_BATCH_SOCKET, else /tmp/spotter-batch-gpu<index>.sock. Under a device mask (Ray gives every replica
    HIP_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES with its one GPU, which is then index 0 in each of them) <index> is
    the mask's entry, so the replicas of different GPUs of one node do not meet on one socket."""
    if os.environ.get(SOCKET_ENV):
        return os.environ[SOCKET_ENV]
    tag = str(device_index)
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        ids = [v.strip() for v in os.environ.get(var, "").split(",") if v.strip()]
        if device_index < len(ids):
            tag = ids[device_index]
            break
    return f"/tmp/spotter-batch-gpu{tag}.sock"


def _up(n: int, a: int) -> int:
    return (n + a - 1) // a * a


def slot_layout(in_elems: int, q: int, c: int):
    """Byte offsets of a slot's logits and boxes areas (64-byte aligned, after the input area) and its size."""
    logits_off = _up(4 * in_elems, 64)
    boxes_off = logits_off + _up(4 * q * c, 64)
    return logits_off, boxes_off, _up(boxes_off + 4 * q * 4, PAGE)


def weights_digest(weights: dict) -> str:
    """sha256 over the host weight dictionary: names, shapes, dtypes and bytes, in name order."""
    h = hashlib.sha256()
    for k in sorted(weights):
        a = np.ascontiguousarray(weights[k])
        h.update(f"{k}:{a.dtype}:{a.shape};".encode())
        h.update(a.view(np.uint8).reshape(-1).data)
    return h.hexdigest()


def _attach(name: str) -> shared_memory.SharedMemory:
    """Attach to another process's block without adopting it: the creator unlinks it."""
    shm = shared_memory.SharedMemory(name=name)
    try:  # Python < 3.13 registers attached blocks with this process's resource tracker, which would unlink them
        resource_tracker.unregister(shm._name, "shared_memory")
    except Exception:
        pass
    return shm


class _Slot:
    """One shared-memory block seen from one process: float32 views of its areas and, once registered, the device
    addresses of the same bytes."""

    def __init__(self, shm, in_elems: int, q: int, c: int, attached: bool = False):
        self.shm, self.in_elems, self.q, self.c, self.attached = shm, in_elems, q, c, attached
        self.logits_off, self.boxes_off, self.size = slot_layout(in_elems, q, c)
        if shm.size < self.size:
            raise ValueError(f"shared-memory block {shm.name} holds {shm.size} bytes, the slot needs {self.size}")
        self.all = np.frombuffer(shm.buf, dtype=np.float32, count=self.size // 4)
        self.addr = self.all.ctypes.data
        self.dev = None  # device address of byte 0 (sp_host_register)

    def image(self, elems: int):
        return self.all[:elems]

    def logits(self):
        return self.all[self.logits_off // 4: self.logits_off // 4 + self.q * self.c].reshape(self.q, self.c)

    def boxes(self):
        return self.all[self.boxes_off // 4: self.boxes_off // 4 + self.q * 4].reshape(self.q, 4)

    def register(self):
        from . import ops

        self.dev = ops.host_register(self.addr, self.size)

    def close(self, unlink: bool):
        if self.dev is not None:
            from . import ops

            try:
                ops.host_unregister(self.addr)
            except RuntimeError:
                pass
            self.dev = None
        self.all = None  # the views hold the buffer: drop them before closing it
        try:
            self.shm.close()
        except BufferError:
            pass
        if unlink:
            try:
                if self.attached:  # not this process's block: remove the name without its resource tracker
                    shared_memory._posixshmem.shm_unlink(self.shm._name)
                else:
                    self.shm.unlink()
            except FileNotFoundError:
                pass


# ------------------------------------------------------------------------------------------------------ owner

def stub_forward(images: np.ndarray, q: int, c: int):
    """The CPU tests' forward: every image's rows are a function of that image alone (its mean and its maximum)."""
    if (images.reshape(images.shape[0], -1)[:, 0] == STUB_FAIL_VALUE).any():
        raise RuntimeError("stub forward failure")
    flat = images.reshape(images.shape[0], -1).astype(np.float64)
    mean, top = flat.mean(1), flat.max(1)
    logits = mean[:, None, None] + 1e-3 * np.arange(q)[None, :, None] + 1e-6 * np.arange(c)[None, None, :]
    boxes = top[:, None, None] + 1e-3 * np.arange(q)[None, :, None] + 0.25 * np.arange(4)[None, None, :]
    return logits.astype(np.float32), boxes.astype(np.float32)


class _Peer:
    def __init__(self, conn):
        self.conn = conn
        self.slot = None
        self.pending = None  # (seq, (H, W), arrival time)


class Owner:
    def __init__(self, a):
        from .config import PRESETS, check_batch_invariant, check_precision

        self.a = a
        self.batch_invariant = check_batch_invariant(a.batch_invariant or None)  # 0 on the command line = off
        self.stub = a.stub
        self.max_batch = max(1, min(a.max_batch, MAX_BATCH_LIMIT))
        self.max_wait = a.max_wait_ms / 1e3
        self.precision = check_precision(a.precision)
        self.batches = self.images = self.max_seen = 0
        self.peers: dict = {}
        self._inputs = {}
        if self.stub:
            from .model import _preset_for

            name = a.model[len("synthetic:"):] if a.model.startswith("synthetic:") else a.model
            self.cfg = PRESETS[name] if name in PRESETS else _preset_for(name)
            self.model, self.digest = None, None
        else:
            import torch

            from .model import SpotterForObjectDetection

            torch.cuda.set_device(a.device)
            self.dev = torch.device("cuda", a.device)
            kw = {"revision": a.revision} if a.revision else {}
            self.model = SpotterForObjectDetection.from_pretrained(a.model, precision=self.precision, batching=False,
                                                                   batch_invariant=self.batch_invariant,
                                                                   **kw).to(self.dev)
            self.cfg = self.model.cfg
            self.digest = weights_digest(self.model._host_weights())
            self.model.engine  # the only Engine of this GPU, built before READY
        self.config_json = self.cfg.to_json()

    # -- connections --------------------------------------------------------------------------------------
    def _hello(self, peer: _Peer, h: dict):
        mine, theirs = json.loads(self.config_json), json.loads(h.get("config", "{}"))
        for k in sorted(set(mine) | set(theirs)):
            if mine.get(k) != theirs.get(k):
                return ("refused", f"config.{k}", f"owner has {mine.get(k)!r}, client has {theirs.get(k)!r}")
        if h.get("precision") != self.precision:
            return ("refused", "precision", f"owner runs {self.precision!r}, client asks {h.get('precision')!r}")
        if h.get("batch_invariant") != self.batch_invariant:  # another plan batch gives other bits
            return ("refused", "batch_invariant",
                    f"owner runs {self.batch_invariant!r}, client asks {h.get('batch_invariant')!r}")
        if self.digest is not None and h.get("digest") != self.digest:
            return ("refused", "digest", "the client's host weights are not the owner's")
        in_elems = int(h.get("in_elems", 0))
        if in_elems <= 0:
            return ("refused", "in_elems", f"input area of {in_elems} floats")
        try:
            slot = _Slot(_attach(h["shm"]), in_elems, self.cfg.num_queries, self.cfg.num_labels, attached=True)
            if not self.stub:
                slot.register()
        except Exception as e:  # a block that is gone or too small, or memory the device cannot pin
            return ("refused", "shm", f"{type(e).__name__}: {e}")
        if peer.slot is not None:
            peer.slot.close(unlink=False)  # the client re-created its block for a larger shape
        peer.slot = slot
        return ("ok", {"pid": os.getpid(), "stub": self.stub})

    def _drop(self, conn):
        peer = self.peers.pop(conn, None)
        if peer is not None and peer.slot is not None:
            peer.slot.close(unlink=True)  # a killed client cannot unlink its block; a live one already has
        try:
            conn.close()
        except OSError:
            pass

    def _send(self, conn, msg) -> bool:
        try:
            conn.send(msg)
            return True
        except (OSError, ValueError):
            self._drop(conn)
            return False

    def _handle(self, conn):
        peer = self.peers[conn]
        try:
            msg = conn.recv()
        except (EOFError, OSError):
            return self._drop(conn)
        kind = msg[0] if isinstance(msg, tuple) and msg else None
        try:
            self._message(conn, peer, kind, msg)
        except (IndexError, KeyError, TypeError, ValueError) as e:  # a malformed message ends nothing but itself
            self._send(conn, ("error", f"bad {kind!r} message: {type(e).__name__}: {e}"))

    def _message(self, conn, peer, kind, msg):
        if kind == "hello":
            self._send(conn, self._hello(peer, msg[1]))
        elif kind == "submit":
            seq, shape = msg[1], tuple(int(v) for v in msg[2])
            if peer.slot is None or peer.pending is not None or 3 * shape[0] * shape[1] > peer.slot.in_elems:
                why = ("no hello yet" if peer.slot is None else "a submit is already waiting"
                       if peer.pending is not None else f"shape {shape} exceeds the slot's input area")
                self._send(conn, ("done", seq, f"submit refused: {why}"))
            else:
                peer.pending = (seq, shape, time.perf_counter())
        elif kind == "stats":
            self._send(conn, ("stats", {"batches": self.batches, "images": self.images, "max_batch": self.max_seen,
                                        "clients": sum(1 for p in self.peers.values() if p.slot is not None),
                                        "waiting": sum(1 for p in self.peers.values() if p.pending is not None),
                                        "pid": os.getpid()}))
        else:
            self._send(conn, ("error", f"unknown message {kind!r}"))

    # -- batches ------------------------------------------------------------------------------------------
    def _due(self):
        """The batch to run now, or (None, seconds until the waiting one is due)."""
        waiting = sorted((p for p in self.peers.values() if p.pending is not None), key=lambda p: p.pending[2])
        if not waiting:
            return None, None
        first = waiting[0]
        batch = [p for p in waiting if p.pending[1] == first.pending[1]][:self.max_batch]
        clients = sum(1 for p in self.peers.values() if p.slot is not None)
        left = first.pending[2] + self.max_wait - time.perf_counter()
        if len(batch) >= self.max_batch or len(waiting) >= clients or left <= 0:
            return batch, 0.0
        return None, left

    def _forward_stub(self, batch, h, w):
        n = 3 * h * w
        x = np.stack([p.slot.image(n).copy() for p in batch])  # the gather, by numpy
        logits, boxes = stub_forward(x.reshape(len(batch), 3, h, w), self.cfg.num_queries, self.cfg.num_labels)
        for i, p in enumerate(batch):  # the scatter
            p.slot.logits()[...] = logits[i]
            p.slot.boxes()[...] = boxes[i]

    def _forward(self, batch, h, w):
        import torch

        from . import ops

        n, b = 3 * h * w, len(batch)
        q, c = self.cfg.num_queries, self.cfg.num_labels
        x = self._inputs.get((h, w))
        if x is None:
            x = self._inputs[(h, w)] = torch.empty((self.max_batch, 3, h, w), dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            ops.copy_segments([(p.slot.dev, x[i].data_ptr(), n) for i, p in enumerate(batch)])
            logits, boxes = self.model._run(x[:b])
            logits, boxes = logits.float().contiguous(), boxes.float().contiguous()
            if tuple(logits.shape) != (b, q, c) or tuple(boxes.shape) != (b, q, 4):
                raise RuntimeError(f"forward returned {tuple(logits.shape)}, {tuple(boxes.shape)}")
            segs = []
            for i, p in enumerate(batch):
                segs.append((logits[i].data_ptr(), p.slot.dev + p.slot.logits_off, q * c))
                segs.append((boxes[i].data_ptr(), p.slot.dev + p.slot.boxes_off, q * 4))
            ops.copy_segments(segs)
            torch.cuda.current_stream().synchronize()

    def _run_batch(self, batch):
        h, w = batch[0].pending[1]
        err = None
        try:
            (self._forward_stub if self.stub else self._forward)(batch, h, w)
            self.batches += 1
            self.images += len(batch)
            self.max_seen = max(self.max_seen, len(batch))
        except Exception as e:  # every client of this batch hears of it; the owner keeps serving
            err = f"{type(e).__name__}: {e}"
            print(f"shared_batch owner: batch of {len(batch)} failed: {err}", file=sys.stderr, flush=True)
        for p in batch:
            seq, p.pending = p.pending[0], None
            self._send(p.conn, ("done", seq, err))

    # -- main loop ----------------------------------------------------------------------------------------
    def serve(self):
        path = self.a.socket
        if os.path.exists(path):
            try:
                Client(path, family="AF_UNIX").close()
            except OSError:
                os.unlink(path)  # a dead owner's socket
            else:
                print(f"shared_batch owner: another owner is serving {path}", file=sys.stderr, flush=True)
                return 3
        listener = Listener(path, family="AF_UNIX", backlog=64)
        fresh, wake_r, wake_w = [], *os.pipe()
        lock = threading.Lock()

        def accept():
            while True:
                try:
                    conn = listener.accept()
                except OSError:
                    return
                with lock:
                    fresh.append(conn)
                os.write(wake_w, b"x")

        threading.Thread(target=accept, name="spotter-shared-accept", daemon=True).start()
        print(f"READY {os.getpid()}", flush=True)
        sys.stdout = sys.stderr  # the starter closes its end of stdout after READY: nothing may write there again
        os.dup2(2, 1)
        idle_since = time.perf_counter()
        try:
            while True:
                batch, left = self._due()
                if batch:
                    self._run_batch(batch)
                    continue
                if self.peers:
                    idle_since = time.perf_counter()
                    timeout = left
                else:
                    timeout = idle_since + self.a.idle_exit_s - time.perf_counter()
                    if timeout <= 0:
                        print(f"shared_batch owner: no client for {self.a.idle_exit_s} s, exiting "
                              f"({self.batches} batches, {self.images} images)", file=sys.stderr, flush=True)
                        return 0
                for r in wait(list(self.peers) + [wake_r], timeout):
                    if r == wake_r:
                        os.read(wake_r, 4096)
                        with lock:
                            new, fresh[:] = list(fresh), []
                        for conn in new:
                            self.peers[conn] = _Peer(conn)
                    elif r in self.peers:
                        self._handle(r)
        finally:
            listener.close()  # unlinks the socket
            for conn in list(self.peers):
                self._drop(conn)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m spotter_amd.shared_batch", description=__doc__.split("\n\n")[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--socket", required=True)
    ap.add_argument("--model", required=True)
    ap.add_argument("--revision", default=None)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--batch-invariant", type=int, default=0, help="plan batch P of the batch-invariant mode; 0 = off")
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--max-wait-ms", type=float, default=2.0)
    ap.add_argument("--idle-exit-s", type=float, default=60.0)
    ap.add_argument("--stub", action="store_true", help=argparse.SUPPRESS)  # CPU tests: numpy forward, no GPU
    return Owner(ap.parse_args(argv)).serve()


# ------------------------------------------------------------------------------------------------------ client

def _close_at_exit(ref):
    client = ref()
    if client is not None:
        client.close()


class SharedBatchClient:
    """A replica's side: one slot, one connection, one image in flight. Thread-safe by one lock."""

    def __init__(self, cfg, precision: str, model_name: str | None, digest_fn, socket_path: str, device_index: int = 0,
                 revision: str | None = None, max_batch: int = 16, max_wait_ms: float = 2.0,
                 idle_exit_s: float = 60.0, timeout_s: float = 30.0, start_timeout_s: float = 300.0,
                 stub: bool = False, batch_invariant: int | None = None):
        self.cfg, self.precision, self.model_name, self.revision = cfg, precision, model_name, revision
        self.batch_invariant = batch_invariant
        self._digest_fn, self._digest = digest_fn, None
        self.socket_path, self.device_index = socket_path, device_index
        self.max_batch, self.max_wait_ms, self.idle_exit_s = max_batch, max_wait_ms, idle_exit_s
        self.timeout_s, self.start_timeout_s, self.stub = timeout_s, start_timeout_s, stub
        self._conn = None
        self._greeted = False  # this connection's hello was accepted
        self._slot = None
        self._seq = 0
        self._lock = threading.Lock()
        self.owner_pid = None
        self.owner_stub = None
        atexit.register(_close_at_exit, weakref.ref(self))  # unlink the slot while the interpreter still can

    # -- owner start-up -----------------------------------------------------------------------------------
    def _spawn_owner(self):
        import select
        import subprocess

        if self.model_name is None:
            raise RuntimeError(f"no shared-batch owner on {self.socket_path}, and this model was not built by "
                               "from_pretrained, so there is no name to start one with")
        cmd = [sys.executable, "-m", "spotter_amd.shared_batch", "--device", str(self.device_index), "--socket",
               self.socket_path, "--model", self.model_name, "--precision", self.precision, "--max-batch",
               str(self.max_batch), "--max-wait-ms", str(self.max_wait_ms), "--idle-exit-s", str(self.idle_exit_s)]
        if self.batch_invariant:
            cmd += ["--batch-invariant", str(self.batch_invariant)]
        if self.revision:
            cmd += ["--revision", self.revision]
        if self.stub:
            cmd.append("--stub")
        env = dict(os.environ)
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        env["PYTHONPATH"] = root + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        env.pop(BATCHING_ENV, None)  # the owner runs the engine itself
        p = subprocess.Popen(cmd, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, env=env, start_new_session=True)
        deadline = time.monotonic() + self.start_timeout_s
        buf = b""
        try:
            while b"\n" not in buf:
                left = deadline - time.monotonic()
                if left <= 0:
                    p.kill()
                    raise RuntimeError(f"shared-batch owner not ready within {self.start_timeout_s} s")
                if select.select([p.stdout], [], [], min(left, 1.0))[0]:
                    chunk = os.read(p.stdout.fileno(), 256)
                    if not chunk:
                        raise RuntimeError(f"shared-batch owner exited before READY (rc {p.wait()})")
                    buf += chunk
            line = buf.split(b"\n")[0].decode(errors="replace")
            if not line.startswith("READY "):
                p.kill()
                raise RuntimeError(f"shared-batch owner said {line!r}, not READY")
        finally:
            p.stdout.close()
        # the owner is its own session and outlives this object; reap it from a thread if it ends first
        threading.Thread(target=p.wait, name="spotter-shared-owner-reaper", daemon=True).start()

    def _dial(self):
        try:
            return Client(self.socket_path, family="AF_UNIX")
        except (FileNotFoundError, ConnectionRefusedError):
            return None

    def _connect(self):
        import fcntl

        conn = self._dial()
        if conn is None:
            with open(self.socket_path + ".lock", "a") as lk:
                fcntl.flock(lk, fcntl.LOCK_EX)  # released when the file closes
                conn = self._dial()  # a concurrent first caller may have started it meanwhile
                if conn is None:
                    self._spawn_owner()
                    conn = self._dial()
            if conn is None:
                raise RuntimeError(f"shared-batch owner on {self.socket_path} does not accept connections")
        self._conn = conn

    # -- slot and hello -----------------------------------------------------------------------------------
    def _recv(self, timeout: float, what: str):
        try:
            if not self._conn.poll(timeout):
                self._reset()
                raise RuntimeError(f"shared-batch owner did not answer {what} within {timeout} s")
            return self._conn.recv()
        except (EOFError, OSError) as e:
            self._reset()
            raise RuntimeError(f"shared-batch owner went away during {what} ({type(e).__name__})") from None

    def _send(self, msg, what: str):
        try:
            self._conn.send(msg)
        except (OSError, ValueError) as e:
            self._reset()
            raise RuntimeError(f"shared-batch owner went away during {what} ({type(e).__name__})") from None

    def _reset(self):
        """Forget the connection (the next call reconnects or respawns); the slot stays."""
        if self._conn is not None:
            try:
                self._conn.close()
            except OSError:
                pass
        self._conn = None
        self._greeted = False

    def _hello(self, in_elems: int, on_gpu: bool):
        q, c = self.cfg.num_queries, self.cfg.num_labels
        if self._slot is None or self._slot.in_elems < in_elems:
            if self._slot is not None:
                self._slot.close(unlink=True)
                self._slot = None
            size = slot_layout(in_elems, q, c)[2]
            self._slot = _Slot(shared_memory.SharedMemory(create=True, size=size), in_elems, q, c)
        if self._digest is None:
            self._digest = self._digest_fn() if not self.stub else "stub"
        self._send(("hello", {"config": self.cfg.to_json(), "precision": self.precision, "digest": self._digest,
                              "batch_invariant": self.batch_invariant,
                              "shm": self._slot.shm.name, "in_elems": self._slot.in_elems}), "hello")
        r = self._recv(self.timeout_s, "hello")
        if r[0] == "refused":
            self._reset()
            raise ValueError(f"shared-batch owner on {self.socket_path} refused this model: {r[1]} differs ({r[2]})")
        if r[0] != "ok":
            self._reset()
            raise RuntimeError(f"shared-batch owner answered hello with {r!r}")
        self.owner_pid, self.owner_stub = r[1]["pid"], r[1]["stub"]
        self._greeted = True
        if on_gpu and not self.owner_stub and self._slot.dev is None:
            self._slot.register()  # pinned: the D2H / H2D copies below run at DMA speed

    def connect(self, in_elems: int, on_gpu: bool = False):
        """Connect (starting an owner if none listens) and announce a slot of in_elems input floats, without a call."""
        with self._lock:
            if self._conn is None:
                self._connect()
            if not self._greeted or self._slot.in_elems < in_elems:
                self._hello(max(in_elems, self._slot.in_elems if self._slot else 0), on_gpu)
        return self

    def stats(self) -> dict:
        with self._lock:
            if self._conn is None:
                self._connect()
            self._send(("stats",), "stats")
            return self._recv(self.timeout_s, "stats")[1]

    # -- one image ----------------------------------------------------------------------------------------
    def _one(self, image):
        """image: [3, H, W] float32 tensor (device or host) → (logits [Q, C], boxes [Q, 4]) on its device."""
        import torch

        h, w = int(image.shape[1]), int(image.shape[2])
        n = 3 * h * w
        if self._conn is None:
            self._connect()
        if not self._greeted or self._slot.in_elems < n:
            self._hello(max(n, self._slot.in_elems if self._slot else 0), image.is_cuda)
        slot = self._slot
        torch.from_numpy(slot.image(n)).copy_(image.reshape(-1))  # D2H, synchronous
        self._seq += 1
        self._send(("submit", self._seq, (h, w)), "submit")
        r = self._recv(self.timeout_s, "a forward")
        if r[0] != "done" or r[1] != self._seq:
            self._reset()
            raise RuntimeError(f"shared-batch owner answered submit {self._seq} with {r!r}")
        if r[2] is not None:
            raise RuntimeError(f"shared-batch forward failed: {r[2]}")
        return (torch.from_numpy(slot.logits()).to(image.device, copy=True),
                torch.from_numpy(slot.boxes()).to(image.device, copy=True))

    def __call__(self, pixel_values):
        """pixel_values [n, 3, H, W] → (logits [n, Q, C], boxes [n, Q, 4]); one image in flight at a time."""
        import torch

        x = pixel_values.float()
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"pixel_values must be [n, 3, H, W], got {tuple(x.shape)}")
        with self._lock:
            outs = [self._one(x[i].contiguous()) for i in range(x.shape[0])]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])

    def close(self):
        with self._lock:
            self._reset()
            if self._slot is not None:
                self._slot.close(unlink=True)
                self._slot = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


if __name__ == "__main__":
    sys.exit(main())
