"""What one deployed MI355X serves: k Serve-replica processes sharing one GPU, each running the whole /detect
request loop of tools/detect_path.py (HTTP fetch from a local server → GPU JPEG decode → processor → model →
post-process → labels → draw → GPU JPEG encode → base64 → response JSON), back to back, for a fixed window.

The unchanged deployment class runs one image at a time on its event loop (reference serve.py:99-100,
179-181), so a replica serves at most one request per whole-request latency; more throughput per GPU needs
more replicas per GPU (Ray Serve `num_replicas` with fractional `ray_actor_options.num_gpus`). This measures
that trade: aggregate images/s and p50 / p95 whole-request latency for k = 1, 2, 4 ... processes on one GPU,
per precision (fp32 = the parity path, bf16 = C4).

    python tools/served_sweep.py --k 1 2 4 --precision fp32 bf16 --seconds 10 --out profiles/r6/served

--batching off shared runs every k in both layouts, alternating: `off` is the deployed layout (every process its own
engine), `shared` hands every forward to the one engine owner of the GPU (spotter_amd/shared_batch.py, started by the
first worker; SPOTTER_BATCHING reaches the workers through the environment). --check-outputs keeps every response's
labels and boxes in the workers and compares them, in the parent, with those of one single-process request of the
same image without batching: labels equal, boxes within tests/test_gpu_model.py's BOX_TOL_PX; any mismatch fails
the run (after that precision's points are written, with the count and the first difference per point).

Each worker process is started before any GPU call of the parent (the parent never touches the GPU), builds
its model, warms up (graph capture, decoder buffers), reports ready on stdout and waits for a common start
time on stdin; all workers then run requests until the common end time. Aggregate img/s = all requests
completed inside the window / the window.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stub_worker(ms: float):
    """CPU test stand-in for worker(): the same READY / start / RESULT protocol, a request is a sleep of `ms`."""
    print("READY", flush=True)
    t_start, t_end = (float(v) for v in sys.stdin.readline().split())
    while time.time() < t_start:
        time.sleep(0.0005)
    lat = []
    while time.time() < t_end:
        t0 = time.time()
        time.sleep(ms / 1e3)
        if time.time() <= t_end:
            lat.append((time.time() - t0) * 1e3)
    print("RESULT " + json.dumps({"pid": os.getpid(), "requests": len(lat), "lat_ms": [round(x, 3) for x in lat]}),
          flush=True)


BOX_TOL_PX = 0.5  # tests/test_gpu_model.py


def _recording(proc):
    """Make proc.post_process_object_detection remember what it returns: one (labels, boxes) per response, before
    the request loop's drawing jitter; identical responses are kept once, with a count."""
    seen = {}
    inner = proc.post_process_object_detection

    def post(*a, **k):
        res = inner(*a, **k)
        for det in res:
            key = json.dumps([[int(v) for v in det["labels"].tolist()],
                              [[round(float(c), 4) for c in b] for b in det["boxes"].tolist()],
                              [round(float(v), 5) for v in det["scores"].tolist()]])
            seen[key] = seen.get(key, 0) + 1
        return res

    proc.post_process_object_detection = post
    return seen


def compare_outputs(ref, got):
    """None if `got` (labels, boxes, scores) has ref's detections: the same labels, each with a box of its own
    within BOX_TOL_PX; else what differs (with the scores of the detections only one side has)."""
    (rl, rb, rs), (gl, gb, gs) = ref, got
    if sorted(rl) != sorted(gl):
        only = []
        for name, (al, as_), bl in (("reference", (rl, rs), gl), ("response", (gl, gs), rl)):
            for l in sorted(set(al)):
                extra = al.count(l) - bl.count(l)
                if extra > 0:  # the lowest-scored ones of that label are the ones at the threshold
                    low = sorted(s for x, s in zip(al, as_) if x == l)[:extra]
                    only.append(f"{name} has {extra} more of label {l} (its lowest scores there: {low})")
        return f"{len(gl)} detections against {len(rl)}: " + "; ".join(only)
    used = set()
    for l, b in zip(rl, rb):
        cand = [(max(abs(x - y) for x, y in zip(gb[j], b)), j) for j in range(len(gl)) if gl[j] == l and j not in used]
        d, j = min(cand)
        if d > BOX_TOL_PX:
            return f"label {l}: nearest box differs by {d:.3f} px > {BOX_TOL_PX}"
        used.add(j)
    return None


def worker(preset: str, precision: str, warmup: int, check: bool = False, reference: bool = False,
           batch_invariant: int | None = None):
    import asyncio

    import httpx
    import numpy as np
    import torch

    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.config import PRESETS
    from tools.detect_path import handle, opener, serve_bytes

    with open(os.path.join(ROOT, "tests", "golden", "test_pic.jpg"), "rb") as f:
        jpeg = f.read()
    srv, url = serve_bytes(jpeg)
    from spotter_amd.shared_batch import batching_from_env

    model = SpotterForObjectDetection(PRESETS[preset], use_graphs=True, precision=precision,
                                      batching=batching_from_env(), batch_invariant=batch_invariant)
    proc = SpotterImageProcessor()
    seen = _recording(proc) if check or reference else None
    body = json.dumps({"image_urls": [url]}).encode()
    open_fn = opener("gpu")
    rng = np.random.default_rng(os.getpid())

    async def run():
        lat = []
        async with httpx.AsyncClient() as client:
            for _ in range(warmup):
                await handle(body, client, proc, model, {}, open_fn, rng)
            torch.cuda.synchronize()
            if reference:  # one request's detections, nothing else
                return []
            if seen is not None:
                seen.clear()
            print("READY", flush=True)
            t_start, t_end = (float(v) for v in sys.stdin.readline().split())
            while time.time() < t_start:
                await asyncio.sleep(0.0005)
            while True:
                t0 = time.time()
                if t0 >= t_end:
                    break
                await handle(body, client, proc, model, {}, open_fn, rng)
                t1 = time.time()
                if t1 <= t_end:  # only requests completed inside the window count
                    lat.append((t1 - t0) * 1e3)
        return lat

    try:
        lat = asyncio.run(run())
    finally:
        srv.shutdown()
    res = {"pid": os.getpid(), "requests": len(lat), "lat_ms": [round(x, 3) for x in lat]}
    if seen is not None:
        res["outputs"] = [[json.loads(k), n] for k, n in seen.items()]
    print("RESULT " + json.dumps(res), flush=True)


def reference_outputs(preset: str, precision: str, timeout: float, batch_invariant: int | None = None):
    """(labels, boxes) of the fixture from ONE process without batching: what every checked response must equal."""
    env = dict(os.environ, SPOTTER_BATCHING="off")
    p = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--worker", "--reference", "--preset", preset,
                        "--precision", precision, "--warmup", "1", *_bi(batch_invariant)], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=timeout)
    line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
    if p.returncode != 0 or line is None:
        raise RuntimeError(f"reference run failed (rc {p.returncode}): {p.stderr[-2000:]}")
    outs = json.loads(line[len("RESULT "):])["outputs"]
    if len(outs) != 1:
        raise RuntimeError(f"reference run gave {len(outs)} different outputs for one request")
    return outs[0][0]


def _bi(batch_invariant):
    """The worker's command-line form of the batch-invariant setting."""
    return ["--batch-invariant", str(batch_invariant)] if batch_invariant else []


def _owner_stats(sock: str):
    from multiprocessing.connection import Client

    with Client(sock, family="AF_UNIX") as c:
        c.send(("stats",))
        if not c.poll(30):
            raise RuntimeError("the shared-batch owner does not answer")
        return c.recv()[1]


def sweep_point(k: int, precision: str, preset: str, seconds: float, warmup: int, timeout: float,
                stub_ms: float | None = None, batching: str = "off", reference=None, batch_invariant=None):
    import numpy as np

    env = dict(os.environ)
    env["SPOTTER_BATCHING"] = batching
    sock = None
    if batching == "shared" and stub_ms is None:  # this point's own owner, started by its first worker
        sock = env["SPOTTER_BATCH_SOCKET"] = f"/tmp/spotter-sweep-{os.getpid()}-{precision}-{k}.sock"
    extra = ["--stub-ms", str(stub_ms)] if stub_ms is not None else []
    if reference is not None:
        extra.append("--check-outputs")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), "--worker", "--preset", preset,
                               "--precision", precision,
                               "--warmup", str(warmup), *extra, *_bi(batch_invariant)],
                              stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)
             for _ in range(k)]
    try:
        deadline = time.time() + timeout
        for p in procs:  # every worker built its model and warmed up
            while True:
                line = p.stdout.readline()
                if not line:
                    raise RuntimeError(f"worker {p.pid} exited before READY (rc {p.wait()})")
                if line.startswith("READY"):
                    break
                if time.time() > deadline:
                    raise RuntimeError("workers not ready in time")
        st0 = _owner_stats(sock) if sock else None
        t_start = time.time() + 0.5
        t_end = t_start + seconds
        for p in procs:
            p.stdin.write(f"{t_start} {t_end}\n")
            p.stdin.flush()
        res = []
        for p in procs:
            out, _ = p.communicate(timeout=seconds + timeout)
            line = next((l for l in out.splitlines() if l.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:
                raise RuntimeError(f"worker {p.pid} failed (rc {p.returncode})")
            res.append(json.loads(line[len("RESULT "):]))
        st1 = _owner_stats(sock) if sock else None
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        if sock:  # the owner is its own session: end it here, so the next point starts with the GPU to itself
            _stop_owner(sock)
    lat = np.array([x for r in res for x in r["lat_ms"]])
    n = int(lat.size)
    out = {"k_processes": k, "precision": precision, "preset": preset, "window_s": seconds, "batching": batching,
           "batch_invariant": batch_invariant, "requests": n, "img_per_s": round(n / seconds, 1),
           "per_process_img_per_s": [round(r["requests"] / seconds, 1) for r in res],
           "p50_ms": round(float(np.percentile(lat, 50)), 3) if n else None,
           "p95_ms": round(float(np.percentile(lat, 95)), 3) if n else None,
           "p99_ms": round(float(np.percentile(lat, 99)), 3) if n else None}
    if st1 is not None:
        b, im = st1["batches"] - st0["batches"], st1["images"] - st0["images"]
        out.update(owner_batches=b, owner_images=im, mean_batch=round(im / b, 2) if b else None,
                   largest_batch=st1["max_batch"])
    if reference is not None:
        checked = wrong = 0
        first = None
        for r in res:
            for got, count in r["outputs"]:
                why = compare_outputs(reference, got)
                if why:
                    wrong += count
                    first = first or why
                checked += count
        out.update(responses_checked=checked, responses_mismatched=wrong)
        if first:
            out["first_mismatch"] = first
    return out


def _stop_owner(sock: str):
    import signal

    try:
        pid = _owner_stats(sock)["pid"]
    except (OSError, RuntimeError, EOFError):
        return
    os.kill(pid, signal.SIGTERM)
    end = time.time() + 30
    while os.path.exists(f"/proc/{pid}") and time.time() < end:
        time.sleep(0.05)
    for f in (sock, sock + ".lock"):
        if os.path.exists(f):
            os.unlink(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--precision", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--preset", default="r101vd")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--timeout", type=float, default=240.0, help="per sweep point: workers ready / finished")
    ap.add_argument("--out", default=None, help="directory for one JSON per precision")
    ap.add_argument("--stub-ms", type=float, default=None, help=argparse.SUPPRESS)  # CPU test: no GPU worker
    ap.add_argument("--batching", nargs="+", default=["off"], choices=["off", "shared"],
                    help="layouts to run at every k, alternating (SPOTTER_BATCHING of the workers)")
    ap.add_argument("--check-outputs", action="store_true",
                    help="compare every response's labels and boxes with a single-process run without batching")
    ap.add_argument("--reference", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch-invariant", type=int, default=0,
                    help="plan batch P of the batch-invariant mode for every replica, the owner and the reference; 0 = off")
    a = ap.parse_args()
    if a.worker:
        if a.stub_ms is not None:
            return stub_worker(a.stub_ms)
        return worker(a.preset, a.precision[0], a.warmup, a.check_outputs, a.reference, a.batch_invariant or None)
    if max(a.k) > 12:
        raise SystemExit("at most 12 processes per GPU (the box allows 16 GPU processes in all)")
    for prec in a.precision:
        ref = reference_outputs(a.preset, prec, a.timeout, a.batch_invariant) if a.check_outputs else None
        pts = {b: [] for b in a.batching}
        for k in a.k:
            for b in a.batching:
                r = sweep_point(k, prec, a.preset, a.seconds, a.warmup, a.timeout, batching=b, reference=ref,
                                batch_invariant=a.batch_invariant or None)
                print(json.dumps(r), flush=True)
                pts[b].append(r)
        for b in a.batching:
            best = max(pts[b], key=lambda r: r["img_per_s"])
            doc = {"what": "whole /detect request loop (tools/detect_path.py) in k processes sharing one MI355X, "
                           "1200x717 JPEG fixture, bs1 per request as the unchanged serve.py runs it"
                           + ("; forwards handed to one engine owner (spotter_amd/shared_batch.py)"
                              if b == "shared" else ""),
                   "precision": prec, "preset": a.preset, "batching": b, "outputs_checked": a.check_outputs,
                   "points": pts[b], "best_k": best["k_processes"], "best_img_per_s": best["img_per_s"]}
            if a.out:
                os.makedirs(a.out, exist_ok=True)
                name = (f"served_{a.preset}_{prec}" + ("" if b == "off" else f"_{b}")
                        + (f"_inv{a.batch_invariant}" if a.batch_invariant else "") + ".json")
                with open(os.path.join(a.out, name), "w") as f:
                    json.dump(doc, f, indent=1)
        bad = [r for b in a.batching for r in pts[b] if r.get("responses_mismatched")]
        if bad:  # after the points are written: the measurement is kept, the run still fails
            raise SystemExit("--check-outputs: responses differ from the single-process run without batching:\n"
                             + "\n".join(f"  k={r['k_processes']} {prec} batching={r['batching']}: "
                                          f"{r['responses_mismatched']} of {r['responses_checked']}: "
                                          f"{r['first_mismatch']}" for r in bad))
    return 0


if __name__ == "__main__":
    sys.exit(main())
