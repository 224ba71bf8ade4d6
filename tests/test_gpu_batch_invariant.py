"""GPU: the batch-invariant mode (sp_set_plan_batch, Engine(batch_invariant=P)).

Every comparison here is exact: bit patterns (int32 views), every image, every row, no tolerance.

Kernel level: one linear and one 3×3 conv per operand mode, on shapes whose default plans at B = 1 and B = 32 differ
(asserted through sp_conv_plan), both Winograd sizes, and the folded split-K tile against the split launch + reduce.
Model level: R18vd at 640² (fp32 and bf16) and one R101vd bf16 case, each image alone against the same image in
every slot of batches of 2, 3, 5 and 8, graph replay against eager, two micro-batch streams against one, P = 4 at
B = 1 against B = 8, and the fp32 parity bar under the mode. Shared batching: co-batched bf16 responses against
single-process ones.
"""
import json
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
from test_gpu_model import GOLD, check_image, load_images  # noqa: E402

MODES = ("x3", "x2", "bf16", "f32")
BATCHES = (1, 2, 5, 32)
NIMG = 32


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _reset():
    from spotter_amd import ops

    yield
    ops.set_plan_batch(0, 0)
    ops.set_tuning(ops.TUNE_FOLD, None)
    ops.force_splitk_config(None)
    ops.force_conv_config(None)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def wkw(mode, wt, dev):
    from spotter_amd import ops

    return {"f32": {}, "x3": {"wt_planes": ops.split_bf16x3(wt)}, "x2": {"wt_planes": ops.split_bf16x2(wt)},
            "bf16": {"wt16": T(ops.bf16_bits(wt.cpu().numpy()).view(np.int16), dev)}}[mode]


class Conv:
    """One conv / linear layer on NIMG random images (h × w × cin rows each), launched on any run of them."""

    def __init__(self, dev, mode, h, w, cin, cout, k, seed, epi=("affine", "res1", "act"), bf16_rows=False, nimg=NIMG):
        from spotter_amd import ops

        rng = np.random.default_rng(seed)
        self.dev, self.mode, self.shape, self.k, self.epi, self.bf16_rows = dev, mode, (h, w, cin, cout), k, epi, bf16_rows
        self.rows = h * w
        x = rng.standard_normal((nimg * self.rows * cin,)).astype(np.float32)
        self.x = T(ops.bf16_bits(x).view(np.int16), dev) if bf16_rows else T(x, dev)
        self.wt = T((rng.standard_normal((cout, k * k * cin)) / np.sqrt(cin * k * k)).astype(np.float32), dev)
        self.kw = wkw(mode, self.wt, dev)
        self.r1 = T(rng.standard_normal(nimg * self.rows * cout).astype(np.float32), dev)
        self.sc = T(rng.uniform(0.5, 1.5, cout).astype(np.float32), dev)
        self.sh = T(rng.standard_normal(cout).astype(np.float32), dev)
        self.rs = T(rng.uniform(0.5, 1.5, self.rows).astype(np.float32), dev)
        self.ws = torch.empty(16 * nimg * self.rows * ((cout + 3) & ~3), device=dev)

    def args(self, first, n, out):
        from spotter_amd.ops import V

        h, w, cin, cout = self.shape
        kw = dict(self.kw)
        if "affine" in self.epi:
            kw.update(scale=self.sc, shift=self.sh)
        if "res1" in self.epi:
            kw["res1"] = V(self.r1, first * self.rows * cout, cout)
        if "act" in self.epi:
            kw["act"] = "silu"
        if "row_scale" in self.epi:
            kw["row_scale"] = self.rs
        if not self.bf16_rows:
            kw["workspace"] = self.ws
        return (V(self.x, first * self.rows * cin, cin), n, h, w, cin, self.wt, cout, self.k, 1, self.k // 2, out), kw

    def out(self, n):
        cout = self.shape[3]
        if self.bf16_rows:
            return torch.full((n * self.rows * cout,), 0x7FC0, dtype=torch.int16, device=self.dev)
        return torch.full((n * self.rows * cout,), float("nan"), device=self.dev)

    def plan(self, n):
        from spotter_amd import ops
        from spotter_amd.ops import view

        a, kw = self.args(0, n, view(self.out(n), self.shape[3]))
        return ops.conv_plan(ops.conv_desc(*a, **kw)[0])

    def run(self, first, n, wino=None):
        from spotter_amd import ops
        from spotter_amd.ops import view

        o = self.out(n)
        a, kw = self.args(first, n, view(o, self.shape[3]))
        if wino is not None:
            kw.pop("workspace", None)
            kw["wino"] = wino
        ops.conv2d(*a, **kw)
        got = o.cpu().numpy()
        got = got.view(np.int16) if self.bf16_rows else got.view(np.int32)
        return got.reshape(n, -1)


def arith(p):
    return tuple(p[f] for f in ("family", "tile", "planes", "generic", "a_bf16", "splits"))


def check_every_slot(layer, run=None):
    """Each of the NIMG images alone (planned as itself), then runs of B images under plan_batch = 1 starting at
    two different images, so every slot of every B is compared and every image is seen in more than one slot."""
    from spotter_amd import ops

    run = run or layer.run
    ops.set_plan_batch(0, 0)
    alone = np.concatenate([run(i, 1) for i in range(NIMG)])
    nan = 0x7FC0 if layer.bf16_rows else np.float32("nan").view(np.int32)
    assert not (alone == nan).all(axis=1).any()
    for B in BATCHES:
        ops.set_plan_batch(B, 1)
        for first in sorted({0, min(3, NIMG - B), NIMG - B}):
            got = run(first, B)
            np.testing.assert_array_equal(got, alone[first:first + B], err_msg=f"B={B} first={first}")
    ops.set_plan_batch(0, 0)


@pytest.mark.parametrize("mode", MODES)
def test_linear_is_batch_invariant(dev, mode):
    """300 rows per image (ragged against 64), K = 1024 → 256: 4-way split-K at B = 1, none at B = 32."""
    layer = Conv(dev, mode, 1, 300, 1024, 256, 1, seed=11)
    p1, p32 = layer.plan(1), layer.plan(32)
    assert p1["splits"] == 4 and p32["splits"] == 1 and arith(p1) != arith(p32), (p1, p32)
    check_every_slot(layer)


@pytest.mark.parametrize("mode", MODES)
def test_conv3x3_is_batch_invariant(dev, mode):
    """20 × 20 × 256 → 256, 3×3: 400 rows per image, 9-way split-K at B = 1 and 2-way at B = 32."""
    layer = Conv(dev, mode, 20, 20, 256, 256, 3, seed=12)
    p1, p32 = layer.plan(1), layer.plan(32)
    assert p1["splits"] > p32["splits"] >= 1 and arith(p1) != arith(p32), (p1, p32)
    check_every_slot(layer)


def test_bf16_rows_tile_change_is_batch_invariant(dev):
    """bf16 rows, 28 × 28 × 256 → 256, 3×3 (784 rows per image): tiles(256, 128) is 8 at B = 1 (the 64×64 tile on
    32x32x16 MFMAs) and 196 >= 192 at B = 32 (tile 41, 256×128 on 16x16x32 MFMAs)."""
    layer = Conv(dev, "bf16", 28, 28, 256, 256, 3, seed=13, epi=("affine", "act"), bf16_rows=True)
    p1, p32 = layer.plan(1), layer.plan(32)
    assert p1["tile"] == 14 and p32["tile"] == 41 and p1["a_bf16"] == p32["a_bf16"] == 1, (p1, p32)
    check_every_slot(layer)


@pytest.mark.parametrize("mode", ("x3", "x2", "bf16"))
@pytest.mark.parametrize("wm", (2, 4))
def test_winograd_is_batch_invariant(dev, wm, mode):
    """18 × 18 × 64 → 128 (ragged against both tile sizes): the component GEMM runs the 64×64 tile at B = 1 and the
    128×128 k16 tile from 12 000 component rows up (B = 32)."""
    from spotter_amd import ops

    layer = Conv(dev, mode, 18, 18, 64, 128, 3, seed=14 + wm)
    h, w, cin, cout = layer.shape
    u = ops.winograd_weights_host(layer.wt.cpu().numpy().reshape(cout, 3, 3, cin), wm)
    planes = {"x3": ops.split_bf16x3_host, "x2": ops.split_bf16x2_host,
              "bf16": lambda a: ops.bf16_bits(a).reshape(1, -1).view(np.int16)}[mode](u)
    planes = T(planes, dev)
    tiles = -(-h // wm) * -(-w // wm)
    work = torch.empty(ops.wino_work_elems(wm, NIMG * tiles, cin, cout), device=dev)

    def plan(n):
        from spotter_amd.ops import view

        a, kw = layer.args(0, n, view(layer.out(n), cout))
        kw.pop("workspace", None)
        d = ops.conv_desc(*a, **kw)[0]
        d.precision = ops.PREC_BY_PLANES[planes.shape[0]]
        return ops.wino_plan(d, wm)["gemm"]

    p1, p32 = plan(1), plan(32)
    assert p1["tile"] == 14 and p32["tile"] == 46, (p1, p32)
    check_every_slot(layer, run=lambda first, n: layer.run(first, n, wino=(planes, work, wm)))


# ------------------------------------------------------------------------------------------------ folded split-K
# (rows per image, K, Cout, k, images, epilogue): S = 2 and S = 16 (the planner's cap), K no multiple of S·32,
# Cout ragged against 64 (with and without the float4 epilogue), one tile of M and ragged M
FOLD_CASES = [
    ((1, 300, 1024, 256, 1), 8, ("affine", "res1", "act")),        # S = 4, the decoder's linear
    ((1, 64, 4096 + 96, 64, 1), 1, ()),                             # S = 16, one tile, K = 131 k-tiles
    ((1, 37, 4096 + 96, 100, 1), 1, ("affine", "res1", "act")),     # S = 16, a ragged tile of M and of Cout
    ((80, 80, 256, 384, 3), 1, ("affine", "act")),                  # S = 2 (6400 rows × 384: 600 tiles, 72 k-tiles)
    ((20, 20, 256, 90, 3), 2, ("res1",)),                           # Cout % 4 != 0: the scalar epilogue
    ((1, 300, 1024, 256, 1), 5, ("affine", "row_scale", "res1")),   # row_scale (period 300), M ragged
    ((5, 7, 288, 96, 3), 3, ("act",)),                              # K = 2592 = 81 k-tiles
]


@pytest.mark.parametrize("mode", ("x3", "x2", "bf16"))
@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: "x".join(map(str, c[0])) + "-" + "+".join(c[2]) if isinstance(c, tuple) and len(c) == 3 else None)
def test_folded_matches_split_reduce(dev, mode, case):
    """The folded 64×64 split tile (forced for every split: sp_set_tuning SP_TUNE_FOLD = 2) against the split launch
    + splitk_reduce_kernel (SP_TUNE_FOLD = 1), bit for bit; the folded launch leaves the workspace untouched."""
    from spotter_amd import ops

    (h, w, cin, cout, k), n, epi = case
    layer = Conv(dev, mode, h, w, cin, cout, k, seed=21, epi=epi, nimg=n)
    ops.set_plan_batch(n, 1)
    p = layer.plan(n)
    want = {(1, 300, 1024, 256, 1): 4, (1, 64, 4192, 64, 1): 16, (1, 37, 4192, 100, 1): 16, (80, 80, 256, 384, 3): 2}
    assert p["splits"] > 1 and p["family"] == 1 and p["tile"] == 4 and not p["generic"], p
    assert p["splits"] == want.get((h, w, cin, cout, k), p["splits"]), p
    ops.set_tuning(ops.TUNE_FOLD, 1)
    layer.ws.fill_(float("nan"))
    ref = layer.run(0, n)
    assert not torch.isnan(layer.ws[:p["splits"] * n * layer.rows * ((cout + 3) & ~3)]).any()  # the slabs were written
    ops.set_tuning(ops.TUNE_FOLD, 2)
    layer.ws.fill_(float("nan"))
    got = layer.run(0, n)
    assert torch.isnan(layer.ws).all()  # no workspace traffic
    assert not (ref == np.float32("nan").view(np.int32)).all(axis=1).any()
    np.testing.assert_array_equal(got, ref)


def test_the_launch_rule_takes_the_folded_form_only_on_a_full_grid(dev):
    """plan_batch = 1 on the 300-row linear: B = 2 (10 × 4 tiles) still splits for real, B = 32 (150 × 4 = 600
    tiles, no split at that M) runs folded: seen in the workspace, which only the real split writes."""
    from spotter_amd import ops

    layer = Conv(dev, "x3", 1, 300, 1024, 256, 1, seed=22)
    for B, folded in ((2, False), (32, True)):
        ops.set_plan_batch(B, 1)
        assert layer.plan(B)["splits"] == 4
        layer.ws.fill_(float("nan"))
        layer.run(0, B)
        assert bool(torch.isnan(layer.ws).all()) == folded, B


def test_fast_1x1_is_bit_identical(dev):
    """sp_conv_plan_info.fast_1x1 follows the launch's own rows (32-bit addressing: M · lda · 4 < 2^32). The two
    forms give the same bits: 1024 rows of 256 → 256 with lda = 256, and the same rows 2^20 floats apart."""
    from spotter_amd import ops
    from spotter_amd.ops import view

    rng = np.random.default_rng(5)
    m, cin, cout, lda = 1024, 256, 256, 1 << 20
    x = rng.standard_normal((m, cin)).astype(np.float32)
    wt = T((rng.standard_normal((cout, cin)) / 16).astype(np.float32), dev)
    wide = torch.zeros((m - 1) * lda + cin, device=dev)
    wide.as_strided((m, cin), (lda, 1)).copy_(T(x, dev))
    for mode in ("x3", "bf16"):
        outs, fast = [], []
        for src in (view(T(x.reshape(-1), dev), cin), view(wide, lda)):
            o = torch.full((m * cout,), float("nan"), device=dev)
            a = (src, 1, 1, m, cin, wt, cout, 1, 1, 0, view(o, cout))
            fast.append(ops.conv_plan(ops.conv_desc(*a, **wkw(mode, wt, dev))[0])["fast_1x1"])
            ops.conv2d(*a, **wkw(mode, wt, dev))
            outs.append(bits(o))
        assert fast == [1, 0]
        assert not np.isnan(outs[0].view(np.float32)).any()
        np.testing.assert_array_equal(outs[1], outs[0])


# ------------------------------------------------------------------------------------------------ model level
@pytest.fixture(scope="module")
def pixels(dev):
    from spotter_amd import SpotterImageProcessor

    g = np.load(os.path.join(GOLD, "r18vd_640.npz"))
    return SpotterImageProcessor()(images=load_images(g), return_tensors="pt")["pixel_values"].to(dev)


def fwd(eng, px, **kw):
    with torch.no_grad():
        lg, bx = eng.forward(px, **kw)
    return bits(lg).copy(), bits(bx).copy()


def rotations(px, B):
    """len(px) batches of B images, slot s of batch r holding image (s + r) % n: every image in every slot."""
    n = px.shape[0]
    for r in range(n):
        idx = [(s + r) % n for s in range(B)]
        yield idx, px[idx].contiguous()


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
def test_r18vd_outputs_do_not_depend_on_batch_or_slot(dev, pixels, precision):
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRESETS

    model = SpotterForObjectDetection(PRESETS["r18vd"], precision=precision, batch_invariant=1, use_graphs=True)
    eng = model.engine
    assert eng.batch_invariant == 1
    n = pixels.shape[0]
    alone = [fwd(eng, pixels[i:i + 1]) for i in range(n)]
    assert not any(np.isnan(a.view(np.float32)).any() for pair in alone for a in pair)
    for B in (2, 3, 5, 8):
        for idx, px in rotations(pixels, B):
            lg, bx = fwd(eng, px)
            for s, i in enumerate(idx):
                np.testing.assert_array_equal(lg[s], alone[i][0][0], err_msg=f"logits B={B} slot={s} image={i}")
                np.testing.assert_array_equal(bx[s], alone[i][1][0], err_msg=f"boxes B={B} slot={s} image={i}")
    # two micro-batch streams against one (B = 5: slices of 2 and 3 images)
    idx, px = next(rotations(pixels, 5))
    one, two = fwd(eng, px, microbatches=1), fwd(eng, px, microbatches=2)
    np.testing.assert_array_equal(two[0], one[0])
    np.testing.assert_array_equal(two[1], one[1])
    # graph replay (B <= 4) against eager: the model's own path, second call captures, third replays
    for B in (1, 3):
        idx, px = next(rotations(pixels, B))
        for _ in range(3):
            with torch.no_grad():
                lg, bx = model._run(px)
            lg, bx = bits(lg).copy(), bits(bx).copy()
        assert tuple(px.shape) in model._graphs
        for s, i in enumerate(idx):
            np.testing.assert_array_equal(lg[s], alone[i][0][0], err_msg=f"graph logits B={B} slot={s}")
            np.testing.assert_array_equal(bx[s], alone[i][1][0], err_msg=f"graph boxes B={B} slot={s}")
    # the library's setting does not outlive a forward
    from spotter_amd import ops

    layer = Conv(dev, "x3", 1, 300, 1024, 256, 1, seed=3)
    assert layer.plan(32)["splits"] == 1


@pytest.mark.parametrize("precision", ("fp32", "bf16"))
def test_plan_batch_4_at_b1_and_b8(dev, pixels, precision):
    from spotter_amd.config import PRESETS
    from spotter_amd.engine import Engine
    from spotter_amd.weights import generate

    eng = Engine(PRESETS["r18vd"], generate(PRESETS["r18vd"], seed=0), dev, precision=precision, batch_invariant=4)
    idx, px = next(rotations(pixels, 8))
    lg8, bx8 = fwd(eng, px)
    for s in (0, 3, 7):
        lg1, bx1 = fwd(eng, px[s:s + 1])
        np.testing.assert_array_equal(lg8[s], lg1[0])
        np.testing.assert_array_equal(bx8[s], bx1[0])


def test_r101vd_bf16_b1_against_b4(dev, pixels):
    from spotter_amd.config import PRESETS
    from spotter_amd.engine import Engine
    from spotter_amd.weights import generate

    eng = Engine(PRESETS["r101vd"], generate(PRESETS["r101vd"], seed=0), dev, precision="bf16", batch_invariant=1)
    idx, px = next(rotations(pixels, 4))
    lg4, bx4 = fwd(eng, px)
    for s in range(4):
        lg1, bx1 = fwd(eng, px[s:s + 1])
        np.testing.assert_array_equal(lg4[s], lg1[0])
        np.testing.assert_array_equal(bx4[s], bx1[0])


def test_invariant_fp32_still_meets_the_parity_bar(dev):
    """batch_invariant=1 at fp32 against the HF goldens, at the existing bar (check_image), with the images batched."""
    from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
    from spotter_amd.config import PRESETS

    g = np.load(os.path.join(GOLD, "r18vd_640.npz"))
    model = SpotterForObjectDetection(PRESETS["r18vd"], use_graphs=False, precision="fp32", batch_invariant=1)
    proc = SpotterImageProcessor(size={"height": int(g["size"]), "width": int(g["size"])})
    imgs = load_images(g)
    with torch.no_grad():
        out = model(**proc(images=imgs, return_tensors="pt").to("cpu"))
    dets = proc.post_process_object_detection(out, target_sizes=torch.tensor(g["target_sizes"]), threshold=0.5)
    topk = model.engine._ws["topk"][:len(imgs) * 300].cpu().numpy().reshape(len(imgs), 300)
    for i in range(len(imgs)):
        check_image(g, i, dets[i], out.logits[i].cpu().numpy(), out.pred_boxes[i].cpu().numpy(), topk[i])


# ------------------------------------------------------------------------------------------------ shared batching
CHILD = r"""
import json, os, sys
a = json.loads(sys.argv[1])
sys.path.insert(0, a["root"])
import numpy as np, torch
from spotter_amd import SpotterForObjectDetection, SpotterImageProcessor
from spotter_amd.synthetic import synthetic_image
m = SpotterForObjectDetection.from_pretrained("synthetic:r18vd", batching="shared", precision="bf16", batch_invariant=1)
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
    res[f"logits{i}"] = out.logits[0].cpu().numpy()
    res[f"boxes{i}"] = out.pred_boxes[0].cpu().numpy()
assert m._engine is None and m._batcher is None
m._shared.close()
np.savez(a["out"], **res)
print("DONE engine_is_none", flush=True)
"""


def test_co_batched_bf16_responses_equal_single_process_ones(tmp_path):
    """tests/test_gpu_shared_batch.py's end-to-end run in bf16 with the setting on: three client processes, one owner;
    every response equals, bit for bit, what a single-process model with the same setting answers."""
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
    env.pop("SPOTTER_BATCH_INVARIANT", None)
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
                       "synthetic:r18vd", "--precision", "bf16", "--batch-invariant", "1", "--max-wait-ms", "50",
                       "--idle-exit-s", "60"], 150, stdin=subprocess.DEVNULL)
        assert line(owner, "READY", "the owner").split()[1] == str(owner.pid)
        kids = []
        for i in range(3):
            arg = json.dumps({"root": ROOT, "seeds": seeds[i], "out": str(tmp_path / f"c{i}.npz")})
            kids.append(start([sys.executable, "-c", CHILD, arg], 150, stdin=subprocess.PIPE))
        ref_model = SpotterForObjectDetection(PRESETS["r18vd"], use_graphs=False, precision="bf16", batch_invariant=1)
        proc = SpotterImageProcessor()
        ref = {}
        for s in sum(seeds, []):
            with torch.no_grad():
                out = ref_model(**proc(images=synthetic_image(s)))
            ref[s] = (out.logits[0].cpu().numpy(), out.pred_boxes[0].cpu().numpy())
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
    assert st["images"] == 6 and st["batches"] < st["images"], st  # some responses were co-batched
    for i in range(3):
        z = np.load(tmp_path / f"c{i}.npz")
        for j, s in enumerate(seeds[i]):
            np.testing.assert_array_equal(z[f"logits{j}"].view(np.int32), ref[s][0].view(np.int32))
            np.testing.assert_array_equal(z[f"boxes{j}"].view(np.int32), ref[s][1].view(np.int32))
