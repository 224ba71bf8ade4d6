"""Every conv / GEMM instance sp_conv2d can launch, pinned by sp_conv_plan and compared with fp64 (tests/conv_refs.py).

One test per target tuple of the coverage ledger (tests/test_conv_refs.py proves on the host that the matrix
reaches every tuple): for each of its cases build the descriptor once (ops.conv_desc), assert that
ops.conv_plan names exactly the targeted instance, launch that same descriptor (ops.conv_launch) into a
NaN-prefilled output with 8 guard columns per row and a guard tail, and compare: `probe` and `ints` bit for bit
with the mode's fp64 operand model, `range` element by element against the derived bound. Guards must still be
NaN (bf16 rows: the 0x7FC0 fill), split-K arrival counters zero.

DESIGN.md 5.13 has the exactness argument, the bound's terms, the ledger rule and the figures measured on the
MI355X (worst err / bound per mode and epilogue variant, wall times, launches, the four kernel mutants); -s prints
them per test and for the file.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as R  # noqa: E402

BF16_NAN = 0x7FC0
LAUNCHES = {"n": 0}
WORST = {}  # (mode, epilogue variant) → worst err / bound of the range family


@pytest.fixture(scope="module")
def dev():
    from spotter_amd._lib import lib

    assert lib().sp_device_init(0) == 0, lib().sp_last_error()
    d = torch.device("cuda", 0)
    yield d
    print(f"\nconv plans: {LAUNCHES['n']} launches; worst range err / bound per (mode, epilogue): "
          + ", ".join(f"{k[0]}/e{k[1]} {v:.3f}" for k, v in sorted(WORST.items())))


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rows(a, ld, off, numel, dev, bf16=False, fill=0.0):
    """[rows, cols] host values → a device buffer of `numel` elements holding them as rows `ld` apart from `off`
    (fp32, or bf16 bit patterns as int16)."""
    rows, cols = a.shape
    if bf16:
        buf = np.full(numel, 0, np.uint16)
        v = R.bf16_bits(a.astype(np.float32))
    else:
        buf = np.full(numel, fill, np.float32)
        v = a.astype(np.float32)
    idx = off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
    buf[idx] = v
    return T(buf.view(np.int16) if bf16 else buf, dev)


def run_case(c, dev):
    """Plan + launch one case → (plan key, splits, got [M, Cout] fp32, got_bits or None); asserts the guards."""
    from spotter_amd import ops
    from spotter_amd.ops import view

    n, h, w, cin, cout, k, st, pad = c["shape"]
    L = R.layout(c)
    m = L["M"]
    with R.overrides(c["ov"]):
        # the plan decides the split factor the bound counts; the operands do not depend on it
        key0, splits = R.plan_of(R.fake_desc(c))
    r = R.build(c, splits)
    kw = {}
    x = view(_rows(r["a1"].reshape(-1, cin), L["lda"], c["a_off"], L["a_numel"], dev, bf16=c["a_rows"]), L["lda"],
             c["a_off"])
    wt = T(r["w"], dev)
    if c["mode"] == "bf16":
        kw["wt16"] = T(r["w_bits"].view(np.int16), dev)
    elif c["mode"] in ("x3", "x2"):
        kw["wt_planes"] = (ops.split_bf16x3 if c["mode"] == "x3" else ops.split_bf16x2)(wt)
    if c["a2"]:
        kw["a2"] = view(T(r["a2"].reshape(-1), dev), cin)
    if c["affine"]:
        kw.update(scale=T(r["scale"], dev), shift=T(r["shift"], dev))
    if c["row_period"]:
        kw["row_scale"] = T(r["row_scale"], dev)
    for key, name, ld in (("r1", "res1", L["ldr1"]), ("r2", "res2", L["ldr2"])):
        if r[key] is not None:
            kw[name] = view(_rows(r[key], ld, 0, m * ld, dev, bf16=c[name] == "bf16"), ld)
    if c["ws"]:
        kw["workspace"] = torch.full((1 << 20,), float("nan"), device=dev)
    if c["cnt"]:
        kw["counters"] = torch.zeros(1024, dtype=torch.int32, device=dev)
    if c["c_bf16"]:
        out = torch.full((L["c_numel"],), BF16_NAN, dtype=torch.int16, device=dev)
    else:
        out = torch.full((L["c_numel"],), float("nan"), device=dev)
    with R.overrides(c["ov"]):
        d, hook = ops.conv_desc(x, n, h, w, cin, wt, cout, k, st, pad, view(out, L["ldc"], L["c_off"]), act=c["act"],
                                rows_per_group=L["rpg"], group_stride=L["gstride"], **kw)
        key, splits2 = R.plan_of(d)
        assert key == c["want"] and key == key0 and splits2 == splits, (c["id"], key, key0, c["want"])
        ops.conv_launch(d, hook)
    LAUNCHES["n"] += 1
    if c["cnt"]:
        assert int(kw["counters"].abs().sum()) == 0, f"{c['id']}: split-K arrival counters not left at zero"
    o = out.cpu().numpy()
    written = np.zeros(o.shape, bool)
    rows = np.arange(m)
    base = (rows // L["rpg"]) * L["gstride"] + (rows % L["rpg"]) * L["ldc"] if L["rpg"] else rows * L["ldc"]
    idx = L["c_off"] + base[:, None] + np.arange(cout)[None, :]
    written[idx] = True
    if c["c_bf16"]:
        bits = o.view(np.uint16)
        assert (bits[~written] == BF16_NAN).all(), f"{c['id']}: a guard element was overwritten"
        return key, splits, R.bf16_val(bits[idx]), bits[idx], r
    assert np.isnan(o[~written]).all(), f"{c['id']}: a guard element was overwritten"
    return key, splits, o[idx], None, r


_MATRIX = R.matrix()


@pytest.mark.parametrize("want,production,cases", _MATRIX,
                         ids=["-".join(map(str, w)) + ("-prod" if p else "") for w, p, _ in _MATRIX])
def test_instance_matches_fp64(dev, want, production, cases):
    """Every case of one target tuple runs exactly that instance; probe / ints outputs equal the fp64 operand model
    bit for bit, every range element is inside its derived bound, guards stay NaN, counters return to zero."""
    fails, worst = [], 0.0
    for c in cases:
        key, splits, got, bits, r = run_case(c, dev)
        bad, w, msg = R.compare(c, r, got, bits)
        if c["fam"] == "range":
            worst = max(worst, w)
            k2 = (c["mode"], want[6])
            WORST[k2] = max(WORST.get(k2, 0.0), w)
        if bad:
            fails.append(msg)
    print(f"{want}: {len(cases)} cases, worst range err / bound {worst:.3f}, {len(fails)} failed")
    assert not fails, (len(fails), fails[:5])
