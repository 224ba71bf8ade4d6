"""The batch-invariant mode without a GPU: the planner under sp_set_plan_batch, its error paths, and the host
plumbing of the setting (environment variable, pickling, the shared-batch handshake).

The planner half replays tests/golden/conv_plan.jsonl.gz (the 6 296 recorded plans test_host.py replays at their own
size) with every descriptor's leading dimension scaled by f and sp_set_plan_batch(f, 1): the plan must be the
recorded one in every field that decides arithmetic. Fields compared: family, tile, planes, generic, a_bf16, splits,
and fast_1x1 wherever the scaled launch is inside the fast path's own 32-bit addressing limit (M·lda·4 < 2^32:
include/spotter_hip.h declares the field an addressing limit of the launch at hand, its alternatives bit-identical;
past the limit the test asserts the planner left the fast path). Left out: epilogue and counters, which the header
declares bit-identical.
"""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
import pickle
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import conv_refs as R  # noqa: E402
import wino_refs as W  # noqa: E402
from test_shared_batch import call, check_rows, image, models, owner, sockdir  # noqa: E402,F401 (the stub fixtures)

ROOT = R.ROOT
FACTORS = (2, 3, 5, 8, 32)
ARITH = ("family", "tile", "planes", "generic", "a_bf16", "splits")
DEFAULTS = [-1, -1, 0, 0, -1]


@pytest.fixture(scope="module")
def L():
    from spotter_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def fixture_lines():
    from spotter_amd import _lib

    with gzip.open(os.path.join(ROOT, "tests", "golden", "conv_plan.jsonl.gz"), "rt") as f:
        head, *lines = [json.loads(ln) for ln in f]
    names = [f for f, _ in _lib.SpConvDesc._fields_]
    assert head["fields"] == names and len(lines) == 6296  # every record of the fixture (6 297 lines with its head)
    out, kw = [], None
    for enc, o, want in lines:
        if enc != 0:
            kw = {names[int(k)]: v for k, v in enc.items()}
        out.append((kw, o + DEFAULTS[len(o):], want))
    return out


@pytest.fixture(autouse=True)
def _reset(L):
    yield
    L.sp_set_plan_batch(0, 0)
    L.sp_set_conv_config(-1)
    L.sp_set_splitk_config(-1, 0, 0)
    L.sp_set_tuning(3, -1)


def scaled(kw, f):
    """The descriptor with f times the rows: W (and Wo) of an H = 1 linear, N of everything else; the workspace with it."""
    kw = dict(kw)
    if kw.get("N") == 1 and kw.get("H") == 1 and kw.get("KH") == 1 and kw.get("KW") == 1 and kw.get("stride") == 1:
        kw["W"] *= f
        kw["Wo"] = kw.get("Wo", 0) * f
    else:
        kw["N"] = kw.get("N", 0) * f
    if "workspace_elems" in kw:
        kw["workspace_elems"] *= f
    return kw


def plan(L, kw, o):
    from spotter_amd import _lib

    L.sp_set_conv_config(o[0])
    L.sp_set_splitk_config(o[1], o[2], o[3])
    L.sp_set_tuning(3, o[4])
    info = _lib.SpConvPlanInfo()
    rc = L.sp_conv_plan(C.byref(_lib.SpConvDesc(**kw)), C.byref(info))
    return {f: getattr(info, f) for f, _ in info._fields_} if rc == 0 else L.sp_last_error().decode()


def fast_addressable(kw):
    """conv_plan.h t1_ok's limits on the launch's own rows."""
    m = kw["N"] * kw["Ho"] * kw["Wo"]
    k = kw["KH"] * kw["KW"] * kw["Cin"]
    return m * kw["lda"] * (2 if kw.get("A_bf16") else 4) < 1 << 32 and kw["Cout"] * k * 2 < 1 << 32


@pytest.mark.parametrize("f", FACTORS)
def test_fixture_plans_are_the_recorded_ones_at_every_batch(L, fixture_lines, f):
    fields = [n for n, _ in __import__("spotter_amd._lib", fromlist=["x"]).SpConvPlanInfo._fields_]
    bad, past_limit = [], 0
    for i, (kw, o, want) in enumerate(fixture_lines):
        L.sp_set_plan_batch(f, 1)
        skw = scaled(kw, f)
        got = plan(L, skw, o)
        if isinstance(want, str) or isinstance(got, str):
            if got != want:  # the recorded refusals keep their text
                bad.append((i + 2, "error", want, got))
            continue
        want = dict(zip(fields, want))
        for n in ARITH:
            if got[n] != want[n]:
                bad.append((i + 2, n, want, got))
        if fast_addressable(skw):
            if got["fast_1x1"] != want["fast_1x1"]:
                bad.append((i + 2, "fast_1x1", want, got))
        else:
            past_limit += 1
            if got["fast_1x1"] != 0:
                bad.append((i + 2, "fast_1x1 past the 32-bit limit", want, got))
    print(f"\nf={f}: {len(fixture_lines)} records, {past_limit} past the fast path's addressing limit")
    assert not bad, (len(bad), bad[:5])


def test_reset_restores_todays_plans(L, fixture_lines):
    fields = [n for n, _ in __import__("spotter_amd._lib", fromlist=["x"]).SpConvPlanInfo._fields_]
    L.sp_set_plan_batch(7, 2)
    assert L.sp_set_plan_batch(0, 0) == 0
    bad = []
    for i, (kw, o, want) in enumerate(fixture_lines):
        got = plan(L, kw, o)
        got = got if isinstance(got, str) else [got[n] for n in fields]
        if got != want:
            bad.append((i + 2, want, got))
    assert not bad, (len(bad), bad[:5])


def _first_of(fixture_lines, pred):
    return [(kw, o, want) for kw, o, want in fixture_lines if not isinstance(want, str) and o[0] == o[1] == -1 and pred(kw, want)]


def test_without_the_setting_the_plan_moves_with_the_batch(L, fixture_lines):
    """The precondition: for the recorded split-K launches, and for the by-shape bf16-row and split-operand launches
    of under 192 tiles, f = 32 times the rows changes the default plan (so the test above is not vacuous)."""
    fields = [n for n, _ in __import__("spotter_amd._lib", fromlist=["x"]).SpConvPlanInfo._fields_]
    split = _first_of(fixture_lines, lambda kw, w: w[fields.index("splits")] > 1 and kw.get("workspace_elems", 0) > 1 << 30
                     and (kw["Cin"], kw["Cout"], kw["KH"]) == (1024, 256, 1))  # the subset: the split 1024 → 256 linears
    assert len(split) >= 10
    for kw, o, want in split:
        got = plan(L, scaled(kw, 32), o)
        assert got["splits"] < want[fields.index("splits")], (kw, want, got)
        L.sp_set_plan_batch(32, 1)
        assert plan(L, scaled(kw, 32), o)["splits"] == want[fields.index("splits")]
        L.sp_set_plan_batch(0, 0)
    # a tile id that changes: 200 rows of 256 → 256 on bf16 rows run the 64×64 tile, 6 400 rows do not
    kw = R_desc(1, 1, 200, 256, 256, 1, A_bf16=True, C_bf16=True)
    small, big = plan(L, kw, DEFAULTS), plan(L, scaled(kw, 32), DEFAULTS)
    assert small["tile"] != big["tile"], (small, big)
    L.sp_set_plan_batch(32, 1)
    assert plan(L, scaled(kw, 32), DEFAULTS)["tile"] == small["tile"]


def R_desc(n, h, w, cin, cout, k, planes=1, **kw):
    """tools/gen_conv_plan_golden.py's `desc` on the same fake pointers."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_conv_plan_golden as G

    return G.desc(n, h, w, cin, cout, k, 1, planes, **{f: (True if v is True else v) for f, v in kw.items()})


def test_rows_that_are_no_multiple_of_the_batch_are_refused(L):
    kw = R_desc(3, 5, 7, 64, 64, 3, planes=3)
    L.sp_set_plan_batch(2, 1)
    got = plan(L, kw, DEFAULTS)
    assert isinstance(got, str) and "no multiple of the batch 2" in got, got
    assert L.sp_set_plan_batch(3, 1) == 0 and not isinstance(plan(L, kw, DEFAULTS), str)
    assert L.sp_set_plan_batch(-1, 1) < 0 and b"sp_set_plan_batch" in L.sp_last_error()
    assert L.sp_set_plan_batch(2, 0) < 0
    # the Winograd stages count tiles
    c = W._case("path", "range", 4, "x3", (3, 4, 4, 32, 4))  # 3 tiles
    L.sp_set_plan_batch(2, 1)
    with pytest.raises(Exception, match="no multiple of the batch 2"):
        W.plan_of(W.fake_desc(c), 4)


def test_a_short_workspace_is_an_error_not_a_smaller_split(L):
    """300 rows, K = 1024 → 256 splits 4-way. With a workspace for the 300 rows of one image only, a launch of 8
    images planned as one image is refused; without the setting the same descriptor silently runs unsplit."""
    one = R_desc(1, 1, 300, 1024, 256, 1, planes=3, workspace=True, workspace_elems=4 * 300 * 256)
    assert plan(L, one, DEFAULTS)["splits"] == 4
    eight = dict(one, W=2400, Wo=2400)
    assert plan(L, eight, DEFAULTS)["splits"] == 1
    L.sp_set_plan_batch(8, 1)
    got = plan(L, eight, DEFAULTS)
    assert isinstance(got, str) and "workspace" in got and "4-way" in got, got
    assert plan(L, dict(eight, workspace_elems=8 * 4 * 300 * 256), DEFAULTS)["splits"] == 4
    # a counters array too short for the launch's tiles changes no arithmetic (the reduce launch sums the same
    # slabs in the same order): no error, the same factor
    cnt = dict(eight, workspace_elems=1 << 40, splitk_counters=0x30000, splitk_counters_len=1)
    got = plan(L, cnt, DEFAULTS)
    assert got["splits"] == 4 and got["counters"] == 0


@pytest.mark.parametrize("f", FACTORS)
def test_winograd_plans_are_the_one_image_plans_at_every_batch(L, f):
    launches = json.load(open(os.path.join(ROOT, "tests", "golden", "wino_launches.json")))["launches"]
    assert launches
    moved = 0
    for wm, n, h, w, cin, cout, mode in launches:
        L.sp_set_plan_batch(0, 0)
        base = W.plan_of(W.fake_desc(W._case("path", "range", wm, mode, (n, h, w, cin, cout))), wm)
        big = W.fake_desc(W._case("path", "range", wm, mode, (n * f, h, w, cin, cout)))
        if big.N * -(-h // wm) * -(-w // wm) * cin * (wm + 2) ** 2 * 4 >= 1 << 32:
            continue  # past the component GEMM's 32-bit addressing: another, bit-identical, form (see above)
        default = W.plan_of(big, wm)
        L.sp_set_plan_batch(n * f, n)
        got = W.plan_of(big, wm)
        assert got[2] == base[2] * f  # the tiles are the launch's own
        assert (got[0], got[1], got[3], got[4]) == (base[0], base[1], base[3], base[4]), (wm, n, h, w, cin, cout, mode)
        moved += (default[0], default[3]) != (base[0], base[3])
    assert f < 8 or moved  # at 8 and 32 times the rows some default Winograd plan does move


# ------------------------------------------------------------------------------------------------ host plumbing
def test_the_environment_variable_is_parsed_and_refused_when_malformed(monkeypatch):
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRESETS, batch_invariant_from_env, check_batch_invariant

    for raw, want in ((None, None), ("", None), ("0", None), ("off", None), ("1", 1), (" 8 ", 8)):
        assert batch_invariant_from_env({} if raw is None else {"SPOTTER_BATCH_INVARIANT": raw}) == want
    for raw in ("-1", "1.5", "yes", "4x", "٣"):
        with pytest.raises(ValueError, match="SPOTTER_BATCH_INVARIANT"):
            batch_invariant_from_env({"SPOTTER_BATCH_INVARIANT": raw})
    for bad in (0, -2, True, 1.0, "1"):
        with pytest.raises(ValueError, match="batch_invariant"):
            check_batch_invariant(bad)
    monkeypatch.delenv("SPOTTER_BATCH_INVARIANT", raising=False)
    assert SpotterForObjectDetection.from_pretrained("synthetic:r18vd").batch_invariant is None
    monkeypatch.setenv("SPOTTER_BATCH_INVARIANT", "4")
    assert SpotterForObjectDetection.from_pretrained("synthetic:r18vd").batch_invariant == 4
    assert SpotterForObjectDetection.from_pretrained("synthetic:r18vd", batch_invariant=None).batch_invariant is None
    assert SpotterForObjectDetection(PRESETS["r18vd"]).batch_invariant is None  # the constructor reads no environment
    monkeypatch.setenv("SPOTTER_BATCH_INVARIANT", "many")
    with pytest.raises(ValueError, match="SPOTTER_BATCH_INVARIANT"):
        SpotterForObjectDetection.from_pretrained("synthetic:r18vd")
    with pytest.raises(ValueError, match="batch_invariant"):
        SpotterForObjectDetection(PRESETS["r18vd"], batch_invariant=0)


def test_the_setting_survives_a_pickle_round_trip():
    from spotter_amd import SpotterForObjectDetection
    from spotter_amd.config import PRESETS

    m = pickle.loads(pickle.dumps(SpotterForObjectDetection(PRESETS["r18vd"], precision="bf16", batch_invariant=4)))
    assert m.batch_invariant == 4 and m.precision == "bf16" and m._engine is None
    assert pickle.loads(pickle.dumps(SpotterForObjectDetection(PRESETS["r18vd"]))).batch_invariant is None


def test_an_owner_refuses_a_replica_with_another_setting(owner, models):  # noqa: F811
    o = owner("--batch-invariant", "4")
    with pytest.raises(ValueError, match="batch_invariant differs"):
        call(models(), image(0, 0))
    with pytest.raises(ValueError, match="batch_invariant differs"):
        call(models(batch_invariant=1), image(0, 0))
    check_rows(call(models(batch_invariant=4), image(0, 2)), image(0, 2))  # a matching replica is served
    assert o.stats()["images"] == 1


def test_a_replica_starts_its_owner_with_its_own_setting(models):  # noqa: F811
    m = models(batch_invariant=2)
    m._name = "synthetic:r18vd"
    check_rows(call(m, image(1, 0)), image(1, 0))  # spawns the stub owner with --batch-invariant 2
    with pytest.raises(ValueError, match="batch_invariant differs"):
        call(models(), image(1, 1))
