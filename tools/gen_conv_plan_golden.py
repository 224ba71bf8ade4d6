"""Records tests/golden/conv_plan.jsonl.gz (gzip of the JSON lines below): which kernel instantiation sp_conv2d picks for a list of descriptors.

    SPOTTER_HIP_LIB=<recorder library> python tools/gen_conv_plan_golden.py <parent commit hash>

The fixture characterises the dispatch of the commit BEFORE the planner (csrc/conv_plan.hip) existed, so it is
taken from a recorder build of that parent commit, never from the code under test: a library in which every
hipLaunchKernelGGL site of the conv path fills sp_conv_plan_info from the template arguments it selected and
returns before launching, exported under sp_conv_plan's signature. tests/test_host.py replays every line against
the planner. No GPU is needed: descriptor pointers are fake addresses chosen for their alignment.

Line 1: {"parent": hash, "fields": sp_conv_desc field names}. Every other line is one case
[desc, overrides, result]: desc maps a field's index to its non-zero value (0 = the previous line's descriptor);
overrides are [forced cfg, split-K cfg, max_splits, min_ktiles, glds-epilogue knob] with trailing defaults
(-1, -1, 0, 0, -1) dropped; result is the nine sp_conv_plan_info fields, or the sp_last_error text.
"""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "conv_plan.jsonl.gz")

# fake addresses: 4 KiB apart, 16-byte aligned unless a case says otherwise
PTR = {f: 0x10000 + 0x1000 * i for i, f in enumerate(
    ["A", "A2", "Wt", "scale", "shift", "row_scale", "res1", "res2", "C", "workspace", "Wt_bf16", "ln_gamma", "ln_beta",
     "A_bf16", "C_bf16", "res1_bf16", "res2_bf16", "splitk_counters"])}
FP32_IDS = [110, 111, 120, 121, 210, 211, 220, 221, 1110, 1111, 1120, 1121, 4110, 4111, 4120, 4121, 4210, 4211]
PREC = {0: 0, 1: 1, 3: 2}  # planes → sp_precision
SPLITK_SHAPES = [(1, 5, 7, 256, 96, 3, 1), (1, 1, 300, 1024, 256, 1, 1), (1, 20, 20, 512, 130, 3, 1),
                 (1, 40, 40, 1024, 256, 1, 1), (1, 40, 40, 256, 256, 3, 1), (1, 12, 12, 512, 202, 3, 1)]
NO_OVERRIDES = (-1, -1, 0, 0, -1)


def glds_ids():
    src = open(os.path.join(ROOT, "spotter_amd", "csrc", "conv_plan.h")).read()
    return sorted(int(m) for m in re.findall(r"^\s*X\((\d+),", src, re.M))


def tile_table():
    src = open(os.path.join(ROOT, "spotter_amd", "csrc", "tile_table.h")).read()
    return [tuple(map(int, m)) for m in re.findall(r"\{(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (-?\d+)\},", src) if int(m[0])]


def desc(n, h, w, cin, cout, k, stride, planes, pad=None, **kw):
    """A valid dense descriptor on fake pointers; kw overrides fields (a pointer field given as True takes its fake
    address, "A_bf16" replaces A)."""
    pad = k // 2 if pad is None else pad
    K = k * k * cin
    d = dict(A=PTR["A"], lda=cin, N=n, H=h, W=w, Cin=cin, KH=k, KW=k, stride=stride, pad=pad,
             Ho=(h + 2 * pad - k) // stride + 1, Wo=(w + 2 * pad - k) // stride + 1, Wt=PTR["Wt"], Cout=cout,
             C=PTR["C"], ldc=cout, precision=PREC[planes])
    if planes:
        d.update(Wt_bf16=PTR["Wt_bf16"], wt_plane_stride=(cout * K + 7) // 8 * 8 if planes == 3 else 0)
    for f, v in kw.items():
        d[f] = PTR[f] if v is True else v
    if d.get("A_bf16"):
        d["A"] = 0
    if d.get("C_bf16"):
        d["C"] = 0
    for f, ld in (("res1", "ldr1"), ("res1_bf16", "ldr1"), ("res2", "ldr2"), ("res2_bf16", "ldr2"), ("A2", "lda2")):
        if d.get(f):
            d.setdefault(ld, cin if f == "A2" else cout)
    return d


EPI = {"none": {}, "bn": dict(scale=True, shift=True), "bn_res": dict(scale=True, shift=True, res1=True),
       "bf16": dict(scale=True, shift=True, A_bf16=True, C_bf16=True),
       "bf16_res": dict(scale=True, shift=True, A_bf16=True, C_bf16=True, res1_bf16=True)}


def cases():
    out = []
    add = lambda d, o=NO_OVERRIDES: out.append((d, tuple(o)))
    # 1. every tile-table row, as a one-row image whose GEMM has the row's (M, Cout, K)
    for M, cout, K, kh, stride, planes, _cfg in tile_table():
        w = (M - 1) * stride + 1
        for e in ["none", "bn", "bn_res"] + (["bf16", "bf16_res"] if planes == 1 else []):
            add(desc(1, 1, w, K // (kh * kh), cout, kh, stride, planes, **EPI[e]))
    # 2. forced ids on three shapes × operand modes × {plain, A2, bf16 A rows}
    ids = list(range(81)) + [100 + i for i in glds_ids()] + [200 + i for i in glds_ids()] + FP32_IDS + [999]
    shapes = [(2, 11, 9, 64, 136, 3, 1), (4, 16, 16, 1024, 256, 1, 1), (1, 9, 9, 3, 32, 3, 2)]
    for shp in shapes:
        for planes in (0, 1, 3):
            variants = [dict(EPI["bn_res"]), dict(EPI["bn_res"], A2=True)]
            if planes == 1 and shp[3] % 32 == 0:
                variants.append(dict(EPI["bf16_res"]))
            for v in variants:
                for cfg in ids:
                    add(desc(*shp, planes, **v), (cfg, -1, 0, 0, -1))
    # 3. split-K: counters absent / long enough / of length 1, the forced split-K tiles, the cap and the floor
    for shp in SPLITK_SHAPES:
        for planes in (0, 1, 3):
            ws = dict(res1=True, act=1, workspace=True, workspace_elems=1 << 40)
            for cnt in ({}, dict(splitk_counters=True, splitk_counters_len=1 << 20),
                        dict(splitk_counters=True, splitk_counters_len=1)):
                for sk in (-1, 14, 13, 16, 11, 46):
                    for mx in (16, 2):
                        for mn in (8, 64):
                            add(desc(*shp, planes, **ws, **cnt), (-1, sk, mx, mn, -1))
            add(desc(*shp, planes, **dict(ws, workspace_elems=64)))  # too small for any split
            add(desc(*shp, planes, **ws), (14, -1, 0, 0, -1))         # a forced id on a split-K launch
    # 4. alignment and epilogue resolution, on the 1×1 1024 → 256 at M = 1024
    shp = (4, 16, 16, 1024, 256, 1, 1)
    mods = [{}, dict(ldc=258), dict(C=PTR["C"] + 8), dict(wt_plane_stride=256 * 1024 + 4), dict(lda=1026),
            dict(res2=True), dict(row_scale=True, row_period=7), dict(out_rows_per_group=256, out_group_stride=256 * 256 + 64),
            dict(out_rows_per_group=256, out_group_stride=256 * 256 + 2), dict(ldc=525000), dict(lda=1 << 20),
            dict(res1=PTR["res1"] + 8), dict(scale=PTR["scale"] + 4), dict(Wt_bf16=PTR["Wt_bf16"] + 8), dict(Cout=254, ldc=256)]
    for m in mods:
        for planes in (0, 1, 3):
            if "wt_plane_stride" in m and planes != 3:
                continue
            for cfg in (-1, 12, 112, 212, 46, 14, 33):
                for knob in (-1, 4):
                    add(desc(*shp, planes, **dict(EPI["bn_res"], **m)), (cfg, -1, 0, 0, knob))
    for m in mods + [dict(lda=1 << 21), dict(res1_bf16=PTR["res1_bf16"] + 8), dict(ldr1=260), dict(C_bf16=PTR["C_bf16"] + 8)]:
        if set(m) & {"wt_plane_stride", "C", "res1"}:
            continue
        for cfg in (-1, 12, 112, 212, 45, 53):
            add(desc(*shp, 1, **dict(EPI["bf16_res"], **m)), (cfg, -1, 0, 0, -1))
            add(desc(*shp, 1, **dict(EPI["bn_res"], A_bf16=True, **m)), (cfg, -1, 0, 0, -1))  # bf16 A, fp32 C rows
    # 5. errors
    add(desc(4, 16, 16, 256, 256, 1, 1, 0, ln_gamma=True, ln_beta=True, ln_eps=1e-5, res1=True))
    add(desc(4, 16, 16, 256, 200, 1, 1, 0, ln_gamma=True, ln_beta=True, ln_eps=1e-5))
    add(desc(4, 16, 16, 256, 256, 1, 1, 3, ln_gamma=True, ln_beta=True, ln_eps=1e-5))
    for planes in (1, 3):
        for cfg in (14, 46, 44, 35):  # Cin % 32 != 0 (generic gather), also where Cin % 16 == 0 and the tile has k16 stages
            add(desc(2, 8, 8, 48, 64, 1, 1, planes), (cfg, -1, 0, 0, -1))
            add(desc(2, 8, 8, 40, 64, 1, 1, planes), (cfg, -1, 0, 0, -1))
    for cfg in (11, 15, 17, 34, 43, 65, 70, 21, 5, 1110):  # bf16 A rows on ids without a bf16-A form
        add(desc(1, 4, 4, 64, 40, 1, 1, 1, **EPI["bf16"]), (cfg, -1, 0, 0, -1))
    for cfg in (15, 34, 37, 38, 18, 62):  # tiles that do not fit the LDS in one of the operand modes
        for planes in (1, 3):
            add(desc(*shp, planes), (cfg, -1, 0, 0, -1))
    bad = desc(*shp, 3)
    for m in (dict(A=0), dict(Ho=17), dict(lda=8), dict(act=7), dict(precision=5), dict(Wt_bf16=0), dict(wt_plane_stride=8),
              dict(res1=True, res1_bf16=True), dict(C_bf16=True), dict(row_scale=True), dict(KH=0)):
        add(dict(bad, **m))
    add(desc(2, 8, 8, 48, 64, 1, 1, 1, A_bf16=True))
    add(desc(*shp, 1, A_bf16=True, A2=True))
    return out


def main():
    from spotter_amd import _lib

    L = _lib.load()
    names = [f for f, _ in _lib.SpConvDesc._fields_]
    plan_fields = [f for f, _ in _lib.SpConvPlanInfo._fields_]
    lines = [json.dumps({"parent": sys.argv[1], "fields": names}, separators=(",", ":"))]
    prev = None
    for d, o in cases():
        assert set(d) <= set(names), set(d) - set(names)
        L.sp_set_conv_config(o[0])
        L.sp_set_splitk_config(o[1], o[2], o[3])
        L.sp_set_tuning(3, o[4])
        info = _lib.SpConvPlanInfo()
        rc = L.sp_conv_plan(C.byref(_lib.SpConvDesc(**d)), C.byref(info))
        res = [getattr(info, f) for f in plan_fields] if rc == 0 else L.sp_last_error().decode()
        o = list(o)
        while o and o[-1] == NO_OVERRIDES[len(o) - 1]:
            o.pop()
        enc = {str(names.index(f)): v for f, v in d.items() if v}
        lines.append(json.dumps([0 if enc == prev else enc, o, res], separators=(",", ":")))
        prev = enc
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0) as f:  # mtime 0: reproducible bytes
        f.write(("\n".join(lines) + "\n").encode())
    print(f"{len(lines) - 1} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
