"""CPU: the GPU entropy decode of baseline JPEGs (spotter_amd/csrc/jpeg_entropy.hip) without a GPU.

The kernels' per-subsequence code lives in csrc/jpeg_entropy_core.h, which also compiles as host C++;
sp_jpeg_entropy_emulate (csrc/jpeg_entropy_host.h) runs the kernels' passes in their order over it: the
speculative decode, the in-workgroup and cross-workgroup synchronisation rounds with the kernels' budget, the
prefix sum, the write pass, the DC pass. Checked here:

1. the emulation's coefficients equal the host decoder's (sp_jpeg_decode_coefs) for the inputs of
   tests/jpeg_entropy_cases.py and for every eligible file of tests/jpeg_corpus.py that the host accepts;
2. the round budget: every non-degenerate input reaches status 0 within it (the most rounds seen: DESIGN §5.21);
3. every file of the corrupt corpus, and of a set of eligible files with 1..48 extra bytes before EOI or before a
   restart marker, is "not eligible", or has a non-zero status word, or decodes to the host's coefficients — and
   never decodes with status 0 where the host parser refuses the file;
4. packer + emulation built with AddressSanitizer + UBSan (tools/sanitize/jpeg_entropy_fuzz.cpp, a stand-alone
   program) run the corpus with no report;
5. SPOTTER_JPEG_ENTROPY parsing, the "host" default, the ctypes mirror of sp_jpeg_scan.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from jpeg_corpus import corpus, pack  # noqa: E402
from jpeg_entropy_cases import cases, non_eligible, resistant, tail_junk  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tools", "sanitize", "jpeg_entropy_fuzz.cpp")
# the budget the kernels run with (csrc/jpeg_entropy_core.h): kLaunches = 3 launches, i.e. 2 cross-workgroup
# rounds after the speculative one, of at most kBlock = 256 in-workgroup rounds each. 256 rounds of 256 threads is
# full serial propagation through a workgroup: a count near it means the stream hardly fell into step by itself.
CROSS_ROUNDS, INNER_ROUNDS = 2, 256


@pytest.fixture(scope="module")
def entries():
    return corpus()


@pytest.fixture(scope="module")
def emulated():
    """name → (data, host coefficients, emulation result) for the non-degenerate inputs, computed once."""
    from spotter_amd.jpeg import decode_coefs, emulate_entropy

    return {name: (data, decode_coefs(data)[1], emulate_entropy(data)) for name, data in cases()}


def test_inputs_cover_the_paths():
    """The input list holds what it is meant to hold: a stream shorter than one subsequence, single-workgroup and
    multi-workgroup streams, restart segments of one MCU, gray."""
    from spotter_amd.jpeg import pack_scan

    scans = {name: pack_scan(data)[1] for name, data in cases()}
    assert scans["shorter than a subsequence"].stream_bits < scans["shorter than a subsequence"].sub_bits
    assert scans["shorter than a subsequence"].nsub == 1
    assert 1 < scans["17x33 sub2"].nsub <= 256  # one workgroup
    assert scans["480x640 sub0"].nsub > 4 * 256  # several workgroups: the cross-workgroup rounds matter
    assert scans["restart 1 mcu"].restart_interval == 1 and scans["restart 1 mcu"].nseg == scans["restart 1 mcu"].nmcu
    assert scans["restart rows"].nseg > 1 and scans["restart rows"].restart_interval == scans["restart rows"].mcux
    assert scans["gray"].ncomp == 1 and scans["gray"].bpm == 1
    assert {scans[f"233x177 sub{s}"].bpm for s in (0, 1, 2)} == {3, 4, 6}


def test_emulation_equals_the_host_decoder(emulated):
    assert len(emulated) >= 25
    for name, (data, ref, got) in emulated.items():
        assert got is not None, f"{name}: not eligible"
        lay, co, status, rounds = got
        assert status == 0, (name, status)
        bad = np.argwhere(co != ref)
        assert bad.size == 0, f"{name}: {len(bad)} coefficients differ, first at {bad[:3].tolist()}"


def test_round_budget_reaches_every_non_degenerate_input(emulated):
    """A condition on the budget, not a measurement: status 0 for every input; the last launch only confirms (no
    exit changes in it); and every in-workgroup loop ends by its vote, not by its cap (the emulation reports 256
    for a loop the cap cut)."""
    worst = [0, 0]
    for name, (data, ref, got) in emulated.items():
        lay, co, status, (cross, inner) = got
        print(f"{name}: cross-workgroup rounds {cross}, in-workgroup rounds {inner}")
        assert status == 0, (name, status)
        assert cross < CROSS_ROUNDS and inner < INNER_ROUNDS, (name, cross, inner)
        worst = [max(worst[0], cross), max(worst[1], inner)]
    print("largest:", worst)


def test_sync_resistant_and_non_eligible_files():
    """Flat and periodic frames: whatever the status, a zero status means the host's coefficients. Progressive
    (multi-scan) files are not eligible."""
    from spotter_amd.jpeg import decode_coefs, emulate_entropy

    for name, data in resistant():
        lay, co, status, rounds = emulate_entropy(data)
        print(f"{name}: status {status}, rounds {rounds}")
        if status == 0:
            assert np.array_equal(co, decode_coefs(data)[1]), name
    for name, data in non_eligible():
        assert emulate_entropy(data) is None, name


def test_corpus_three_way_rule(entries):
    """Every corpus file: not eligible, or status non-zero, or the host's coefficients. The eligible files the
    host accepts give the host's coefficients whatever the status; a file the host refuses never comes back with
    status 0 (the GPU path would show pixels where the host path raises)."""
    from spotter_amd.jpeg import UnsupportedJpeg, decode_coefs, emulate_entropy

    n_eq = n_status = n_not = n_refused = 0
    for lab, data in list(entries) + list(tail_junk()):
        try:
            ref = decode_coefs(data)[1]
        except UnsupportedJpeg:
            ref = None
        try:
            got = emulate_entropy(data)
        except UnsupportedJpeg:
            assert ref is None, lab  # the packer's parser refuses exactly what the host's refuses
            n_refused += 1
            continue
        if got is None:
            n_not += 1
            continue
        lay, co, status, rounds = got
        if ref is None:
            assert status != 0, lab
            n_status += 1
            continue
        assert np.array_equal(co, ref), lab
        if lab.split(":")[1] in ("valid", "com_segment", "fill_between", "after_eoi", "double_eoi") or \
                lab.split(":")[1].endswith("_fill"):
            assert status == 0, (lab, status)  # well-formed files stay on the GPU path
        n_eq += status == 0
        n_status += status != 0
    print(n_eq, n_status, n_not, n_refused)
    assert n_eq >= 100 and n_status >= 30 and n_not >= 100 and n_refused >= 100


def test_extra_bytes_after_the_last_block_are_never_accepted():
    """Bytes between a segment's last block and its marker: 8 zero bytes before EOI of a 24x24 gray file begin a
    block that the segment's end cuts short — no bad code, no overrun, the block count right. The host decoder
    refuses the file (extraneous data before a marker), so the status must be non-zero; and so for every file of
    the set, whether the host's reader happens to see the bytes or not."""
    from spotter_amd.jpeg import UnsupportedJpeg, decode_coefs, emulate_entropy

    files = dict(tail_junk())
    with pytest.raises(UnsupportedJpeg):
        decode_coefs(files["gray 24x24:8x00_before_eoi"])
    refused = 0
    for lab, data in files.items():
        got = emulate_entropy(data)
        assert got is not None and got[2] != 0, (lab, got and got[2])
        try:
            decode_coefs(data)
        except UnsupportedJpeg:
            refused += 1
    assert len(files) >= 300 and refused >= 200, (len(files), refused)


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_packer_and_emulation_are_sanitizer_clean(entries, tmp_path):
    exe = tmp_path / "jpeg_entropy_fuzz"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", HARNESS, "-o", str(exe)], check=True, timeout=300)
    blob = tmp_path / "corpus.bin"
    good = [(name, data) for name, data in cases() if len(data) < 40000]
    junk = list(tail_junk())
    blob.write_bytes(pack(list(entries) + good + junk + list(resistant())))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe), str(blob)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
    rows = [ln.split() for ln in r.stdout.strip().split("\n")]
    assert len(rows) == len(entries) + len(good) + len(junk) + len(resistant())
    for (lab, _), row in zip(list(entries) + good + junk, rows):
        idx, rc, status, hrc, eq = row
        if rc == "big":
            continue
        assert rc in ("0", "1", "-10"), (lab, row)
        if rc == "0":  # packed: a zero status needs the host's acceptance and its coefficients
            assert status != "0" or (hrc == "0" and eq == "1"), (lab, row)
            assert eq != "0", (lab, row)
    for (lab, _), row in zip(good, rows[len(entries):]):
        assert row[1:] == ["0", "0", "0", "1"], (lab, row)


def test_entropy_mode_parsing_and_default(monkeypatch):
    import inspect

    from spotter_amd import config, jpeg

    assert config.jpeg_entropy_from_env({}) == "host"
    assert config.jpeg_entropy_from_env({"SPOTTER_JPEG_ENTROPY": ""}) == "host"
    assert config.jpeg_entropy_from_env({"SPOTTER_JPEG_ENTROPY": " GPU "}) == "gpu"
    assert config.jpeg_entropy_from_env({"SPOTTER_JPEG_ENTROPY": "auto"}) == "auto"
    for bad in ("cpu", "1", "gpu,host"):
        with pytest.raises(ValueError, match="SPOTTER_JPEG_ENTROPY"):
            config.jpeg_entropy_from_env({"SPOTTER_JPEG_ENTROPY": bad})
    monkeypatch.delenv("SPOTTER_JPEG_ENTROPY", raising=False)
    assert jpeg.image_module()._spotter_entropy == "host"
    monkeypatch.setenv("SPOTTER_JPEG_ENTROPY", "gpu")
    assert jpeg.image_module()._spotter_entropy == "gpu"
    monkeypatch.setattr(jpeg, "_env_entropy", None)
    assert jpeg.default_entropy() == "gpu"
    monkeypatch.setenv("SPOTTER_JPEG_ENTROPY", "fast")
    assert jpeg.default_entropy() == "gpu"  # read once per process: no per-request look at the environment
    with pytest.raises(ValueError, match="SPOTTER_JPEG_ENTROPY"):  # what fails the import of the drop-in serve.py
        jpeg.image_module()
    assert inspect.signature(jpeg.decoder).parameters["entropy"].default == "host"  # decoder() reads no environment
    assert inspect.signature(jpeg.JpegDecoder.__init__).parameters["entropy"].default == "host"
    with pytest.raises(ValueError):
        config.check_jpeg_entropy("device")


def test_scan_struct_mirror_matches_the_header(tmp_path):
    import ctypes

    from spotter_amd import _lib

    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "spotter_hip.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(sp_jpeg_scan));']
    for f, _ in _lib.SpJpegScan._fields_:
        lines.append(f'  printf("{f} %zu\\n", offsetof(sp_jpeg_scan, {f}));')
    lines.append("  return 0;\n}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    assert int(got["sizeof"]) == ctypes.sizeof(_lib.SpJpegScan)
    for f, _ in _lib.SpJpegScan._fields_:
        assert int(got[f]) == getattr(_lib.SpJpegScan, f).offset, f
    assert {"sp_jpeg_entropy_pack", "sp_jpeg_entropy_decode", "sp_jpeg_entropy_emulate"} <= set(_lib.EXPORTS)
