"""CPU: the fingerprint host layer's plain-C++ parts under the host compiler.

csrc/fp_layout.h (the LDS carves of fp_wave_kernel and mfcc_pair_kernel) through
tests/c_abi/build/fp_layout_check: the offsets are those of the inline formulas the header replaced, for
W in {128 .. 2048}, both precisions, the SPEC epilogue on and off, banks of 26, 40 and 64 filters, every
pair-kernel J and NMP; a float64 pair bank with J = 16 and NMP = 64 runs 7 waves inside 160 KiB.

csrc/fp_tables.cpp's pair-kernel table builder through tests/c_abi/build/fp_tables_check against its
specification tools/pair_lds_model.py (tables): the same J, row stride, chunk start bins per lane, source
list of every filter and source maximum, for the float32 lane order ("b64") and the float64 one ("b128",
one pad row).  The lane order changes no result bit, so no GPU test sees it."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CABI = os.path.join(ROOT, "tests", "c_abi")
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _build(name):
    subprocess.run(["make", "-s", "-C", CABI, f"build/{name}"], check=True)
    return os.path.join(CABI, "build", name)


def test_fp_lds_layouts():
    run = subprocess.run([_build("fp_layout_check")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "fp_layout ok", run.stdout + run.stderr


def _library_tables(sr, nf):
    """precision -> dict of what fp_tables_check prints for the bank, and the section lines"""
    run = subprocess.run([_build("fp_tables_check"), "pair", str(sr), str(nf)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    t = {"f32": {"src": {}}, "f64": {"src": {}}}
    sections = []
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "section":
            sections.append(w)
        elif w[0] in t and w[1] == "J":
            t[w[0]].update({w[i]: int(w[i + 1]) for i in range(1, len(w), 2)})
        elif w[0] in t and w[1] == "ks":
            t[w[0]]["ks"] = [int(x) for x in w[2:]]
        elif w[0] in t and w[1] == "src":
            t[w[0]]["src"][int(w[2].rstrip(":"))] = [int(x) for x in w[3:]]
    return t, sections


@pytest.mark.parametrize("sr,nf", [(44100, 40), (16000, 26)])
def test_pair_tables_equal_the_lds_model(sr, nf):
    import pair_lds_model as M
    lib, sections = _library_tables(sr, nf)
    assert len(sections) == 15 and all(int(s[3]) % 256 == 0 for s in sections)    # 7 per precision + zeros
    for pr, want in (("f32", M.tables(sr, nf, order_kind="b64")), ("f64", M.tables(sr, nf, order_kind="b128", pad=1))):
        got = lib[pr]
        assert got["n_mels"] == nf and got["NMP"] == want["NMP"]
        assert got["J"] == want["J"]
        assert got["JS"] == (want["JS64"] if pr == "f64" else want["JS"])
        assert len(got["ks"]) == 64 and got["ks"] == want["ks"]
        assert [got["src"][m] for m in range(nf)] == want["src"]
        assert got["max_src"] == want["MS"]
