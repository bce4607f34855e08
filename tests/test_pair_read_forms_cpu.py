"""The read forms of the float32 mfcc_pair_kernel (DESIGN.md Kernel 1a "Read forms"), held against
the LDS model (tools/pair_lds_model.py): the weight row stride that makes two bins' weights one
conflict-free ds_read_b128, the sixteen single T2 reads, and the LDS cycles per pair that the
MI355X cost table gives for the instructions the loop issues."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_lds_model as M  # noqa: E402


def _table(J):
    """layout-only chunk table (the weight and T2 phases need no filterbank)"""
    ks = [min(512, 8 * l) for l in range(64)]
    src = [[2 * (m + k) for k in range(4)] for m in range(40)]
    return dict(J=J, JS=M.weight_stride(J), JS64=M.weight_stride(J, True), ks=ks, src=src, nf=40, NMP=40, MS=4)


@pytest.mark.parametrize("J", range(1, 17))
def test_weight_stride_rule(J):
    JS = M.weight_stride(J)
    # the smallest stride that holds the chunk (and a zero slot after an odd one) and is 2 mod 4
    want = next(s for s in range(J + (J & 1), 64) if s % 4 == 2)
    assert JS == want and JS >= J + (J & 1)
    # rows of JS (wa, wb) float pairs: 16-byte aligned, lanes an odd number of 16-byte units apart
    assert (8 * JS) % 16 == 0 and (8 * JS // 16) % 2 == 1
    for i in range(0, J - 1, 2):
        assert all(((l * JS + i) * 8) % 16 == 0 for l in range(64))
    # every ds_read_b128 of two bins' weights: no bank conflict in any of its 16-lane groups
    for i in range(0, J - 1, 2):
        assert M.extra("read_b128", [(l * JS + i) * 8 for l in range(64)]) == 0
    # an odd J's last bin is one ds_read_b64 (lanes l and l + 16 share a bank at these strides: one
    # extra cycle per half-wave, in the runtime-J instances only)
    assert M.model(_table(J), False)["fb_weight"] == (2 if J & 1 else 0)
    # float64 keeps the odd stride
    assert M.weight_stride(J, True) == J | 1


def test_weight_stride_values_and_kernel_source():
    got = {J: M.weight_stride(J) for J in range(9, 17)}
    assert got == {9: 10, 10: 10, 11: 14, 12: 14, 13: 14, 14: 14, 15: 18, 16: 18}
    src = open(os.path.join(ROOT, "sonido-sonar_amd", "csrc", "mfcc_pair_layout.h")).read()
    body = re.search(r"constexpr int mfcc_pair_w_stride\(int J, int f64\) \{(.*?)\n\}", src, re.S).group(1)
    assert "return J | 1;" in body and "J + (J & 1)" in body and "(m & 3) == 2 ? m : m + 2" in body


def test_single_t2_reads_conflict_free():
    ph = M.model(_table(12), False)
    assert ph["t2_load"] == 0 and ph["t2_store"] == 0
    # one by one: the 32 columns of each half-wave are distinct mod 32 (8-byte words on 64 banks)
    RS = M.PM.row_stride(False)
    for j in range(16):
        a = [8 * (M.PM.col(l) + 64 * (j >> 3) + RS * (j & 7)) for l in range(64)]
        assert M.extra("read_b64", a) == 0
        for half in (range(32), range(32, 64)):
            assert len({M.PM.col(l) % 32 for l in half}) == 32
        assert max(a) - min(a) < 65536 and 8 * (64 + 7 * RS) < 65536      # one base, 16-bit immediates


@pytest.mark.parametrize("sr,nf,J,JS", [(44100, 40, 12, 14), (44100, 26, 10, 10), (44100, 32, 11, 14),
                                         (44100, 48, 15, 18), (22050, 48, 14, 14)])
def test_gpu_test_banks_cover_the_paths(sr, nf, J, JS):
    """the banks of tests/test_gpu_pair_read_forms.py: compile-time J, even and odd runtime J, each stride"""
    t = M.tables(sr, nf, search=False)
    assert (t["J"], t["JS"]) == (J, JS)


@pytest.fixture(scope="module")
def headline():
    return M.tables(44100, 40)


def test_lds_cycles_headline_bank(headline):
    t = headline
    assert (t["J"], t["JS"], t["JS64"], t["NMP"], t["MS"]) == (12, 14, 13, 40, 8)
    old, new = M.lds_cycles(t, paired_reads=True), M.lds_cycles(t)
    # 8 two-address T2 reads (8 cycles each) -> 16 ds_read_b64 (2); 6 ds_read2_b64 -> 6 ds_read_b128 (4)
    assert old["t2_load"] - new["t2_load"] == 8 * M.COST["read2st64_b64"] - 16 * M.COST["read_b64"] == 32
    assert old["fb_weight"] - new["fb_weight"] == 6 * (M.COST["read2_b64"] - M.COST["read_b128"]) == 24
    assert {k: old[k] - new[k] for k in old if old[k] != new[k]} == {"t2_load": 32, "fb_weight": 24}
    assert sum(old.values()) == 367 and sum(new.values()) == 311
    # the model's conflicts of the as-built forms: none in the two changed phases
    ph = M.model(t, False)
    assert ph["t2_load"] == 0 and ph["fb_weight"] == 0
