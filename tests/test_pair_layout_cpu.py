"""The T2 ("combo") layout of mfcc_pair_kernel as tools/pair_model.py specifies it: the lane-level
numpy model reproduces numpy.fft's power spectra of both frames for every bin, every lane runs
the same 16 stores (lane-uniform immediates on at most five per-lane bases), the stores and loads
are bank-conflict-free in tools/pair_lds_model.py's terms, and the kernel source carries the
model's constants.  DESIGN.md Kernel 1a "One T2 store sequence"."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pair_lds_model as M  # noqa: E402
import pair_model as PM  # noqa: E402

N = np.arange(1024)


def _tone(k, phase=0.3):
    return np.cos(2 * np.pi * k * N / 1024 + phase)


def _inputs():
    rng = np.random.default_rng(7)
    imp = np.zeros(1024)
    imp[0] = 1.0
    late = np.zeros(1024)
    late[777] = -2.0
    out = [("noise", rng.standard_normal(1024), rng.standard_normal(1024)), ("impulse", imp, late)]
    # tones on the bins the k1 & 7 == 0 lanes carry (residues 0, 8, 16, ... and the self-paired 0 / 64 / 512)
    for k in (0, 8, 16, 64, 120, 128, 192, 256, 320, 384, 448, 512):
        out.append((f"tone{k}", _tone(k), 0.5 * _tone((k + 64) % 513, 1.1)))
    return out


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("name,x0,x1", _inputs(), ids=[i[0] for i in _inputs()])
def test_model_reproduces_both_power_spectra(name, x0, x1, f64):
    P0, P1 = PM.model(x0, x1, f64)
    assert P0.shape == P1.shape == (513,) and not np.isnan(P0).any() and not np.isnan(P1).any()
    for P, x in ((P0, x0), (P1, x1)):
        R = np.abs(np.fft.rfft(x)) ** 2
        # float64 arithmetic on both sides: 1024-point transforms agree to ~1e-13 of the peak
        assert np.max(np.abs(P - R)) <= 1e-11 * R.max(), name


def _targets(f64):
    """[lane][h][c] -> complex index the readers expect: register 8 h + c of lane b0 + 8 kl is the
    value (k1 = kl + 8 h, c0 = c, b0), residue r = k1 + 16 c0, in the slot of the lane holding r"""
    rA, rB = PM.residues()
    where = {}
    for lane in range(64):
        where[int(rA[lane])] = (lane, 0)
        where[int(rB[lane])] = (lane, 1)
    assert sorted(where) == list(range(128))
    t = np.empty((64, 2, 8), int)
    for lane in range(64):
        b0, kl = lane & 7, lane >> 3
        for h in range(2):
            for c in range(8):
                rl, slot = where[kl + 8 * h + 16 * c]
                t[lane, h, c] = PM.row_stride(f64) * b0 + PM.col(rl) + 64 * slot
    return t


@pytest.mark.parametrize("f64", [False, True])
def test_sixteen_stores_have_lane_uniform_immediates(f64):
    t, base = _targets(f64), PM.store_bases(f64)
    assert base.shape == (64, 5)
    for h in range(2):
        for c in range(8):
            imm = t[:, h, c] - base[:, PM.store_reg(h, c)]
            assert len(set(imm.tolist())) == 1, (h, c)
            assert int(imm[0]) == PM.store_imm(h, c) and 0 <= imm[0] * 16 < 65536   # a DS offset field
    # lanes with k1 & 7 != 0 hold one value per h; only lanes 0-7 need all five bases
    assert all(len(set(base[lane, :2])) == 1 and len(set(base[lane, 2:])) == 1 for lane in range(8, 64))
    # the buffer fits the wave's region (64 x 17 complex) and is written exactly once per pair
    flat = t.reshape(-1)
    assert len(set(flat.tolist())) == 1024 and flat.max() < 64 * 17


@pytest.mark.parametrize("f64", [False, True])
def test_t2_is_bank_conflict_free(f64):
    CB = 16 if f64 else 8
    t = _targets(f64)
    for h in range(2):
        for c in range(8):
            assert M.extra("write_b128" if f64 else "write_b64", [CB * int(a) for a in t[:, h, c]]) == 0
    RS = PM.row_stride(f64)
    for j in range(16):
        a = [CB * (PM.col(l) + 64 * (j >> 3) + RS * (j & 7)) for l in range(64)]
        assert M.extra("read_b128" if f64 else "read_b64", a) == 0
        if not f64:
            assert M.extra("_r2", a) == 0          # one access of a ds_read2*_b64


def test_kernel_source_carries_the_model_constants():
    src = open(os.path.join(ROOT, "sonido-sonar_amd", "csrc", "mfcc_pair.hip")).read()
    m = re.search(r"kT2Irr\[5\] = \{([0-9, ]+)\}", src)
    assert m and tuple(int(v) for v in m.group(1).split(",")) == PM.IRR
    assert re.search(r"sizeof\(T\) == 8 \? %d : %d" % (PM.row_stride(True), PM.row_stride(False)), src)
    assert "kT2Irreg" not in src
    assert [c if c < 5 else 12 - c for c in range(8)] == list(PM.PI)
    assert [(c & 4) | ((c + 1) & 3) for c in range(8)] == list(PM.XI)
    assert "c < 5 ? c : 12 - c" in src and "(c & 4) | ((c + 1) & 3)" in src
