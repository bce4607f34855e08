"""The LPC formant checker (formant_ref.py) and the shared inputs (formant_cases.py), on the CPU:
the checker equals the oracle on every case, the cases reach the branches they are there for (computed
from the checker alone), few of their frames are undecided, and the checker's own libm envelope lies
inside the admissible error the decided flag and the GPU tests' tolerances are derived from."""
import math

import mpmath
import numpy as np
import pytest

import formant_cases as C
import formant_ref as R


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_checker_equals_oracle(cid):
    """Status, counts, frequencies, bandwidths and `stable` exactly, the record's floats to 1e-9, the
    coefficients within the measured d, which itself must leave the device a bound under 1e-6."""
    ref, o = C.reference(cid), C.oracle_frames(cid)
    sr = C.CASES[cid][1]
    p = C.RATES[sr][1]
    assert R.geometry(sr) == C.RATES[sr]
    assert 0 < len(ref) == len(o["status"]) <= 16
    for i, f in enumerate(ref):
        assert o["status"][i] == f["status"] == 0
        assert o["n_formants"][i] == f["n_formants"] and o["stable"][i] == f["stable"]
        assert np.array_equal(o["frequency"][i], f["frequency"]) and np.array_equal(o["bandwidth"][i], f["bandwidth"])
        for k in ("amplitude", "confidence", "vocal_tract_length", "quality", "gain", "residual_energy"):
            assert np.allclose(o[k][i], f[k], rtol=1e-9, atol=1e-9, equal_nan=True), (i, k)
        nz = np.nonzero(o["reflection"][i])[0]
        assert (int(nz[-1]) + 1 if len(nz) else 0) == f["order"]          # the order reached
        assert not np.any(o["lpc_coeffs"][i][f["order"] + 1:]) and not any(f["lpc_coeffs"][f["order"] + 1:])
        assert (o["residual_energy"][i] > 0) == (f["residual_energy"] > 0)
        assert len(f["lpc_coeffs"]) == p + 1 and len(f["reflection"]) == p
    d = C.measured_d(cid)
    print("%s: d = %.3g" % (cid, d))
    assert 16.0 * d <= 1e-6


@pytest.mark.parametrize("sr", sorted(C.RATES))
def test_cases_reach_their_branches(sr):
    """The census of the class's decided frames holds every count REQUIRED states."""
    got = C.census(sr)
    print(sr, got)
    short = {k: (got[k], n) for k, n in C.REQUIRED[sr].items() if got[k] < n}
    assert not short, short
    assert got["max_order"] == C.RATES[sr][1] > 4
    assert got["bw_outside"] == 0                       # the clamp to [50, 500] leaves that arm dead


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_undecided_cap(cid):
    """At most 10 % of a case's ok frames are undecided and at least 8 are decided: a condition on the
    inputs, not a measurement.  An input that misses it is replaced."""
    ok = [f for f in C.reference(cid) if f["status"] == 0]
    dec = sum(1 for f in ok if f["decided"])
    assert dec >= 8 and 10 * (len(ok) - dec) <= len(ok)


def test_every_arm_is_reached_somewhere():
    tot = {}
    for sr in C.RATES:
        for k, v in C.census(sr).items():
            tot[k] = tot.get(k, 0) + v
    for k in ("freq_300-3500", "freq_100-5000", "freq_outside", "bw_50-300", "bw_30-500", "full_drop_conf",
              "full_merge", "full_merge_replaced", "full_vtl_rejected_conf", "full_vtl_rejected_window",
              "quality_E_pos", "quality_E_nonpos", "full_nf0", "full_nf1"):
        assert tot[k] > 0, k
    merged = [f for c in C.CASE_IDS for f in C.reference(c) if f["census"]["merges"] > f["census"]["merge_replaced"]]
    assert merged                                       # a merge that keeps the earlier formant


_MP_TABLE = []


def _mp_table():
    """cos and sin of 2 pi j / 1024 at 50 digits as integers scaled by 2^200 (every angle -i w is one)."""
    if not _MP_TABLE:
        with mpmath.workdps(70):
            for j in range(R.NFFT):
                t = 2 * mpmath.pi * j / R.NFFT
                _MP_TABLE.append((int(mpmath.floor(mpmath.cos(t) * 2 ** 200)), int(mpmath.floor(mpmath.sin(t) * 2 ** 200))))
    return _MP_TABLE


def _exact_inverse_envelope_sq(a, p):
    """|A(w_k)|^2 * 2^800 for k = 0..512 in integer arithmetic: a_i exact, the table good to 2^-200."""
    T = _mp_table()
    ai = [int(math.ldexp(v, 200)) for v in a]            # exact: |a_i| is 0 or far above 2^-147
    out = []
    for kk in range(R.NFFT // 2 + 1):
        rp = 1 << 400
        ip = 0
        for i in range(1, p + 1):
            c, s = T[(i * kk) % R.NFFT]
            rp += ai[i] * c
            ip -= ai[i] * s                              # sin(-i w)
        out.append(rp * rp + ip * ip)
    return out


@pytest.mark.parametrize("cid", C.CASE_IDS)
def test_libm_envelope_inside_the_bound(cid):
    """Guards the derivation in formant_ref's docstring (it does not measure the kernel): on every case
    frame the checker's own envelope is within rel_k of the envelope at 50 digits."""
    worst = 0.0
    with mpmath.workdps(50):
        for f in C.reference(cid):
            a = f["lpc_coeffs"]
            p = len(a) - 1
            assert all(v == 0 or abs(v) > 1e-40 for v in a)
            env, rel = R.envelope(a, p)
            for kk, sq in enumerate(_exact_inverse_envelope_sq(a, p)):
                true = 1 / mpmath.sqrt(mpmath.mpf(sq) / mpmath.mpf(2) ** 800)
                e = float(abs(mpmath.mpf(float(env[kk])) - true) / true)
                assert e <= rel[kk], (kk, e, rel[kk])
                worst = max(worst, e / rel[kk])
    print("%s: worst |env - true| / bound = %.3g" % (cid, worst))


def test_stages_feed_from_outside():
    """Each stage takes its input from outside: the textbook order-2 case by hand."""
    st, a, k, E, order = R.levinson([1.0, 0.5, 0.25], 2)
    assert (st, order) == (0, 2) and a == [1.0, 0.5, 0.0] and k == [0.5, 0.0] and E == 0.75
    assert R.levinson([0.0, 1.0], 1)[0] == 3
    st, a, k, E, order = R.levinson([1.0, 1.0, 0.0], 2)
    assert (st, order, E) == (0, 1, 0.0)                 # k = 1: E <= 0 breaks before E == 0 can be status 4
    st, a, k, E, order = R.levinson([1.0, 2.0, 0.0, 0.0], 3)
    assert (st, order) == (0, 1) and E == -3.0 and a[2:] == [0.0, 0.0]   # E <= 0 breaks, no error
    env, rel = R.envelope([1.0, -0.5], 1)
    assert env[0] == 2.0 and abs(env[512] - 1 / 1.5) < 1e-15 and np.all(rel > 0)
    t = R.tail([1.0, -0.5], 0.75, 8000)
    assert t["n_formants"] == 0 and t["vocal_tract_length"] == 17.5 and t["stable"] == 1 and t["decided"]
    z = R.preprocess(np.arange(1024.0), 8000)
    assert abs(float(np.mean(z))) < 1e-12 and abs(float(np.mean(z * z)) - 1.0) < 1e-12
    assert R.preprocess(np.zeros(1024), 8000).tolist() == [0.0] * 1024    # sd < 1e-10: no division
    assert len(R.lags(z, 20)) == 21
