"""sonar_chroma_cqt on the GPU against the Python checker (tests/chroma_cqt_ref.py, held to F24 and to a
closed form in test_chroma_cqt_cpu.py).

Tolerances are the project's float64 rule: CQT magnitudes within 1e-9 of scale[f][k] = N |frame[:L_k]|
|g_k| (the "1e-9 of the row norm" rule), chroma within 1e-9 absolute.  Inputs are 0.5 + 0.1 N(0, 1):
the reference's kernels are Gaussian low-passes, so a signal needs low-frequency content for the
reference itself to be well conditioned; every chroma comparison first asserts on the checker's output
that each frame has max_k cqt / scale >= 0.1.

Shapes: the kernel takes 8 frames x 8 bins per wave, 4 waves (32 frames) per block, 64 taps per step.
A (36 bins: 5 groups, the last ragged) at 45 frames has a ragged frame tile and frames past the
signal's end; 1,092 frames are 35 blocks with a ragged last one; D crosses hundreds of tap steps and
zero-pads inside its longest kernels; the capped configuration has even lengths; 108 bins are 14
groups; the 5-bin case has one ragged group."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401 -- before the library loads HIP (one HIP runtime in the process)

import chroma_cqt_ref as R
import sonar

pytestmark = pytest.mark.gpu

A = dict(sample_rate=8000, min_freq=200.0, max_freq=1600.0, bins_per_octave=12, q_factor=5.0, tuning_freq=440.0)
A36 = dict(A, bins_per_octave=36)
D = dict(sample_rate=44100, **R.DEFAULT)
CAPPED = dict(sample_rate=8000, min_freq=30.0, max_freq=480.0, bins_per_octave=12, q_factor=25.0, tuning_freq=440.0)
FIVE = dict(sample_rate=8000, min_freq=200.0, max_freq=400.0, bins_per_octave=5, q_factor=5.0, tuning_freq=432.0)
CFGS = {"A": A, "A36": A36, "D": D, "capped": CAPPED, "five": FIVE}


@functools.lru_cache(maxsize=None)
def _signal(n, amp=1.0, kind="noise"):
    if kind == "zeros":
        x = np.zeros(n)
    else:
        x = amp * (0.5 + 0.1 * np.random.default_rng(n).standard_normal(n))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(name, n, hop, amp=1.0, kind="noise"):
    ref = R.chroma_cqt(_signal(n, amp, kind), hop, **CFGS[name])
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _run(ctx, name, n, hop, amp=1.0, kind="noise"):
    cfg = CFGS[name]
    return ctx.chroma_cqt(_signal(n, amp, kind), hop, return_cqt=True, **cfg)


def _compare(ctx, name, n, hop, frames):
    ref = _ref(name, n, hop)
    assert ref["cqt"].shape[0] == frames
    conditioning = np.max(ref["cqt"] / ref["scale"], axis=1)
    print(f"{name} n={n} hop={hop}: min over frames of max_k cqt/scale = {conditioning.min():.3g}")
    assert conditioning.min() >= 0.1
    chroma, cqt = _run(ctx, name, n, hop)
    assert chroma.shape == (frames, 12) and cqt.shape == ref["cqt"].shape
    err_cqt = np.max(np.abs(cqt - ref["cqt"]) / ref["scale"])
    err_chroma = np.max(np.abs(chroma - ref["chroma"]))
    print(f"  cqt error / scale = {err_cqt:.3g}, chroma error = {err_chroma:.3g}")
    assert err_cqt <= 1e-9
    assert err_chroma <= 1e-9
    return chroma, cqt, ref


def test_a_frames_past_the_end(ctx):
    _compare(ctx, "A", 3000, 64, 45)                         # 44 * 64 + 201 > 3000


def test_a_many_frame_tiles(ctx):
    _compare(ctx, "A", 70000, 64, 1092)


@pytest.mark.parametrize("hop,frames", [(512, 77), (4096, 8)])
def test_default_configuration(ctx, hop, frames):
    """L_0 = 16,857 taps; at hop 512 every frame past the 46th is zero-padded inside its longest kernels."""
    _compare(ctx, "D", 40000, hop, frames)


def test_capped_even_lengths(ctx):
    _compare(ctx, "capped", 9000, 100, 89)


def test_more_than_one_wave_of_bins(ctx):
    _, cqt, _ = _compare(ctx, "A36", 3000, 50, 59)
    assert cqt.shape[1] == 108


def test_five_bins_leave_seven_classes_empty(ctx):
    chroma, _, ref = _compare(ctx, "five", 3000, 64, 45)
    used = sorted(set(ref["plan"]["chroma_bin"].tolist()))
    assert used == [0, 3, 5, 8, 10]
    empty = [c for c in range(12) if c not in used]
    assert np.all(chroma[:, empty] == 0.0)
    assert np.max(np.abs(chroma[:, used].sum(axis=1) - 1.0)) <= 1e-12


@pytest.mark.parametrize("hop", [5000, -5])
def test_one_frame_when_the_hop_exceeds_the_signal_or_is_negative(ctx, hop):
    _compare(ctx, "A", 3000, hop, 1)


def test_single_sample(ctx):
    """One sample: every bin is N x[0] g_k[0], at 0.004 of its scale in the longest kernels, so the
    chroma is held to the fold of the returned CQT."""
    ref = _ref("A", 1, 64)
    chroma, cqt = _run(ctx, "A", 1, 64)
    assert chroma.shape == (1, 12) and cqt.shape == (1, 36)
    assert np.max(np.abs(cqt - ref["cqt"]) / ref["scale"]) <= 1e-9
    folded, _ = R.fold(cqt, ref["plan"]["chroma_bin"])
    assert np.max(np.abs(chroma - folded)) <= 1e-12


def test_threshold(ctx):
    chroma, cqt = _run(ctx, "A", 3000, 64, kind="zeros")
    assert chroma.shape == (45, 12) and np.all(chroma == 0.0) and np.all(cqt == 0.0)
    # far below 1e-10: the frame is not divided by its sum
    ref = _ref("A", 3000, 64, amp=1e-12)
    assert ref["energy"].max() < 1e-12 and ref["energy"].min() > 0.0
    assert np.array_equal(ref["chroma"].sum(axis=1) < 1e-12, np.ones(45, bool))
    chroma, cqt = _run(ctx, "A", 3000, 64, amp=1e-12)
    tol = 1e-9 * np.min(ref["scale"] ** 2, axis=1)           # the strictest reading: the smallest bin's scale^2
    assert np.all(np.abs(chroma - ref["chroma"]) <= tol[:, None])
    assert np.max(np.abs(cqt - ref["cqt"]) / ref["scale"]) <= 1e-9
    # the same noise at amplitude 1: far above, normalised
    ref1 = _ref("A", 3000, 64)
    assert ref1["energy"].min() > 1.0
    chroma1, _ = _run(ctx, "A", 3000, 64)
    assert np.max(np.abs(chroma1.sum(axis=1) - 1.0)) <= 1e-12
    assert np.max(np.abs(chroma1 - ref1["chroma"])) <= 1e-9


def test_errors_and_results(ctx):
    x = _signal(3000)
    with pytest.raises(sonar.SonarError, match="runtime error: integer divide by zero") as e:
        ctx.chroma_cqt(x, 0, **A)
    assert e.value.code == sonar.ERR_PANIC
    with pytest.raises(sonar.SonarError, match="runtime error: makeslice: len out of range") as e:
        ctx.chroma_cqt(x, 64, **dict(A, max_freq=100.0))
    assert e.value.code == sonar.ERR_PANIC
    with pytest.raises(sonar.SonarError, match=r"runtime error: index out of range \[0\] with length 0") as e:
        ctx.chroma_cqt(x, 64, **dict(A, max_freq=200.0))
    assert e.value.code == sonar.ERR_PANIC
    bad = x.copy()
    bad[1234] = np.nan
    for args, kw in (((bad, 64), A), ((x, 64), dict(A, q_factor=0.0)), ((x, 64), dict(A, q_factor=-1.0)),
                     ((x, 64), dict(A, bins_per_octave=0))):
        with pytest.raises(sonar.SonarError, match="not reproduced") as e:
            ctx.chroma_cqt(*args, **kw)
        assert e.value.code == sonar.ERR_UNSUPPORTED
    out = ctx.chroma_cqt(np.zeros(0), 64, **A)
    assert out.shape == (0, 12)
    assert ctx.chroma_cqt(np.zeros(0), 0, **A).shape == (0, 12)   # Go returns before the division


def test_device_pointers_repeat_calls_and_the_table_cache(ctx):
    x = _signal(3000)
    chroma, cqt = ctx.chroma_cqt(x, 64, return_cqt=True, **A)
    again = ctx.chroma_cqt(x, 64, return_cqt=True, **A)
    assert np.array_equal(again[0], chroma) and np.array_equal(again[1], cqt)
    dx = torch.from_numpy(x.copy()).cuda()
    dchroma = torch.zeros(45, 12, dtype=torch.float64, device="cuda")
    dcqt = torch.zeros(45, 36, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ctx.chroma_cqt_device(dx.data_ptr(), 3000, 64, A["sample_rate"], dchroma.data_ptr(), cqt_ptr=dcqt.data_ptr(),
                          **{k: v for k, v in A.items() if k != "sample_rate"})
    assert np.array_equal(dchroma.cpu().numpy(), chroma) and np.array_equal(dcqt.cpu().numpy(), cqt)
    dchroma.zero_()
    torch.cuda.synchronize()
    ctx.chroma_cqt_device(dx.data_ptr(), 3000, 64, A["sample_rate"], dchroma.data_ptr(),
                          **{k: v for k, v in A.items() if k != "sample_rate"})   # null cqt: library scratch
    assert np.array_equal(dchroma.cpu().numpy(), chroma)
    # a second parameter set on the context leaves the first one's cached table alone
    other = ctx.chroma_cqt(_signal(40000), 4096, **D)
    assert other.shape == (8, 12)
    assert np.array_equal(ctx.chroma_cqt(x, 64, **A), chroma)
    ctx.trim()                                               # the tables are rebuilt after a trim
    assert np.array_equal(ctx.chroma_cqt(x, 64, **A), chroma)
