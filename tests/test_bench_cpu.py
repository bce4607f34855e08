"""bench.py's roofline helpers on the CPU (no GPU calls): the C5 roofline's algorithmic bytes and
the committed kernel-family shares it carries, and the committed PMC summaries the bench line
reads (the newest per pattern)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
bench = pytest.importorskip("bench")


def test_c5_roofline_bytes_and_families():
    F = 10_333
    samples = 2 * 2_646_000
    r = bench.c5_roofline(1000, 0.5, samples, F)
    per_pair = samples * 8 + bench.DTW_BYTES_PER_CELL * F * F
    assert r["alg_bytes_per_pair"] == pytest.approx(per_pair)
    assert r["achieved"] == pytest.approx(1000 * per_pair / 0.5 / 1e9)
    assert r["frac"] == pytest.approx(r["achieved"] / bench.HBM_PEAK_GBS)
    fam = r["kernel_families"]
    assert fam is not None and fam["source"].startswith("profiles/")
    shares = fam["shares"]
    assert abs(sum(shares.values()) - 1.0) < 1e-3
    assert {"dtw_band", "features"} <= set(shares)


def test_dump_outputs_whole_and_sampled(tmp_path):
    """--dump-outputs: an output within the budget is saved whole as float32; a larger one as a
    seeded sample of whole rows in frame order with their indices, the two files within the budget."""
    import numpy as np
    import torch
    x = torch.arange(13 * 1000, dtype=torch.float32).reshape(1000, 13)
    bench.dump_outputs(str(tmp_path / "a"), x, 1, 0)
    a = np.load(tmp_path / "a" / "mfcc.npy")
    assert sorted(os.listdir(tmp_path / "a")) == ["mfcc.npy"]
    assert a.dtype == np.float32 and np.array_equal(a, x.numpy())
    for d in ("b", "c"):                                   # the sample is the same from run to run
        bench.dump_outputs(str(tmp_path / d), x, 1, 0, budget=20000)
    b, rows = np.load(tmp_path / "b" / "mfcc.npy"), np.load(tmp_path / "b" / "mfcc_rows.npy")
    assert b.dtype == np.float32 and rows.dtype == np.float64
    assert 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(b, x.numpy()[rows.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 20000
    assert np.array_equal(rows, np.load(tmp_path / "c" / "mfcc_rows.npy"))
    bench.dump_outputs(str(tmp_path / "r"), x, 2, 1)       # N ranks: one file per rank
    assert sorted(os.listdir(tmp_path / "r")) == ["mfcc_rank1.npy"]


def test_committed_pmc_summaries_load():
    dtw = bench.load_pmc_bytes("*dtw_pmc*.json", "dtw_band_kernel<12, true, false, false")
    assert dtw is not None and dtw["bytes_per_launch"] > 0
