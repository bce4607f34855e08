"""bench.py's plain run (no --full), in a fresh child process on a 20 s stream: the result line holds
the headline fields and none of the --full legs, --steps sets the number of timed steps, and
--dump-outputs saves the MFCC rows the timed path wrote in its last step -- equal, bit for bit, to
the product's own call on the same stream."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sonar
from sonar import shard

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SR = 1024, 256, 44100


def test_plain_run_line_and_dumped_outputs(ctx, tmp_path):
    seconds = 20.0
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--seconds", str(seconds), "--dump-outputs", str(tmp_path / "dump")]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["frames_total"] / (d["ms_per_step"] * 1e-3))
    assert d["roofline"]["kernel"] == "mfcc_pair_kernel"
    assert d["cpu_baseline"] is None and d["parity"] is None
    legs = ("headline_f64", "c1_", "dtw_", "ingest_", "fp_batch", "c5_", "c3_", "c4_", "c6_", "c7_")
    assert [k for k in d if k.startswith(legs)] == []

    n = int(round(seconds * SR))
    pcm = shard.stream_pcm(0, n, device="cuda")
    F = sonar.stft_frames(n, W, H)
    out = torch.empty((F, 13), dtype=torch.float32, device="cuda")
    cfg = ctx.config(window_size=W, hop_size=H, sample_rate=SR, n_filters=40, n_mfcc=13, precision=sonar.F32,
                     pcm_dtype=sonar.F32, out_dtype=sonar.F32, flags=sonar.FP_MFCC)
    torch.cuda.synchronize()        # pcm was written on torch's stream; ctx launches on its own non-blocking one
    ctx.fingerprint_device(pcm.data_ptr(), n, cfg, mfcc=out.data_ptr())
    torch.cuda.synchronize()
    assert sorted(os.listdir(tmp_path / "dump")) == ["mfcc.npy"]
    got = np.load(tmp_path / "dump" / "mfcc.npy")
    assert got.dtype == np.float32 and got.shape == (F, 13)
    assert np.array_equal(got, out.cpu().numpy())
