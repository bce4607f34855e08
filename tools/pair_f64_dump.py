"""float64 MFCCs of mfcc_pair_kernel<double> on a fixed signal, saved for a byte-for-byte comparison
of two builds (the float32 headline has bench.py --dump-outputs for the same purpose).

Usage (GPU box): [SONAR_LIB=.../libsonar_gpu.so] python tools/pair_f64_dump.py DIR [seconds]
writes DIR/mfcc_f64.npy (float64 PCM) and DIR/mfcc_f64w.npy (float32 PCM widened); compare two
builds' files with cmp."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sonido-sonar_amd"), ROOT]
import numpy as np  # noqa: E402
import sonar  # noqa: E402
from sonar import synth  # noqa: E402


def main():
    out = sys.argv[1]
    seconds = float(sys.argv[2]) if len(sys.argv) > 2 else 120.0
    os.makedirs(out, exist_ok=True)
    ctx = sonar.Context(0)
    x = synth.c2_hour(seconds=seconds)
    for name, pcm, pdt in (("mfcc_f64", x.astype(np.float64), sonar.F64), ("mfcc_f64w", x.astype(np.float32), sonar.F32)):
        cfg = ctx.config(window_size=1024, hop_size=256, sample_rate=44100, n_filters=40, n_mfcc=13,
                         precision=sonar.F64, pcm_dtype=pdt, out_dtype=sonar.F64)
        got = ctx.fingerprint(pcm, cfg)["mfcc"]
        assert ctx.last_fp_kernel() == "mfcc_pair_kernel" and got.dtype == np.float64
        np.save(os.path.join(out, name + ".npy"), got)
        print(name, got.shape, "sum", repr(float(got.sum())))


if __name__ == "__main__":
    main()
