"""CPU: csrc/pair_batch_layout.h (the one layout of a pair batch's device and pinned buffers) compiled by
the plain host C++ compiler into tests/c_abi/build/pair_layout_check, which checks for 1, 2, 8 and 128
pairs, 1, 2 and n x 162 bands, with and without correlation and path bytes: every section 256-byte
aligned, sections disjoint and in order, the head a prefix, the upload one run from the DTW arguments,
the total the sum, and the byte offsets those of the hand-written layout the header replaced."""
import os
import subprocess

CABI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi")


def test_pair_batch_layout_offsets():
    subprocess.run(["make", "-s", "-C", CABI, "build/pair_layout_check"], check=True)
    run = subprocess.run([os.path.join(CABI, "build", "pair_layout_check")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "pair_layout ok", run.stdout + run.stderr
