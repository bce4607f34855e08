"""CPU: csrc/go_math.h (math.Max, math.Min, math.Log2 for the host layer and the kernels) compiled by
the plain host C++ compiler into tests/c_abi/build/go_math_check, which checks the answers Go's math
documentation gives: the signed zeros, NaN against +-Inf, Log2 exact at every power of two from
2^-1074 to 2^1023, the special values, and the Frexp / Log formula to the last bit elsewhere."""
import os
import subprocess

CABI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi")


def test_go_math_header_known_answers():
    subprocess.run(["make", "-s", "-C", CABI, "build/go_math_check"], check=True)
    run = subprocess.run([os.path.join(CABI, "build", "go_math_check")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "go_math ok", run.stdout + run.stderr
