"""CPU: csrc/staging.h compiled by the plain host C++ compiler (HIP headers, no HIP library) into
tests/c_abi/build/staging_check, against an asynchronous stub of the runtime calls Staging makes: the
exact call list of an entry that uses every method, in both pointer modes, with the values arriving;
and, with every call of that list failed in turn, SONAR_ERR_DEVICE naming the call and nothing left
queued once the entry's Staging is gone."""
import os
import subprocess

CABI = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c_abi")


def test_staging_call_lists_and_failure_injection():
    subprocess.run(["make", "-s", "-C", CABI, "build/staging_check"], check=True)
    run = subprocess.run([os.path.join(CABI, "build", "staging_check")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "staging ok", run.stdout + run.stderr
