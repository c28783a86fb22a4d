"""The plan of a fused step launch (StepPolicy::plan_step, terrarium.jl_amd/csrc/trm_host.hpp) is a pure function of the context:
tests/step_plan_preconditions.cpp asserts it on hand-built contexts, as a stand-alone program under AddressSanitizer and UBSan.  This
builds and runs it (with the other precondition programs of the same make target); no GPU."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "terrarium.jl_amd", "csrc")


def test_step_plan_preconditions_hold_under_the_host_sanitizers():
    env = {k: v for k, v in os.environ.items() if k not in ("TRM_STAGED_SMALL", "TRM_SCALAR_INPUTS")}      # (the rules, not the experiments' switches)
    r = subprocess.run(["make", "-C", CSRC, "-s", "check-preconditions"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "step plan preconditions ok" in r.stdout
