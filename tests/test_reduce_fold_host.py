"""The two-operand folds of TRM_REDUCE_MIN / TRM_REDUCE_MAX (terrarium.jl_amd/csrc/trm_reduce_fold.hpp) are __host__ __device__: the
host folds of trm_reduce and trm_reduce_global_all call the functions the kernel calls.  tests/reduce_fold_preconditions.cpp asserts
Julia's Base.minimum / maximum on NaN, infinities and zeros of both signs, in every operand order, as a stand-alone program under
AddressSanitizer and UBSan.  This builds and runs it; no GPU.  (The device side: tests/test_gpu_field_io_edges.py.)"""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "terrarium.jl_amd", "csrc")


def test_reduce_fold_preconditions_hold_under_the_host_sanitizers():
    r = subprocess.run(["make", "-C", CSRC, "-s", "check-preconditions", "PRECONDITIONS=reduce_fold_preconditions"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "reduce fold preconditions ok" in r.stdout
