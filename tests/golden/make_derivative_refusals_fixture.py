"""Writes tests/golden/derivative_refusals.json: what tests/test_gpu_derivative_refusals.py compares against.  Run ONCE, on a GPU, with
the library of the commit whose answers are to be pinned (TRM_LIBRARY names a library other than the tree's):
    python tests/golden/make_derivative_refusals_fixture.py [OUT.json]
The committed file was recorded with the library of the parent commit of the change that moved the derivative entry points into
trm_derivative_api.hip."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import test_gpu_derivative_refusals as T

out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
scenarios = {s.__name__: T.record(s) for s in T.SCENARIOS}
header = ("recorded once with the library of the parent commit (cff79be: the derivative host layer inside terrarium_hip.hip), ABI "
          f"{T.trm._capi.lib().trm_abi_version()}; entries are [call, return code, trm_last_error text of a refusal]")
with open(out, "w") as f:
    json.dump(dict(header=header, scenarios=scenarios), f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{sum(len(v) for v in scenarios.values())} calls in {len(scenarios)} scenarios -> {out}")
