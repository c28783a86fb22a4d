"""Writes tests/golden/derivative_driver_calls.json: what tests/test_derivative_driver_calls_host.py compares against.  Run ONCE, with
the package of the commit whose drivers are to be pinned (TREE names a checkout other than this one; no GPU, no library):
    python tests/golden/make_derivative_driver_calls_fixture.py [OUT.json] [TREE]
The committed file was recorded with the package of the parent commit of the change that moved the derivative drivers from
integrator.py into derivatives.py."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TREE = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else ROOT
sys.path[:0] = [TREE, os.path.join(ROOT, "tests")]

import test_derivative_driver_calls_host as T

assert os.path.dirname(os.path.abspath(T.trm.__file__)) == os.path.join(TREE, "terrarium.jl_amd"), T.trm.__file__
out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
scenarios = T.record_all()
header = ("recorded once with the package of the parent commit (d784711: the five drivers inside integrator.py); entries are the calls a "
          "driver makes on a stub state, [method, {parameter: value}] in order (arrays by shape), and what it returned or raised")
with open(out, "w") as f:
    json.dump(dict(header=header, scenarios=scenarios), f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{sum(len(v['calls']) for v in scenarios.values())} calls in {len(scenarios)} scenarios -> {out}")
