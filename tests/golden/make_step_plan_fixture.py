"""Writes tests/golden/step_plan_programs.json: what tests/test_gpu_step_plan.py compares against.  Run ONCE, on a GPU, with the library
of the commit whose selection is to be pinned (TRM_LIBRARY names a library other than the tree's):
    python tests/golden/make_step_plan_fixture.py [OUT.json]
The committed file was recorded with the library of the parent commit of the change that introduced the step plan."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import test_gpu_step_plan as T

out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
cases = {c["name"]: dict(context=c, after_each_call=T.record(c)) for c in T.CASES}
with open(out, "w") as f:
    json.dump(dict(info=list(T.INFO), calls=[[n, int(fin)] for n, fin in T.CALLS], cases=cases), f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(cases)} cases -> {out}")
