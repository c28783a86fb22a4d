"""Writes tests/golden/launch_dispatch_programs.json: what tests/test_gpu_launch_dispatch.py compares against.  Run ONCE, on a GPU, with
the library of the commit whose launches are to be pinned (TRM_LIBRARY names a library other than the tree's):
    python tests/golden/make_launch_dispatch_fixture.py [OUT.json]
Before a case is recorded its final state is checked against the oracle (the helpers and tolerances of tests/test_gpu_parity.py), so the
fixture holds states the reference agrees with.  The committed file was recorded with the library of the parent commit of the change that
put the launch files on one value-to-instance dispatcher."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import test_gpu_launch_dispatch as T
import test_gpu_parity as P
import workloads as W


def check_against_the_oracle(c):
    """The calls of T.CALLS on the device and, step for step, on the oracle; a refused call ends the comparison before it."""
    w = T.workload(c)
    d, o = T.device(c, w), W.setup_oracle(w)
    T.attach_series(c, w, o)
    for steps, finalize in T.CALLS:
        try:
            (d.step_heun if c["heun"] else d.step)(w["dt"], steps, finalize=finalize)
        except T.trm._capi.TerrariumHipError:
            break
        for n in range(steps):
            (o.timestep_heun if c["heun"] else o.timestep)(w["dt"], finalize=bool(finalize and n == steps - 1))
    exact = P.bit_exact_config(c["config"], c["hydraulics"], w["dtype"]) and not c["series"]
    names = list(T.HASHED) if c["config"] != "heat" else ["internal_energy", "temperature"]
    P.assert_fields_match(d, o, names, exact, P.TOL64 if w["dtype"] == np.float64 else P.TOL32, c["name"] + " ")
    assert d.clock() == o.clock()
    d.close()


out = sys.argv[1] if len(sys.argv) > 1 else T.FIXTURE
cases = {}
for c in T.CASES:
    check_against_the_oracle(c)
    cases[c["name"]] = dict(context=c, after_each_call=T.record(c))
    print(c["name"], [r.get("refused", r.get("info", [0])[0]) for r in cases[c["name"]]["after_each_call"]], flush=True)
with open(out, "w") as f:
    json.dump(dict(info=list(T.INFO), hashed=list(T.HASHED), calls=[[n, int(fin)] for n, fin in T.CALLS], cases=cases), f, indent=1, sort_keys=True)
    f.write("\n")
print(f"{len(cases)} cases -> {out}")
