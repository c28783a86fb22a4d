"""The deriving, deferring and interior instances of the fp64 column step against the CPU oracle on edge states (tests/edge_states.py;
tests/test_edge_states_host.py pins on the oracle alone that the states are what that module claims).

tests/test_gpu_deferred_closure.py and tests/test_gpu_interior_steps.py compare a context with the option on against its twin with the
option off, on the smooth state of workloads.make_workload: an error both twins share, or one that needs a saturation of exactly 1, a
moving water table or a kink of the energy closure to show, passes there.  Here every instance is one context, forced through
set_option and identified by TRM_INFO_LAST_PROGRAM (a test must not pass because the library chose another instance), and compared
with the oracle after every call of

    step(dt, 1, False); step(dt, 7, False); step(dt, 1, False); step(dt, 7, True)                    (edge_states.CALLS, 16 steps)

-- the oracle taking timestep(dt, finalize) with the same flags.  Default hydraulics (BrooksCorey + linear K): bit for bit, the sign
bit included (pressure_head<NF, HYD, true> asserts that the loaded saturation is never -0.0).  van Genuchten: every variant is
byte-identical to the reference-order kernels ("unfused": all implementations share the device arithmetic), and those are measured
against the wide oracle with the metric and the M of tests/test_gpu_accuracy.py.

INTERIOR LAUNCHES.  By the rule of tests/test_gpu_interior_steps.py (Ops::step: a launch goes interior if it is not its call's last
and derives T / liq; the first launch after trm_initialize reads them as stored) a first call of n steps has max(0, n - 2) interior
launches and a later one n - 1: 0 + 6 + 0 + 6 = 12 over the four calls.  A context prepared with trm_closure derives from its first
launch on; its first call is a single launch all the same: 12 again.

THE ILLEGAL STATE (test_status_and_lane_isolation).  illegal_dry_workload leaves the composition bounds in step 3 on the unfrozen
kind-5 columns (edge_states.ILLEGAL_AT).  The 13-column workload named for this test holds a single kind-5 column and that one is
frozen, so it stays valid on the oracle (tests/test_edge_states_host.py::test_illegal_dry_workload pins this): (13, 32) checks the
status word and the lane sharing with a dry but valid column, and (67, 32) is added so that an invalid column shares a wave with a
valid one at 32 lanes per column as well as at 64 (67, 40).

Measured on one MI355X (profiles/r11): every case passes; the worst ratio of the van Genuchten rows is 3.6
(tend_saturation_water_ice) against M = 8, no cell left out.  Every test prints its rows before it asserts (pytest -s)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (_ROOT, os.path.join(_ROOT, "oracle"), os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:      # (the child process of the staged case runs this file as a script)
        sys.path.insert(0, _p)

import accuracy as A
import edge_states as E
import terrarium_jl_amd as trm
import workloads as W
from test_gpu_accuracy import M
from test_gpu_interior_steps import SIGNATURES

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("internal_energy", "saturation_water_ice", "surface_excess_water", "water_table", "temperature", "liquid_water_fraction",
                "pressure_head")
HEAT_STATE_FIELDS = ("internal_energy", "temperature", "liquid_water_fraction")

VARIANTS = {
    "classic": dict(derive_closure_fields=0),
    "derive": dict(derive_closure_fields=1, defer_closure_stores=0, interior_steps=0),
    "defer": dict(derive_closure_fields=1, defer_closure_stores=1, interior_steps=0),
    "interior": dict(derive_closure_fields=1, defer_closure_stores=1, interior_steps=1),
    "runtime_kinds": dict(derive_closure_fields=1, bc_signature=0),
    "multi3": dict(steps_per_launch=3),
    "multi": dict(steps_per_launch=0),
    "unfused": dict(step_kernel="unfused"),
}
DERIVING = ("derive", "defer", "interior", "runtime_kinds")
AUTO_STEPS_PER_LAUNCH = 50      # (Ops::auto_steps_per_launch)


# ---- workloads and references, computed once per key and left unchanged ---------------------------------------------------------------
def _workload(key):
    """key = (what, hydraulics, ncol, Nz, config, index into SIGNATURES or None); what in {"edge", "kink", "illegal"}"""
    what, hydraulics, ncol, Nz, config, sig = key
    w = E.illegal_dry_workload(Nz, ncol) if what == "illegal" else E.edge_workload(hydraulics, Nz, ncol, config=config)
    if sig is not None:
        w = E.with_signature(w, SIGNATURES[sig][0])
    return A.rounded_workload(w)


def _kink_columns(w):
    return np.flatnonzero((w["kind"] == 6) | (w["kind"] == 7))


def _prepare(key, w, sides):
    if key[0] == "kink":
        E.put_energy_on_lower_kink(w, sides, _kink_columns(w))


def _state_fields(w):
    return HEAT_STATE_FIELDS if w["config"] == "heat" else STATE_FIELDS


def _snapshot(source, names):
    out = {}
    for n in names:
        a = np.array(source.get(n))
        a.setflags(write=False)
        out[n] = a
    return out


def _names_of_call(w, finalize):
    return list(A.field_names(w)) if finalize else list(_state_fields(w))


@functools.lru_cache(maxsize=None)
def oracle_reference(key, wide=False):
    """per call of E.CALLS: (fields, status, clock) of the CPU oracle -- fp64, or the wide one"""
    w = _workload(key)
    o = A.setup_oracle(w, wide=wide)
    _prepare(key, w, [o])
    calls = []
    for nsteps, finalize in E.CALLS:
        for n in range(nsteps):
            o.timestep(w["dt"], finalize and n == nsteps - 1)
        calls.append((_snapshot(o, _names_of_call(w, finalize)), o.status(), o.clock()))
    return calls


# ---- one context per variant ----------------------------------------------------------------------------------------------------------
def _signature(key, w):
    if key[5] is not None:
        return SIGNATURES[key[5]][1]
    return 2 if w["config"] == "heat" else 34      # (T at the top; + the top saturation flux of the edge workload)


def expected_program(variant, w, signature, call, nsteps, staged, prepared):
    """what TRM_INFO_LAST_PROGRAM must decode to after call number `call` (of `nsteps` steps), from the host rules"""
    lanes = 32 if w["Nz"] <= 32 else 64
    hyd = "vg_n2" if w["params"].get("swrc") else "default"
    if variant == "unfused":
        return dict(family="unfused", lanes_per_column=0, derive="none", staged=False, scalar_inputs=False, bc_signature=-1)
    classic = dict(family="column_euler", hydraulics=hyd, lanes_per_column=lanes, derive="none", staged=False, scalar_inputs=True,
                   bc_signature=-1 if variant == "runtime_kinds" else signature)
    if variant in ("multi3", "multi"):
        spl = 3 if variant == "multi3" else AUTO_STEPS_PER_LAUNCH
        last = nsteps - spl * ((nsteps - 1) // spl)      # steps of the call's last launch; a launch of one step is the per-step program
        if last > 1:
            return dict(family="column_multi", hydraulics=hyd, lanes_per_column=lanes, derive="none", staged=False, scalar_inputs=True, bc_signature=-1)
        return classic
    if variant in DERIVING and (call > 0 or prepared):      # (the first launch after trm_initialize reads T / liq as stored)
        return dict(classic, derive="T_liq", staged=staged, scalar_inputs=not staged)
    return classic


def expected_interior_launches(variant, calls_done):
    """cumulative count after `calls_done` calls of E.CALLS, by the rule in this module's docstring"""
    if variant != "interior":
        return 0
    total = 0
    for i, (nsteps, _) in enumerate(E.CALLS[:calls_done]):
        total += max(0, nsteps - 2) if i == 0 else nsteps - 1
    return total


def _device(key, w, variant):
    d = W.setup_device(w)
    for k, v in VARIANTS[variant].items():
        d.set_option(k, v)
    _prepare(key, w, [d])
    return d


def run_device(key, variant, check, staged=False):
    """The four calls on one context of `variant`; after each: the program, the info keys, then check(call, names, device, w)."""
    w = _workload(key)
    d = _device(key, w, variant)
    signature = _signature(key, w)
    if variant != "unfused":
        assert d.get_option("info_bc_signature") == signature
    prepared = key[0] == "kink"
    for call, (nsteps, finalize) in enumerate(E.CALLS):
        d.step(w["dt"], nsteps, finalize=finalize)
        # (before anything is downloaded: a download materialises deferred T / liq)
        program = d.last_program()
        for k, v in expected_program(variant, w, signature, call, nsteps, staged, prepared).items():
            assert program[k] == v, (variant, call, k, program)
        assert d.get_option("info_interior_launches") == expected_interior_launches(variant, call + 1), (variant, call)
        if variant in ("defer", "interior") and nsteps > 1:
            assert d.get_option("info_closure_stored") == 0, (variant, call)
        if variant in ("classic", "derive", "unfused"):
            assert d.get_option("info_closure_stored") == 1, (variant, call)
        check(call, _names_of_call(w, finalize), d, w)
    assert E.CALLS[-1][1] and sum(n for n, _ in E.CALLS) == E.NSTEPS
    d.close()


def assert_same_bits(a, b, label, columns=None):
    assert a.shape == b.shape and a.dtype == b.dtype, label
    if columns is not None:
        a, b = a[..., columns], b[..., columns]
    if not np.array_equal(a, b):
        where = np.argwhere(a != b)
        raise AssertionError(f"{label}: {where.shape[0]} values differ, first at {where[:5].tolist()}: {a[tuple(where[0])]!r} != {b[tuple(where[0])]!r}")
    assert np.array_equal(np.signbit(a), np.signbit(b)), f"{label}: sign of zero"


def check_against_oracle(key):
    """bit for bit against the fp64 oracle, status and clock included"""
    ref = oracle_reference(key)

    def check(call, names, d, w):
        fields, status, clock = ref[call]
        assert d.status() == status == 0, (call, d.status(), status)
        assert d.clock() == clock
        for n in names:
            assert_same_bits(d.get(n), fields[n], f"call {call} {n}")
    return check


@functools.lru_cache(maxsize=None)
def unfused_reference(key):
    """per call: (fields, status, clock) of the reference-order kernels on the device"""
    calls = []

    def keep(call, names, d, w):
        calls.append((_snapshot(d, names), d.status(), d.clock()))
    run_device(key, "unfused", keep)
    return calls


def check_against_unfused(key):
    ref = unfused_reference(key)
    orc = oracle_reference(key)

    def check(call, names, d, w):
        fields, status, clock = ref[call]
        assert d.status() == status == orc[call][1] == 0, (call, d.status(), status)
        assert d.clock() == clock == orc[call][2]
        for n in names:
            assert d.get(n).tobytes() == fields[n].tobytes(), f"call {call} {n}"
    return check


def measure_unfused_against_the_wide_oracle(key, label):
    """accuracy.compare / accuracy.violations of the unfused run after every call; returns the rows of the last call"""
    w = _workload(key)
    dev, orc, ref = unfused_reference(key), oracle_reference(key), oracle_reference(key, True)
    rows = []
    for call, (nsteps, finalize) in enumerate(E.CALLS):
        names = _names_of_call(w, finalize)
        assert dev[call][1] == orc[call][1] == ref[call][1] == 0
        assert dev[call][2] == orc[call][2]
        rows = A.compare(dev[call][0], orc[call][0], ref[call][0], names, np.float64, label=f"{label} unfused, call {call}")
        worst = max(A.old_metric(dev[call][0][n], orc[call][0][n]) for n in names)
        print(f"  max |dev - orc| / max(1, |orc|) over the fields: {worst:.3e}")
        bad = A.violations(rows, np.float64, M)
        assert not bad, "\n".join(bad)
    return rows


def run_case(key, variant, staged=False, measure=True):
    exact = not _workload(key)["params"].get("swrc")
    if exact:
        run_device(key, variant, check_against_oracle(key), staged)
    elif variant == "unfused":
        if measure:
            if A.wide_skip_reason() is not None:
                pytest.skip(str(A.wide_skip_reason()))
            measure_unfused_against_the_wide_oracle(key, str(key))
        else:
            unfused_reference(key)
    else:
        run_device(key, variant, check_against_unfused(key), staged)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("ncol,Nz", E.SHAPES)
@pytest.mark.parametrize("hydraulics", ["default", "vg"])
def test_instances_against_the_oracle(hydraulics, ncol, Nz, variant):
    run_case(("edge", hydraulics, ncol, Nz, "richards", None), variant)


@pytest.mark.parametrize("variant", ["classic", "defer", "interior", "unfused"])
@pytest.mark.parametrize("index", range(len(SIGNATURES)), ids=[str(s) for _, s in SIGNATURES])
@pytest.mark.parametrize("hydraulics,ncol,Nz", E.SIGNATURE_SHAPES)
def test_every_signature(hydraulics, ncol, Nz, index, variant):
    """the four signatures column_psi_supported lists (0, 2, 6, 34); for 34 the edge workload's own top flux stands"""
    run_case(("edge", hydraulics, ncol, Nz, "richards", index), variant)


@pytest.mark.parametrize("config,variant", [("heat", v) for v in ("classic", "derive", "defer", "unfused")] +
                         [("richards", v) for v in ("classic", "derive", "defer", "interior", "unfused")])
def test_energy_kinks(config, variant):
    """U == -Lth exactly on every cell of kinds 6 and 7 (uploaded after initialize, closure() behind it), U == 0 on kind 6 before:
    the context derives T / liq from its first launch on.  Default hydraulics: bit-exact."""
    ncol, Nz = E.KINK_SHAPE
    run_case(("kink", "default", ncol, Nz, config, None), variant)


@pytest.mark.parametrize("variant", ["classic", "defer", "interior", "unfused"])
@pytest.mark.parametrize("ncol,Nz", E.STATUS_SHAPES)
def test_status_and_lane_isolation(ncol, Nz, variant):
    run_status_case(ncol, Nz, variant)


def run_status_case(ncol, Nz, variant, staged=False):
    """After every call the composition bit of the status word equals the oracle's -- the interior variant raises the bit of a skipped
    exit closure through ColumnArgs::check_entry, one launch late but inside the same call (step 3 is the second step of the second
    call) -- and every column the oracle keeps finite matches it bit for bit: at 32 lanes per column an invalid column shares its wave
    with a valid one, and a ballot or a lane shift that leaks across the half-wave shows here.  Values of the invalid columns are
    outside the contract and are not compared.  NaN arithmetic only."""
    key = ("illegal", "default", ncol, Nz, "richards", None)
    ref = oracle_reference(key)
    seen = []

    def check(call, names, d, w):
        fields, status, clock = ref[call]
        seen.append(status)
        assert d.status() & trm._capi.STATUS_COMPOSITION == status & trm._capi.STATUS_COMPOSITION, (call, d.status(), status)
        assert d.clock() == clock
        finite = np.ones(ncol, dtype=bool)
        for n in names:
            x = fields[n]
            finite &= np.isfinite(x).all(axis=0) if x.ndim == 2 else np.isfinite(x)
        assert set(w["kind"][~finite]) <= {5}
        assert (status != 0) == (not finite.all())
        for n in names:
            assert_same_bits(d.get(n), fields[n], f"call {call} {n}", columns=finite)

    run_device(key, variant, check, staged)
    first = E.ILLEGAL_AT[(ncol, Nz)]
    assert seen == ([0, 0, 0, 0] if first is None else [0, 2, 2, 2]) and first in (None, 3)


def test_staged_instances_in_a_child_process():
    """The staged + vector-input instances (what HBM-resident states take): TRM_STAGED_SMALL=1 TRM_SCALAR_INPUTS=0 are read once per
    process, hence the child process, which runs the defer and interior variants of edge_states.STAGED_SHAPES for both hydraulics and
    the status cases at 32 lanes per column, and asserts `staged` and not `scalar_inputs` of every launch it checks."""
    env = dict(os.environ, TRM_STAGED_SMALL="1", TRM_SCALAR_INPUTS="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--staged-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "staged child ok" in out.stdout


def _staged_child():
    for ncol, Nz in E.STAGED_SHAPES:
        for hydraulics in ("default", "vg"):
            for variant in ("defer", "interior"):
                run_case(("edge", hydraulics, ncol, Nz, "richards", None), variant, staged=True)
    for ncol, Nz in E.STATUS_SHAPES:
        if Nz <= 32:
            for variant in ("defer", "interior"):
                run_status_case(ncol, Nz, variant, staged=True)
    print("staged child ok")


if __name__ == "__main__":
    if "--staged-child" in sys.argv:
        _staged_child()
