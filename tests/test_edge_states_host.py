"""The inputs of tests/test_gpu_edge_states.py are what tests/edge_states.py claims, on the CPU oracle alone: a change of the recipe
that lets the GPU module compare a smooth state again shows here.  For every (hydraulics, ncol, Nz) that module uses: the oracle stays
valid over the 16 steps, stepping by hand equals timestep, the run reaches every edge the recipe is for, and the fp64 oracle follows
the wide oracle through the same regimes (so that the accuracy metric of the van Genuchten cases measures arithmetic, not flips)."""
import numpy as np
import pytest

import accuracy as A
import edge_states as E
import workloads as W
from test_gpu_interior_steps import SIGNATURES

HYDRAULICS = ("default", "vg")
STATUS_COMPOSITION = 2      # (oracle/terrarium_oracle.hpp: volumetric_fractions' bounds; TRM_STATUS_COMPOSITION of the library)


def _all_fields(o, names):
    return {n: np.array(o.get(n)) for n in names}


def _valid(o, names, label):
    assert o.status() == 0, label
    for n in names:
        assert np.all(np.isfinite(o.get(n))), (label, n)


def _run_both_ways(w, seen=None, prepare=None):
    """16 steps in the calls of E.CALLS with timestep and by hand: valid after every step, bit-identical after every call"""
    names = A.field_names(w)
    a, b = W.setup_oracle(w), W.setup_oracle(w)
    if prepare:
        prepare(w, [a, b])
    step = 0
    for nsteps, finalize in E.CALLS:
        for n in range(nsteps):
            fin = finalize and n == nsteps - 1
            a.timestep(w["dt"], fin)
            E.step_by_hand(b, w["dt"], fin, seen)
            step += 1
            _valid(a, names, f"step {step}")
        assert a.clock() == b.clock()
        for n in names:
            assert a.get(n).tobytes() == b.get(n).tobytes(), (step, n)
    assert step == E.NSTEPS
    return a


@pytest.mark.parametrize("ncol,Nz", E.SHAPES)
@pytest.mark.parametrize("hydraulics", HYDRAULICS)
def test_the_recipe_reaches_every_edge(hydraulics, ncol, Nz):
    w = E.edge_workload(hydraulics, Nz, ncol)
    assert set(w["kind"]) == set(range(E.KINDS))
    seen = dict.fromkeys(E.FEATURES, 0)
    o = _run_both_ways(w, seen)
    print(hydraulics, ncol, Nz, seen, "water tables", np.unique(o.get("water_table")).size)
    for feature in E.FEATURES:
        assert seen[feature] > 0, (feature, seen)
    assert o.get("saturation_water_ice").min() > 0                 # (the deficit pass of the repair is not reached from a legal state)
    assert np.count_nonzero(o.get("surface_excess_water") > 0) >= ncol // 2 - 1
    surface = o.grid()["zF"][-1]
    wt = o.get("water_table")
    assert np.all(wt[w["kind"] == 0] == surface)                   # kind 0 ends where it began: saturated to the surface


@pytest.mark.parametrize("ncol,Nz", E.SHAPES)
@pytest.mark.parametrize("hydraulics", HYDRAULICS)
def test_initial_states_are_the_table(hydraulics, ncol, Nz):
    """what initialize leaves per kind (the table of edge_states.py)"""
    w = E.edge_workload(hydraulics, Nz, ncol)
    o = W.setup_oracle(w)
    kind, sat, T, U, wt = w["kind"], o.get("saturation_water_ice"), o.get("temperature"), o.get("internal_energy"), o.get("water_table")
    zF = o.grid()["zF"]
    assert np.all(sat[:, kind == 0] == 1.0) and np.all(wt[kind == 0] == zF[-1])
    assert sat[:, kind == 1].max() <= 0.97 and np.all(wt[kind == 1] == zF[0])
    assert np.all(sat[E.pocket(Nz)][:, kind == 2] == 1.0) and np.count_nonzero(sat[:, kind == 2] == 1.0) == E.pocket(Nz).size * np.count_nonzero(kind == 2)
    assert np.all(sat[:, kind == 3] == 0.995)
    assert np.all(sat[:-1, kind == 4] == 1.0) and np.all(sat[-1, kind == 4] == 0.9) and np.all(wt[kind == 4] == zF[-2])
    assert np.all(sat[:, kind == 5] == E.DRY[hydraulics])
    assert np.all(T[:, kind == 6] == 0.0) and np.all(U[:, kind == 6] == 0.0) and not np.any(np.signbit(U[:, kind == 6]))
    assert np.all(T[0, kind == 7] == -0.5) and np.all(T[-1, kind == 7] == 0.5)
    flux = w["bcs"][("saturation_water_ice", "top")][1]
    assert np.all(flux[::2] == E.TOP_FLUX) and not np.any(flux[1::2])


@pytest.mark.skipif(A.wide_skip_reason() is not None, reason=str(A.wide_skip_reason()))
@pytest.mark.parametrize("ncol,Nz", E.SHAPES)
@pytest.mark.parametrize("hydraulics", HYDRAULICS)
def test_no_regime_flips_against_the_wide_oracle(hydraulics, ncol, Nz):
    """a condition on the inputs: the fp64 oracle and the wide oracle take the same branches (measured: 0 cells left out)"""
    w = A.rounded_workload(E.edge_workload(hydraulics, Nz, ncol))
    names = A.field_names(w)
    out = []
    for wide in (False, True):
        o = A.setup_oracle(w, wide=wide)
        for nsteps, finalize in E.CALLS:
            for n in range(nsteps):
                o.timestep(w["dt"], finalize and n == nsteps - 1)
        assert o.status() == 0
        out.append(A.fields_of(o, names))
    rows = A.compare(out[0], out[0], out[1], names, np.float64, label=f"edge {hydraulics} {ncol} x {Nz}: fp64 oracle against the wide oracle")
    for q in rows:
        assert q["left_out"] <= A.MAX_LEFT_OUT * q["cells"], (q["name"], q["left_out"], q["cells"])
        assert q["bad_nonfinite"] == 0, q["name"]


@pytest.mark.parametrize("extra,signature", SIGNATURES)
@pytest.mark.parametrize("hydraulics,ncol,Nz", E.SIGNATURE_SHAPES)
def test_every_signature_stays_valid(hydraulics, ncol, Nz, extra, signature):
    w = E.with_signature(E.edge_workload(hydraulics, Nz, ncol), extra)
    has_flux = ("saturation_water_ice", "top") in w["bcs"]
    assert has_flux == (signature == 34)
    _run_both_ways(w)


@pytest.mark.parametrize("config", ["heat", "richards"])
def test_energy_on_the_lower_kink(config):
    """U == -Lth exactly on every cell of kinds 6 and 7: the closure gives liq = 0 and T = 0 there, not the frozen branch"""
    ncol, Nz = E.KINK_SHAPE
    w = E.edge_workload("default", Nz, ncol, config=config)
    columns = np.flatnonzero((w["kind"] == 6) | (w["kind"] == 7))
    assert columns.size == 2

    def prepare(w, sides):
        U = E.put_energy_on_lower_kink(w, sides, columns)
        assert np.all(U[:, columns] < 0)
        for s in sides:
            assert np.all(s.get("liquid_water_fraction")[:, columns] == 0.0)
            assert np.all(s.get("temperature")[:, columns] == 0.0)
            # one ulp below the kink is the frozen branch: the upload sits on the kink, not beside it
            t = s.clone()
            t.set("internal_energy", np.nextafter(U, -np.inf))
            t.closure()
            assert np.all(t.get("temperature")[:, columns] < 0.0)

    _run_both_ways(w, prepare=prepare)


@pytest.mark.parametrize("ncol,Nz", E.STATUS_SHAPES)
def test_illegal_dry_workload(ncol, Nz):
    """where and when the oracle leaves the composition bounds (E.ILLEGAL_AT), and that only kind-5 columns go non-finite"""
    w = E.illegal_dry_workload(Nz, ncol)
    names = A.field_names(w)
    o = W.setup_oracle(w)
    first, step = None, 0
    finite = np.ones(ncol, dtype=bool)
    for nsteps, finalize in E.CALLS:
        for n in range(nsteps):
            o.timestep(w["dt"], finalize and n == nsteps - 1)
            step += 1
            if first is None and o.status() != 0:
                first = step
            if first is not None:
                assert o.status() == STATUS_COMPOSITION, step
    for n in names:
        x = o.get(n)
        finite &= np.isfinite(x).all(axis=0) if x.ndim == 2 else np.isfinite(x)
    assert first == E.ILLEGAL_AT[(ncol, Nz)]
    if first is None:
        assert finite.all()
        assert np.all(w["T0"][w["kind"] == 5] < 0)      # (every dry column of this shape is frozen: see illegal_dry_workload)
    else:
        assert set(w["kind"][~finite]) == {5}
        assert np.all(w["T0"][~finite] > 0) and np.all(w["T0"][(w["kind"] == 5) & finite] < 0)
