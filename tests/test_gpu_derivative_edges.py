"""Heat-only derivatives at the edges of the lane layouts, value by value against an exact Jacobian (tests/linearised_heat.py).

The depths are the smallest at which the lane mapping of the derivative kernels can go wrong: Nz = 2 and 3 (the bottom lane's
neighbour is the top lane, six steps cover the whole column), 31, 32 (the top cell on lanes 30 and 31 of the 32-lane layout), 33 (the
first depth of the 64-lane layout, the top cell on lane 32), 63 and 64 (no tail lanes, the top cell on lane 63).  13 columns: the last
wave of the 32-lane layout is half filled and the one workgroup is partly filled in both layouts; one column for Nz = 2 and 64.  The
grid is uniform, 0.1 m, where a seed moves its neighbours by far more than rounding.  Six steps of DT under steps_per_launch = 4:
launches of 4 and 2.

Every derivative the device forms -- tangents of a dense seed and of one-hot seeds on levels 0, Nz - 1, 31 and 32; tangents of boundary,
parameter and series-node seeds; the gradients of the per-step tape and of the checkpointed tape (K = 4) with respect to the initial
internal energy, the boundary values, the ten thermal parameters and the nodes of a series -- is compared with the extended-precision
Jacobian of the restatement, which owes nothing to the device: |dev - ref| / S, S = sum |J| |v| from the reference's Jacobian.  The
bound of a case is 8 x e_ref: e_ref is the same normalised difference between the float64 and the extended-precision evaluation of
the restatement itself, computed here on the CPU (`reference`), so no figure of the device enters the bound; 8 is what the project
grants a second evaluation order (M <= 8 in accuracy.py, 8 x err_tan in the transpose checks).  A bound above 1e-12 is refused as a
broken measurement.  Where S is zero (locality, a pair whose kind reads no value, a temperature in phase change) the device's value
must be 0.0.  Columns are compared unless the regime mask of linearised_heat.kept_columns drops them; test_linearised_heat_host.py
proves on the CPU that no case loses more than one, and prints e_ref of every case.

With it, what the suite states exactly elsewhere, at these depths: the primal after step_tangent and step_record is trm_step's bit for
bit, the checkpointed gradient is the per-step tape's bit for bit, and the layout is 32 lanes a column up to Nz = 32, 64 above."""
import functools

import numpy as np
import pytest

import linearised_heat as LH
import series_derivatives as S
import terrarium_jl_amd as trm
from boundary_derivatives import FD_DZ, HALOS, LD, PAIRS
from parameter_derivatives import PARAMS, RHO_SOC, thermal_params
from test_gpu_adjoint import cotangents
from test_gpu_tangent import DT, STATE, TANGENTS, bits, boundary_sets, mixed_state

pytestmark = pytest.mark.gpu

EDGE_SIZES = (2, 3, 31, 32, 33, 63, 64)
NH = 13
SHAPES = [(Nz, NH) for Nz in EDGE_SIZES] + [(2, 1), (64, 1)]
DZ = FD_DZ[0]
STEPS, SPL, K = 6, 4, 4
SETS = ("T_top+flux_bottom", "flux_top+T_bottom", "gradient_top+flux_bottom")
# the seriesed pair of the two sets that may carry a series: a Value and a Flux, both on the top lane -- 31, 32 or 63 at these depths
SERIES_PAIR = {"T_top+flux_bottom": ("temperature", "top"), "flux_top+T_bottom": ("internal_energy", "top")}
FACTOR, BROKEN = 8.0, 1e-12

# (Nz, Nh, boundary set, halo policy, rho_soc, time indexing of the series or None)
BASE_CASES = [(Nz, Nh, bcset, halo, rho, None) for Nz, Nh in SHAPES for bcset in SETS for halo in HALOS for rho in RHO_SOC]
SERIES_CASES = [(Nz, Nh, bcset, halo, 0.0, S.FD_INDEXINGS[(n + m + h) % 3]) for n, (Nz, Nh) in enumerate(SHAPES)
                for m, bcset in enumerate(SERIES_PAIR) for h, halo in enumerate(HALOS)]
CASES = BASE_CASES + SERIES_CASES


def case_id(case):
    Nz, Nh, bcset, halo, rho, indexing = case
    return f"Nz{Nz}-Nh{Nh}-{bcset}-{halo}-rho{rho:g}" + (f"-{indexing}" if indexing else "")


def one_hot_levels(Nz):
    return sorted({0, Nz - 1} | ({31, 32} if Nz >= 33 else set()))


# ---- the inputs of a case ------------------------------------------------------------------------------------------------------------
# The seed of mixed_state per shape: the first from 1 up with which, in every case of the shape, the regime mask keeps every column, the
# kept columns hold all three regimes, and 8 x e_ref stays under 1e-12 (a frozen cell close to -L_theta loses digits in U + L_theta in any
# fp64 evaluation; with enough of them e_ref itself outgrows the ceiling).  All three are properties of the reference alone and are
# asserted in test_linearised_heat_host.py.
STATE_SEEDS = {(2, 13): 3, (2, 1): 2}


def state_seed(case):
    return STATE_SEEDS.get((case[0], case[1]), 1)


def inputs(case):
    """(p, U0, sat, bcs, series, vectors): vectors are the seeds and cotangents every contraction of the case uses"""
    Nz, Nh, bcset, halo, rho, indexing = case
    p = thermal_params(halo, rho)
    U0, sat = mixed_state(Nz, Nh, p, seed=state_seed(case))
    bcs = {pair: (kind, np.broadcast_to(np.asarray(value, dtype=np.float64), (Nh,)).copy()) for pair, (kind, value) in boundary_sets(Nh)[bcset].items()}
    series = S.series_on(bcs, [SERIES_PAIR[bcset]], indexing, Nh) if indexing else {}
    rng = np.random.default_rng(1000 + state_seed(case))
    w = cotangents(Nz, Nh, 41)
    vectors = {
        "state": rng.normal(0.0, 1e3, (Nz, Nh)),
        "boundary": rng.normal(0.0, 1.0, (len(PAIRS), Nh)),                                      # K, K/m, W/m2
        "params": np.array([getattr(p, name) for name in PARAMS]) * rng.uniform(0.5, 1.5, len(PARAMS)) * rng.choice([-1.0, 1.0], len(PARAMS)),
        "series": rng.normal(0.0, 1.0, (S.NT, Nh)),
        "cotangents": np.stack([w[x] for x in TANGENTS]),
    }
    return p, U0, sat, bcs, series, vectors


def restatement(case, dtype):
    p, U0, sat, bcs, series, _ = inputs(case)
    return LH.run([DZ] * case[0], U0, sat, bcs, p, DT, STEPS, dtype=dtype, mirror=case[3] == "mirror", series=series)


def blocks(result, case):
    """{input: dX_n / d(input) stacked over the three fields}: state [3][Nz][Nz][Nh], boundary [3][Nz][4][Nh] (zeros for a pair the set
    does not hold or that carries the series), params [3][Nz][10][Nh], series [3][Nz][nt][Nh]"""
    out = {"state": np.stack([result.block("state")[x] for x in TANGENTS]), "params": np.stack([result.block("params")[x] for x in TANGENTS])}
    per_pair = [result.block(("boundary", pair)) for pair in PAIRS]
    out["boundary"] = np.stack([np.stack([b[x] for b in per_pair], axis=1) for x in TANGENTS])
    if case[5]:
        out["series"] = np.stack([result.block(("series", SERIES_PAIR[case[2]]))[x] for x in TANGENTS])
    return out


def contractions(case, vectors):
    """{label: (input, vector, einsum axes)}: every product of the Jacobian the device is asked for.  Tangents come back per field and
    cell, gradients per input."""
    Nz, Nh = case[0], case[1]
    out = {"tangent dense": ("state", vectors["state"], "xijc,jc->xic")}
    for j in one_hot_levels(Nz):
        e = np.zeros((Nz, Nh))
        e[j] = 1.0
        out[f"tangent one-hot {j}"] = ("state", e, "xijc,jc->xic")
    w = vectors["cotangents"]
    out["gradient state"] = ("state", w, "xijc,xic->jc")
    if case[5]:
        out["tangent series"] = ("series", vectors["series"], "xinc,nc->xic")
        out["gradient series"] = ("series", w, "xinc,xic->nc")
    else:
        out["tangent boundary"] = ("boundary", vectors["boundary"], "xipc,pc->xic")
        out["tangent params"] = ("params", vectors["params"], "xiqc,q->xic")
        out["gradient boundary"] = ("boundary", w, "xipc,xic->pc")
        out["gradient params"] = ("params", w, "xiqc,xic->qc")
    return out


class Reference:
    """The reference of a case, computed once on the CPU: inputs, the kept columns, the regimes over the run, per contraction (ref, S) in
    extended precision and its e_ref, and e_ref of the case (the largest).  The Jacobians themselves are not kept."""

    def __init__(self, case):
        self.case = case
        self.inputs = inputs(case)
        wide, narrow = restatement(case, LD), restatement(case, np.float64)
        self.keep = LH.kept_columns(wide, narrow)
        self.regimes = np.stack(wide.regimes)
        J_wide, J_narrow = blocks(wide, case), blocks(narrow, case)
        self.expected, self.parts = {}, {}
        for label, (key, v, axes) in contractions(case, self.inputs[5]).items():
            err, ref, Ssum = LH.contraction_error(J_narrow[key][..., self.keep], J_wide[key][..., self.keep], v[..., self.keep] if v.ndim > 1 else v, axes)
            self.expected[label], self.parts[label] = (ref, Ssum), err
        self.e_ref = max(self.parts.values())

    def bound(self):
        b = FACTOR * self.e_ref
        assert 0.0 < b <= BROKEN, (case_id(self.case), "e_ref is no measurement of fp64 rounding", self.e_ref)
        return b

    def error(self, label, dev):
        """|dev - ref| / S of a device result shaped like the contraction, on the kept columns; exact zeros where S is zero"""
        ref, Ssum = self.expected[label]
        dev = np.asarray(dev)[..., self.keep]
        zero = Ssum == 0
        assert np.all(dev[zero] == 0.0), (case_id(self.case), label, "non-zero where the reference is exactly zero")
        return 0.0 if zero.all() else float(np.max(np.abs(dev.astype(LD) - ref)[~zero] / Ssum[~zero]))


@functools.lru_cache(maxsize=None)
def reference(case):
    """shared by the two tests of a case (and by test_linearised_heat_host.py); nothing in it is modified later"""
    return Reference(case)


# ---- the device ----------------------------------------------------------------------------------------------------------------------
def device(case, steps_per_launch=SPL):
    Nz, Nh = case[0], case[1]
    p, U0, sat, bcs, series, _ = inputs(case)
    d = trm.DeviceState(trm.ColumnGrid(trm.PrescribedSpacing(dz=[DZ] * Nz), Nh), p)
    d.set_option("steps_per_launch", steps_per_launch)
    d.set("saturation_water_ice", sat)
    d.set("internal_energy", U0)
    for (var, side), (kind, value) in bcs.items():
        d.set_bc(var, side, kind, value)
    d.closure()
    if series:
        S.attach(d, series)
        d.set_option("derivative_series", 1)
    d.save_state()
    return d


def stepped_twin(case):
    """the state trm_step leaves, under the library's own choice of program"""
    b = device(case, steps_per_launch=0)
    b.step(DT, STEPS, finalize=True)
    return {name: bits(b.get(name)) for name in STATE}, b.status(), b.clock()


def assert_primal(d, twin, case, family):
    state, status, clock = twin
    for name in STATE:
        assert np.array_equal(bits(d.get(name)), state[name]), (case_id(case), family, name)
    assert d.status() == status and d.clock() == clock
    prog = d.last_program()
    assert prog["family"] == family and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64), (case_id(case), prog)


def tangents(d, dU, boundary=None, params=None, series=None):
    """the three tangents stacked, of the saved state under the given seeds; a fresh open_tangent zeroes every other seed"""
    d.restore_state()
    d.open_tangent()
    d.set_tangent("internal_energy", dU)
    if boundary is not None:
        for pair, values in zip(PAIRS, boundary):
            d.set_bc_tangent(*pair, values)
    if params is not None:
        d.set_param_tangent(dict(zip(PARAMS, params)))
    for pair, values in (series or {}).items():
        d.set_bc_series_tangent(*pair, values)
    d.step_tangent(DT, STEPS)
    prog = d.last_program()
    assert prog["boundary_seeds"] == (boundary is not None or params is not None or bool(d.get_option("info_derivative_series")))
    assert prog["parameter_seeds"] == (params is not None)
    return np.stack([d.tangent(x) for x in TANGENTS])


def gradients(d, w, ride, checkpoint_every=None, series_pair=None):
    """{input: gradient} of the saved state: records the run on a fresh tape and pulls the cotangents back.  ride: "state" (dL/dU_0
    alone), "boundary" (with the four boundary values), "params" (with those and the ten thermal parameters), "series" (the nodes)"""
    d.restore_state()
    d.open_adjoint(STEPS, checkpoint_every)
    if ride == "boundary":
        d.open_bc_gradient()
    if ride == "params":
        d.open_param_gradient()
    d.step_record(DT, STEPS)
    recorded = {name: bits(d.get(name)) for name in STATE}, d.status(), d.clock(), d.last_program()
    for x, wx in zip(TANGENTS, w):
        d.set_cotangent(x, wx)
    d.adjoint_backward()
    prog = d.last_program()
    assert prog["backward"] and prog["checkpointed"] == (checkpoint_every is not None)
    out = {"state": d.cotangent("internal_energy")}
    if ride in ("boundary", "params"):
        out["boundary"] = np.stack([d.bc_gradient(*pair) for pair in PAIRS])
    if ride == "params":
        out["params"] = np.stack([d.param_gradient(name) for name in PARAMS])
    if ride == "series":
        out["series"] = d.bc_series_gradient(*series_pair)
    d.close_adjoint()
    return out, recorded


def report(ref, figures):
    bound = ref.bound()
    worst = max(figures.values())
    print(f"{case_id(ref.case)}: e_ref = {ref.e_ref:.3e}, bound = {bound:.3e}, device = {worst:.3e}, kept {int(ref.keep.sum())}/{ref.keep.size}")
    for label, err in figures.items():
        print(f"    {label}: device = {err:.3e}, e_ref = {ref.parts[label.split(' [')[0]]:.3e}")
    over = {label: err for label, err in figures.items() if not err <= bound}
    assert not over, (case_id(ref.case), f"bound {bound:.3e}", over)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tangents_match_the_exact_jacobian(case):
    ref = reference(case)
    vectors = ref.inputs[5]
    d = device(case)
    figures = {}
    for label, (key, v, _) in contractions(case, vectors).items():
        if not label.startswith("tangent"):
            continue
        zero = np.zeros((case[0], case[1]))
        if key == "state":
            t = tangents(d, v)
        elif key == "boundary":
            t = tangents(d, zero, boundary=v)
        elif key == "params":
            t = tangents(d, zero, params=v)
        else:
            t = tangents(d, zero, series={SERIES_PAIR[case[2]]: v})
        figures[label] = ref.error(label, t)
        if label == "tangent dense":
            assert_primal(d, stepped_twin(case), case, "column_tangent")
    report(ref, figures)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradients_match_the_exact_jacobian(case):
    ref = reference(case)
    w = ref.inputs[5]["cotangents"]
    d = device(case)
    twin = stepped_twin(case)
    rides = ("series",) if case[5] else ("state", "boundary", "params")
    figures = {}
    for ride in rides:
        per_step, recorded = gradients(d, w, ride, series_pair=SERIES_PAIR.get(case[2]))
        state, status, clock, prog = recorded
        for name in STATE:                                                       # the recorded primal is trm_step's
            assert np.array_equal(state[name], twin[0][name]), (case_id(case), ride, name)
        assert (status, clock) == twin[1:]
        assert prog["family"] == "column_adjoint" and prog["lanes_per_column"] == (32 if case[0] <= 32 else 64)
        checkpointed, _ = gradients(d, w, ride, checkpoint_every=K, series_pair=SERIES_PAIR.get(case[2]))
        for key, g in per_step.items():
            assert np.array_equal(bits(checkpointed[key]), bits(g)), (case_id(case), ride, key, "checkpointed against per-step")
            figures[f"gradient {key} [{ride}]"] = ref.error(f"gradient {key}", g)
    report(ref, figures)
