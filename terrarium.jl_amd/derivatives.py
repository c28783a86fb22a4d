"""Derivatives of the heat-only SoilModel run through a `ModelIntegrator`: forward-mode tangents (`jvp`, `record_jvp`), reverse-mode
gradients (`vjp`) and the misfit to a temperature record with its gradient (`misfit_gradient`, `record_gradient`,
`record_normal_equations`).  `jvp` also covers the heat + Richards run, with seeds on the initial internal energy and saturation
(the option `derivative_richards`), and so does `vjp`, with cotangents of the five final fields on the per-step tape (the option
`derivative_richards_adjoint`).  The drivers issue the calls of `DeviceState` (trm_tangent_*, trm_adjoint_*); the two skeletons they
share are `_tangent_run` and `_taped`."""
from contextlib import ExitStack, contextmanager

import numpy as np

from . import _capi
from .io import RasterInputSource
from .integrator import FieldTimeSeries, ForwardEuler, ModelIntegrator, checkpoint, restore
from .models import RichardsEq

# the (variable, side) pairs whose boundary value the heat-only step reads, and the kinds that read it
_BOUNDARY_DERIVATIVE_KINDS = {"temperature": ("value", "gradient"), "internal_energy": ("flux",)}
_COTANGENTS = ("internal_energy", "temperature", "liquid_water_fraction")


def _series_driven(integ, var, side):
    """The boundary condition on (var, side) is a device-resident time series: a FieldTimeSeries or a time-indexed raster source."""
    value = integ.boundary_conditions.get((var, side), (None, None))[1]
    return isinstance(value, FieldTimeSeries) or (isinstance(value, RasterInputSource) and not value.static)


class _derivative_series:
    """Sets the option `derivative_series` for the duration of a jvp / vjp call where a boundary series drives the run, and
    `derivative_series_params` with it where the call carries thermal-parameter seeds or asks for their gradient (`params`)."""

    def __init__(self, integ, params=False):
        self.st = integ.state
        self.wanted = any(_series_driven(integ, var, side) for var, side in integ.boundary_conditions)
        self.params = self.wanted and bool(params)

    def __enter__(self):
        self.before = self.st.get_option("derivative_series")
        self.before_params = self.st.get_option("derivative_series_params")
        if self.wanted:
            self.st.set_option("derivative_series", 1)
        if self.params:
            self.st.set_option("derivative_series_params", 1)
        return self

    def __exit__(self, *exc):
        if self.params:
            self.st.set_option("derivative_series_params", self.before_params)
        if self.wanted:
            self.st.set_option("derivative_series", self.before)
        return False


def _refuse_uncovered(integ, who):
    """What every driver refuses before it touches the state."""
    if not isinstance(integ.timestepper, ForwardEuler):
        raise ValueError(f"{who}: ForwardEuler only")
    if integ._has_time_dependence() or integ._windowed():
        raise ValueError(f"{who}: boundary conditions and inputs must be constant over the run")


class _derivative_richards:
    """Sets the option `derivative_richards` for the duration of a jvp call on a heat + Richards integrator -- for a vjp call,
    `option` = `derivative_richards_adjoint`."""

    def __init__(self, integ, option="derivative_richards"):
        self.st = integ.state
        self.option = option
        self.wanted = _richards(integ)

    def __enter__(self):
        if self.wanted:      # (a heat-only run makes the calls it always made)
            self.before = self.st.get_option(self.option)
            self.st.set_option(self.option, 1)
        return self

    def __exit__(self, *exc):
        if self.wanted:
            self.st.set_option(self.option, self.before)
        return False


def _richards(integ):
    """The integrator's model has RichardsEq (read off the model, not the state: a heat-only run makes the calls it always made)."""
    hydrology = getattr(getattr(getattr(integ, "model", None), "soil", None), "hydrology", None)
    return isinstance(getattr(hydrology, "vertical_flow", None), RichardsEq)


def _tangent_run(integ, steps, d_internal_energy, d_boundary, d_params, record, result, d_saturation=None):
    """The tangent drivers: opens the tangent unless it is open, sets the series options, seeds U, the boundary pairs and the
    parameters, attaches `record` = (positions, levels) if one is given, steps, and returns `result(state)`.  On the way out it closes
    the tangent if it opened it, and otherwise detaches the record it attached."""
    st = integ.state
    with _derivative_richards(integ):
        return _tangent_run_open(integ, st, steps, d_internal_energy, d_boundary, d_params, record, result, d_saturation)


def _tangent_run_open(integ, st, steps, d_internal_energy, d_boundary, d_params, record, result, d_saturation):
    opened = not getattr(st, "_tangent_open", False)
    if opened:
        st.open_tangent()
    attached = False
    try:
        with _derivative_series(integ, params=d_params is not None):
            st.set_tangent("internal_energy", d_internal_energy)
            if _richards(integ):
                st.set_tangent("saturation", 0.0 if d_saturation is None else d_saturation)
            for (var, side), values in (d_boundary or {}).items():
                if _series_driven(integ, var, side):
                    st.set_bc_series_tangent(var, side, values)
                else:
                    st.set_bc_tangent(var, side, values)
            if d_params is not None:
                st.set_param_tangent(d_params)
            if record is not None:
                st.attach_tangent_record(*record)
                attached = True
            st.step_tangent(integ.timestepper.dt, steps)
            return result(st)
    finally:
        if opened:
            st.close_tangent()
        elif attached:
            st.detach_tangent_record()


@contextmanager
def _taped(integ, slots, K, wrt_params, reuse=False, detach=False):
    """The adjoint drivers: a tape of `slots` slots (checkpointed every K; None: one slot per step) and the series options for the
    duration of the block, which gets the state.  The tape is opened anew -- with `reuse`, only where none is open or the open one
    has another shape or holds steps.  On the way out the adjoint is closed if the driver opened it; otherwise, with `detach`, the
    attached record is detached."""
    st = integ.state
    opened = not getattr(st, "_adjoint_open", False)
    if opened or not reuse or st.adjoint_checkpoints() != (K or 0, 0, slots):
        st.open_adjoint(slots, K)
    try:
        with _derivative_series(integ, params=wrt_params):
            yield st
    finally:
        if opened:
            st.close_adjoint()
        elif detach:
            st.detach_record()


def _arm_sweep(st, cotangents, wrt_boundary, wrt_params):
    """In front of adjoint_backward: the cotangents of the final U, T and liq, and the accumulators that ride along."""
    for name, w in zip(_COTANGENTS, cotangents):
        st.set_cotangent(name, 0.0 if w is None else w)
    if wrt_boundary:
        st.open_bc_gradient()
    if wrt_params:
        st.open_param_gradient()


def _sweep_gradients(integ, st, wrt_boundary, wrt_params):
    """Behind adjoint_backward: [dL/dU_0], then the boundary / series dict, then the parameter dict."""
    out = [st.cotangent("internal_energy")]
    if wrt_boundary:
        pairs = [(var, side) for (var, side), (kind, _) in integ.boundary_conditions.items() if kind in _BOUNDARY_DERIVATIVE_KINDS.get(var, ())]
        out.append({(var, side): st.bc_series_gradient(var, side) if _series_driven(integ, var, side) else st.bc_gradient(var, side)
                    for var, side in pairs})
    if wrt_params:
        out.append({name: st.param_gradient(name) for name in _capi.THERMAL_PARAMS})
    return out


def jvp(integ: ModelIntegrator, d_internal_energy, steps: int, d_boundary=None, d_params=None) -> dict:
    """Forward-mode derivative of `run!(integ; steps)` with respect to the initial internal energy: the integrator is stepped `steps`
    times with its own dt, its state carrying the tangent seeded by `d_internal_energy` ([Nz][Nh], or anything that broadcasts to
    it).  Returns {"internal_energy", "temperature", "liquid_water_fraction"}: the tangents of those fields after the last step.
    `d_boundary` = {(var, side): values}: seeds d(value) of boundary conditions, [Nh] or a scalar each -- a Value or a Gradient on
    `temperature`, a Flux on `internal_energy` -- held over the run like the values themselves (trm_tangent_bc_upload).
    For a pair driven by a `FieldTimeSeries` or a time-indexed raster source the seeds have the series' shape, [nt][Nh]: d(node value)
    of every node of the record (trm_tangent_bc_series_upload); the option `derivative_series` is set for the duration of the call.
    `d_params` = {name: value}: seeds on the thermal parameters (`k_mineral`, `c_water`, ...: trm_tangent_param_set).  They go together
    with a boundary series, and with seeds on its nodes, in one run: the option `derivative_series_params` is set for the duration of
    the call as well.
    The heat-only SoilModel in fp64 with ForwardEuler and boundary conditions that are constant over the run or whole-record time
    series (trm_step_tangent); callables, state functions and windowed sources are refused.
    On an integrator with `RichardsEq` (heat + Richards, the branch-free boundary kinds, constant boundary values) the seeds are the
    state's: `d_internal_energy` may be a dict {"internal_energy": dU, "saturation": dsat} (each [Nz][Nh], or anything that broadcasts
    to it; one left out is zero) -- a plain value seeds the internal energy alone -- and the result holds five tangents: `saturation`
    and `pressure_head` beside the three above.  The option `derivative_richards` is set for the duration of the call.  `d_boundary`
    and `d_params` are refused there; a saturation seed on a heat-only integrator raises a ValueError (its saturation is a constant)."""
    _refuse_uncovered(integ, "jvp")
    d_saturation = None
    if isinstance(d_internal_energy, dict):
        unknown = sorted(set(d_internal_energy) - {"internal_energy", "saturation"})
        if unknown:
            raise KeyError(f"jvp: no state seed {unknown[0]!r} (internal_energy, saturation)")
        d_saturation = d_internal_energy.get("saturation")
        d_internal_energy = d_internal_energy.get("internal_energy", 0.0)
    if d_saturation is not None and not _richards(integ):
        raise ValueError("jvp: saturation seeds need an integrator with RichardsEq (the heat-only run keeps its saturation)")
    # (the tangent fields a context holds are the ids below a count: tangent_fields, trm_derivative_api.hip)
    count = _capi.TANGENT["pressure_head" if _richards(integ) else "liquid_water_fraction"] + 1
    names = [name for name, which in _capi.TANGENT.items() if which < count]
    return _tangent_run(integ, int(steps), d_internal_energy, d_boundary, d_params, None,
                        lambda st: {name: st.tangent(name) for name in names}, d_saturation)


def record_jvp(integ: ModelIntegrator, positions, levels, d_internal_energy=0.0, d_boundary=None, d_params=None, steps=None):
    """`jvp` sampled at a record's positions: the integrator is stepped `steps` times (None: to the last position) with its own dt,
    and the temperature and its tangent are stored on `levels` behind the steps `positions` lists (step counts, strictly increasing,
    0 = the initial state) inside the tangent launches -- one attach and one step_tangent (trm_tangent_record_attach).  Returns
    (T, dT), each [npos][nlevels][Nh]: the model's samples and J v at the samples for the seeds v = (`d_internal_energy`,
    `d_boundary`, `d_params`) of `jvp`.  Zero seeds give the record the model itself produces.  State and clock end where `run`
    leaves them.  Coverage, refusals and option handling of `jvp`."""
    _refuse_uncovered(integ, "record_jvp")
    positions = [int(q) for q in np.asarray(positions).reshape(-1)]
    if not positions or positions[0] < 0 or any(b <= a for a, b in zip(positions, positions[1:])):
        raise ValueError("record_jvp: the positions must be >= 0 and strictly increasing, one sample per position")
    steps = positions[-1] if steps is None else int(steps)
    return _tangent_run(integ, steps, d_internal_energy, d_boundary, d_params, (positions, levels),
                        lambda st: (st.tangent_record("temperature"), st.tangent_record("tangent")))


def vjp(integ: ModelIntegrator, steps: int, temperature=None, internal_energy=None, liquid_water_fraction=None,
        checkpoint_every=None, wrt_boundary=False, wrt_params=False):
    """Reverse-mode derivative of `run!(integ; steps)`: the integrator is stepped `steps` times with its own dt (state and clock end
    where `run` leaves them), then the given cotangents of the final temperature, internal energy and liquid water fraction ([Nz][Nh],
    or anything that broadcasts to it; None: zero) are pulled back.  Returns dL/dU_0 as [Nz][Nh], L the sum of the three inner
    products.  One tape slot per step (trm_step_record, trm_adjoint_backward); with `checkpoint_every` = K one slot per K steps, the
    states in between formed again by the backward sweep -- the same gradient bit for bit.  The coverage and refusals of `jvp`.
    With `wrt_boundary` it returns (dL/dU_0, {(var, side): dL/d(value) as [Nh]}) for the boundary conditions of the integrator whose
    value the run reads -- a Value or a Gradient on `temperature`, a Flux on `internal_energy` -- from the same sweep
    (trm_adjoint_bc_open); a pair driven by a `FieldTimeSeries` or a time-indexed raster source gets dL/d(node value) as [nt][Nh], the
    shape of its record (trm_adjoint_bc_series_download; the option `derivative_series` is set for the duration of the call).
    With `wrt_params` it appends {name: dL/d(parameter) as [Nh]} for the ten thermal parameters, each column's
    share (trm_adjoint_param_open): (dL/dU_0, params), or (dL/dU_0, boundary, params) with `wrt_boundary` as well.  On a run driven by
    a boundary series too: one sweep gives dL/dU_0, the node gradients and the ten parameter gradients (the option
    `derivative_series_params` is set for the duration of the call).
    On an integrator with `RichardsEq` (what `jvp` covers there) the cotangents are the five final fields': `internal_energy` may be a
    dict {"internal_energy": wU, "saturation": wsat, "temperature": wT, "liquid_water_fraction": wliq, "pressure_head": wpsi} (each
    [Nz][Nh], or anything that broadcasts to it; one left out is zero; `temperature` and `liquid_water_fraction` may also come as the
    arguments above) and the result is {"internal_energy": dL/dU_0, "saturation": dL/dsat_0}, L the sum of the five inner products:
    the transpose of `jvp` there.  The option `derivative_richards_adjoint` is set for the duration of the call.  `checkpoint_every`,
    `wrt_boundary` and `wrt_params` raise a ValueError there; a `saturation` or `pressure_head` cotangent on a heat-only integrator
    raises a ValueError (neither field is a function of the initial internal energy)."""
    _refuse_uncovered(integ, "vjp")
    saturation = pressure_head = None
    if isinstance(internal_energy, dict):
        given = dict(internal_energy)
        unknown = sorted(set(given) - set(_capi.ADJOINT))
        if unknown:
            raise KeyError(f"vjp: no cotangent {unknown[0]!r} ({', '.join(_capi.ADJOINT)})")
        if ("temperature" in given and temperature is not None) or ("liquid_water_fraction" in given and liquid_water_fraction is not None):
            raise ValueError("vjp: a cotangent is given twice, as an argument and in the dict")
        temperature, liquid_water_fraction = given.get("temperature", temperature), given.get("liquid_water_fraction", liquid_water_fraction)
        saturation, pressure_head, internal_energy = given.get("saturation"), given.get("pressure_head"), given.get("internal_energy")
    if _richards(integ):
        for name, value in (("checkpoint_every", checkpoint_every is not None), ("wrt_boundary", wrt_boundary), ("wrt_params", wrt_params)):
            if value:
                raise ValueError(f"vjp: no {name} on an integrator with RichardsEq (final-state cotangents on a per-step tape only)")
        steps = int(steps)
        with _derivative_richards(integ, "derivative_richards_adjoint"), _taped(integ, max(steps, 1), None, False, reuse=True) as st:
            st.step_record(integ.timestepper.dt, steps)
            for name, w in zip(_capi.ADJOINT, (internal_energy, temperature, liquid_water_fraction, saturation, pressure_head)):
                st.set_cotangent(name, 0.0 if w is None else w)
            st.adjoint_backward()
            return {name: st.cotangent(name) for name in ("internal_energy", "saturation")}
    if saturation is not None or pressure_head is not None:
        raise ValueError("vjp: saturation and pressure_head cotangents need an integrator with RichardsEq (the heat-only run keeps its saturation)")
    steps = int(steps)
    K = None if checkpoint_every is None else int(checkpoint_every)
    slots = max(steps, 1) if K is None else max(-(-steps // max(K, 1)), 1)
    with _taped(integ, slots, K, wrt_params, reuse=True) as st:
        st.step_record(integ.timestepper.dt, steps)
        _arm_sweep(st, (internal_energy, temperature, liquid_water_fraction), wrt_boundary, wrt_params)
        st.adjoint_backward()
        out = _sweep_gradients(integ, st, wrt_boundary, wrt_params)
        return tuple(out) if len(out) > 1 else out[0]


def hydraulic_parameter_gradient(integ: ModelIntegrator, steps: int, cotangents: dict):
    """`vjp` on an integrator with `RichardsEq`, with the gradients with respect to the seven hydraulic parameters from the same sweep:
    the integrator is stepped `steps` times with its own dt, then `cotangents` -- the dict `vjp` takes there, {"internal_energy": wU,
    "saturation": wsat, "temperature": wT, "liquid_water_fraction": wliq, "pressure_head": wpsi}, one left out is zero -- are pulled
    back.  Returns ({"internal_energy": dL/dU_0, "saturation": dL/dsat_0}, {name: dL/d(parameter) as [Nh]}) for the names `K_sat`,
    `theta_res`, `bc_psi_s`, `bc_lambda`, `vg_alpha`, `vg_n`, `impedance`: each column's share, their sum the gradient of the scalar L
    (trm_adjoint_param_open under TRM_OPT_DERIVATIVE_RICHARDS_PARAMS).  A parameter the model's hydraulics never read gives zeros.  The
    state gradients are bit for bit `vjp`'s.  The options `derivative_richards_adjoint` and `derivative_richards_params` are set for the
    duration of the call.  The coverage of `vjp` there; an integrator without `RichardsEq` raises a ValueError."""
    _refuse_uncovered(integ, "hydraulic_parameter_gradient")
    if not _richards(integ):
        raise ValueError("hydraulic_parameter_gradient: needs an integrator with RichardsEq (the heat-only run reads no hydraulic parameter)")
    given = dict(cotangents)
    unknown = sorted(set(given) - set(_capi.ADJOINT))
    if unknown:
        raise KeyError(f"hydraulic_parameter_gradient: no cotangent {unknown[0]!r} ({', '.join(_capi.ADJOINT)})")
    steps = int(steps)
    with _derivative_richards(integ, "derivative_richards_adjoint"), _derivative_richards(integ, "derivative_richards_params"), \
            _taped(integ, max(steps, 1), None, False, reuse=True) as st:
        st.step_record(integ.timestepper.dt, steps)
        for name in _capi.ADJOINT:
            w = given.get(name)
            st.set_cotangent(name, 0.0 if w is None else w)
        st.open_param_gradient()
        st.adjoint_backward()
        return ({name: st.cotangent(name) for name in ("internal_energy", "saturation")},
                {name: st.param_gradient(name) for name in _capi.HYDRAULIC_PARAMS})


class TemperatureRecord:
    """A temperature record as a borehole logger leaves it: `values[nobs][nlevels][Nh]` at the step counts `steps` (non-decreasing,
    0 = the initial state) on the rows `levels` of the host layout (row 0 = bottom layer, strictly increasing).  `weight` >= 0
    broadcasts to the shape of `values` (None: 1); a NaN in `values` is a gap and counts for nothing."""

    def __init__(self, steps, levels, values, weight=None):
        self.steps = [int(s) for s in np.asarray(steps).reshape(-1)]
        self.levels = np.ascontiguousarray(levels, dtype=np.int32).reshape(-1)
        self.values = np.asarray(values, dtype=np.float64)
        if self.values.ndim != 3 or self.values.shape[:2] != (len(self.steps), self.levels.size):
            raise ValueError("TemperatureRecord: values must be [len(steps)][len(levels)][Nh]")
        if any(s < 0 for s in self.steps) or any(b < a for a, b in zip(self.steps, self.steps[1:])):
            raise ValueError("TemperatureRecord: steps must be >= 0 and non-decreasing")
        self.weight = None if weight is None else np.broadcast_to(np.asarray(weight, dtype=np.float64), self.values.shape)


class SoilMoistureRecord(TemperatureRecord):
    """A soil-moisture record as a probe logs it: `values[nobs][nlevels][Nh]` are saturations (saturation_water_ice, 0 ... 1) at the
    step counts `steps` (non-decreasing, 0 = the initial state) on the rows `levels` of the host layout (row 0 = bottom layer, strictly
    increasing).  `weight` >= 0 broadcasts to the shape of `values` (None: 1); a NaN in `values` is a gap and counts for nothing.  The
    shape rules of `TemperatureRecord`; read by `soil_moisture_gradient` (the option `derivative_richards_record`)."""

    def __init__(self, steps, levels, values, weight=None):
        try:
            super().__init__(steps, levels, values, weight)
        except ValueError as err:
            raise ValueError(str(err).replace("TemperatureRecord", "SoilMoistureRecord")) from None


def soil_moisture_gradient(integ: ModelIntegrator, record: SoilMoistureRecord, steps=None, cotangents=None, wrt_params=False):
    """The misfit L = sum_k sum_levels 1/2 w (sat_{steps_k} - values_k)^2 of `run!(integ; steps)` to a soil-moisture record, per column,
    and the gradient of L plus the final cotangents, on an integrator with `RichardsEq`: one attach, one step_record(dt, steps) and one
    sweep, the record read inside the backward launches (trm_adjoint_observe_record under TRM_OPT_DERIVATIVE_RICHARDS_RECORD).  The
    integrator is stepped `steps` times (None: to the last observation) with its own dt.  `cotangents` is the dict `vjp` takes there
    (None: all zero).  Returns (L as [Nh], {"internal_energy": dL/dU_0, "saturation": dL/dsat_0}) and, with `wrt_params`, a third item
    {name: dL/d(parameter) as [Nh]} for the seven hydraulic parameters of `hydraulic_parameter_gradient`.  The options
    `derivative_richards_adjoint`, `derivative_richards_record` and, with `wrt_params`, `derivative_richards_params` are set for the
    duration of the call.  `record.steps` must be strictly increasing (one sample per position) and none may lie behind `steps`,
    otherwise ValueError, as from `record_gradient`; an integrator without `RichardsEq` raises a ValueError.  The coverage of `vjp`."""
    _refuse_uncovered(integ, "soil_moisture_gradient")
    if not _richards(integ):
        raise ValueError("soil_moisture_gradient: needs an integrator with RichardsEq (the heat-only run keeps its saturation)")
    if not record.steps or any(b <= a for a, b in zip(record.steps, record.steps[1:])):
        raise ValueError("soil_moisture_gradient: the record's steps must be strictly increasing, one sample per position")
    last = record.steps[-1]
    steps = last if steps is None else int(steps)
    if steps < last:
        raise ValueError("soil_moisture_gradient: the record has observations behind the last step")
    given = dict(cotangents or {})
    unknown = sorted(set(given) - set(_capi.ADJOINT))
    if unknown:
        raise KeyError(f"soil_moisture_gradient: no cotangent {unknown[0]!r} ({', '.join(_capi.ADJOINT)})")
    with ExitStack() as options:
        for name in ("derivative_richards_adjoint", "derivative_richards_record") + (("derivative_richards_params",) if wrt_params else ()):
            options.enter_context(_derivative_richards(integ, name))
        with _taped(integ, max(steps, 1), None, False, detach=True) as st:
            st.attach_record(record.steps, record.levels, record.values, record.weight)
            st.step_record(integ.timestepper.dt, steps)
            for name in _capi.ADJOINT:
                w = given.get(name)
                st.set_cotangent(name, 0.0 if w is None else w)
            if wrt_params:
                st.open_param_gradient()
            st.adjoint_backward()          # (the residuals and the misfit are the sweep's)
            out = [st.record_misfit(), {name: st.cotangent(name) for name in ("internal_energy", "saturation")}]
            if wrt_params:
                out.append({name: st.param_gradient(name) for name in _capi.HYDRAULIC_PARAMS})
            return tuple(out)


def _tape_slots(positions, steps, K):
    """Slots a run of `steps` taped steps observed at `positions` takes: one per step, or, checkpointed every K, ceil(stretch / K) over
    the stretches between observed positions (an observation closes the open segment)."""
    if K is None:
        return max(steps, 1)
    cuts = sorted({0, steps} | {p for p in positions if 0 < p < steps})
    return max(sum(-(-(b - a) // K) for a, b in zip(cuts, cuts[1:])), 1)


def misfit_gradient(integ: ModelIntegrator, record: TemperatureRecord, steps=None, checkpoint_every=None, wrt_boundary=False,
                    wrt_params=False):
    """The misfit L = sum_k sum_levels 1/2 w (T_{steps_k} - values_k)^2 of `run!(integ; steps)` to a temperature record, per column,
    and its gradient from one forward run and one backward sweep: the integrator is stepped `steps` times (None: to the last
    observation) with its own dt, the record's samples registered where the run reaches their step counts
    (trm_adjoint_observe_misfit), then everything is pulled back at once.  Returns (L as [Nh], dL/dU_0 as [Nz][Nh]) and behind them
    what `vjp` appends for `wrt_boundary` and `wrt_params`.  The tape is sized here: one slot per step, or with `checkpoint_every` = K
    the sum of ceil(stretch / K) over the stretches between observed positions.  Coverage, refusals and option handling of `vjp`."""
    _refuse_uncovered(integ, "misfit_gradient")
    last = record.steps[-1] if record.steps else 0
    steps = last if steps is None else int(steps)
    if steps < last:
        raise ValueError("misfit_gradient: the record has observations behind the last step")
    K = None if checkpoint_every is None else int(checkpoint_every)
    with _taped(integ, _tape_slots(record.steps, steps, K), K, wrt_params) as st:
        dt, at = integ.timestepper.dt, 0
        for k, s in enumerate(record.steps):
            if s > at:
                st.step_record(dt, s - at)
                at = s
            st.observe_misfit(record.levels, record.values[k], None if record.weight is None else record.weight[k])
        if steps > at:
            st.step_record(dt, steps - at)
        _arm_sweep(st, (0.0, 0.0, 0.0), wrt_boundary, wrt_params)
        misfit = st.misfit()           # (the sweep zeroes the accumulator)
        st.adjoint_backward()
        return tuple([misfit] + _sweep_gradients(integ, st, wrt_boundary, wrt_params))


def record_gradient(integ: ModelIntegrator, record: TemperatureRecord, steps=None, checkpoint_every=None, wrt_boundary=False,
                    wrt_params=False):
    """What `misfit_gradient` returns, from a record that is attached once and read inside the backward launches
    (trm_adjoint_observe_record): one attach, one step_record(dt, steps) and one sweep.  No sample is a launch boundary or takes a
    slot: the tape has `steps` slots, or ceil(steps / K) with `checkpoint_every` = K, however dense the record.  `record.steps` must
    be strictly increasing (one sample per position), otherwise ValueError.  Coverage, refusals and option handling of `vjp`."""
    _refuse_uncovered(integ, "record_gradient")
    if not record.steps or any(b <= a for a, b in zip(record.steps, record.steps[1:])):
        raise ValueError("record_gradient: the record's steps must be strictly increasing, one sample per position")
    last = record.steps[-1]
    steps = last if steps is None else int(steps)
    if steps < last:
        raise ValueError("record_gradient: the record has observations behind the last step")
    K = None if checkpoint_every is None else int(checkpoint_every)
    with _taped(integ, _tape_slots([], steps, K), K, wrt_params, detach=True) as st:
        st.attach_record(record.steps, record.levels, record.values, record.weight)
        st.step_record(integ.timestepper.dt, steps)
        _arm_sweep(st, (0.0, 0.0, 0.0), wrt_boundary, wrt_params)
        st.adjoint_backward()          # (the residuals and the misfit are the sweep's)
        return tuple([st.record_misfit()] + _sweep_gradients(integ, st, wrt_boundary, wrt_params))


def _normal_equation_sums(T, S, values, weight):
    """(misfit [Nh], b [q][Nh], A [q][q][Nh]) of the samples T [npos][nlevels][Nh], their sensitivities S [q][npos][nlevels][Nh] and a
    record: r = T - values, misfit = sum 1/2 w r r, b_q = sum w s_q r, A_qq' = sum w s_q s_q'.  float64, positions ascending, levels in
    list order, one term at a time; a NaN sample or a weight that is not > 0 counts for nothing."""
    nq, Nh = len(S), T.shape[2]
    misfit, b, A = np.zeros(Nh), np.zeros((nq, Nh)), np.zeros((nq, nq, Nh))
    for k in range(T.shape[0]):
        for j in range(T.shape[1]):
            w = np.ones(Nh) if weight is None else np.asarray(weight[k, j], dtype=np.float64)
            r = T[k, j] - values[k, j]
            use = (w > 0.0) & ~np.isnan(r)
            w, r = np.where(use, w, 0.0), np.where(use, r, 0.0)
            misfit = misfit + 0.5 * w * r * r
            for q in range(nq):
                sq = np.where(use, S[q][k, j], 0.0)
                b[q] = b[q] + w * sq * r
                for q2 in range(nq):
                    A[q, q2] = A[q, q2] + w * sq * np.where(use, S[q2][k, j], 0.0)
    return misfit, b, A


def record_normal_equations(integ: ModelIntegrator, record: TemperatureRecord, params):
    """The Gauss-Newton normal equations of the misfit of `run!(integ; steps = record.steps[-1])` to a temperature record in the thermal
    parameters `params` (names of `jvp`'s `d_params`), per column: (misfit [Nh], b [q][Nh], A [q][q][Nh]) with r = T - values,
    misfit = sum 1/2 w r^2, b_q = sum w s_q r (the gradient of the misfit), A_qq' = sum w s_q s_q', s_q = dT/d(parameter q) at the
    samples.  One `record_jvp` with a unit seed per name; state and clock are restored in between and afterwards
    (`checkpoint` / `restore`), so the integrator is left where it was.  The sums run in float64 on the host, positions ascending,
    levels in list order, one term at a time; a NaN sample or a weight that is not > 0 counts for nothing.  `record.steps` must be
    strictly increasing."""
    if not record.steps or any(b <= a for a, b in zip(record.steps, record.steps[1:])):
        raise ValueError("record_normal_equations: the record's steps must be strictly increasing, one sample per position")
    params = list(params)
    if not params:
        raise ValueError("record_normal_equations: no parameter")
    start = checkpoint(integ)
    T, S = None, []
    for name in params:
        restore(integ, start)
        T_q, dT_q = record_jvp(integ, record.steps, record.levels, d_params={name: 1.0})
        T = T_q if T is None else T
        S.append(dT_q)
    restore(integ, start)
    return _normal_equation_sums(T, S, record.values, record.weight)
