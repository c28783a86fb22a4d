"""The five derivative drivers of the package (jvp, record_jvp, vjp, misfit_gradient, record_gradient) against a stub state: which
DeviceState methods each calls, in which order and with which scalar arguments, what it returns and what it does on the way out when a
step fails -- against tests/golden/derivative_driver_calls.json, recorded once with the drivers of the commit before they moved into
terrarium.jl_amd/derivatives.py (tests/golden/make_derivative_driver_calls_fixture.py).  The test never regenerates the fixture.  No
GPU and no library: the stub stands in for the state, and the drivers touch nothing else.

Every driver runs plain, with boundary seeds / gradients on a constant pair and on a pair driven by a FieldTimeSeries, with thermal
parameters, checkpointed (the adjoint drivers), on a tangent / adjoint that is open already (vjp: with the tape it would open, and with
another), and with a step call that raises, on a state the driver opened and on one that was open."""
import inspect
import json
import os

import numpy as np
import pytest

import terrarium_jl_amd as trm

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derivative_driver_calls.json")
NH, NZ, NT, DT = 3, 4, 5, 300.0
TOP_T, BOTTOM_U = ("temperature", "top"), ("internal_energy", "bottom")


def show(v):
    """A value as the fixture keeps it: scalars as they are, arrays by shape, containers element by element."""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.integer, np.floating, np.bool_)):
        return v.item()
    if isinstance(v, np.ndarray):
        return {"array": list(v.shape)} if v.ndim else v.item()
    if isinstance(v, dict):
        return {"/".join(k) if isinstance(k, tuple) else str(k): show(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [show(x) for x in v]
    return type(v).__name__


class StubState:
    """Stands in for a DeviceState: logs [method, {parameter: value}] of every call, bound to the signature of the DeviceState method
    of that name (a name DeviceState does not have is an AttributeError), and returns a token that names the call."""

    def __init__(self, log, tangent_open=False, adjoint_open=False, checkpoints=(0, 0, 1), fail=None):
        self._log, self._checkpoints, self._fail = log, checkpoints, fail
        self._options = {"derivative_series": 5, "derivative_series_params": 6}      # (not 0 / 1: the restore shows what was read)
        if tangent_open:
            self._tangent_open = True
        if adjoint_open:
            self._adjoint_open = True

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        signature = inspect.signature(getattr(trm.DeviceState, name))

        def call(*args, **kwargs):
            bound = signature.bind(self, *args, **kwargs)
            bound.apply_defaults()
            shown = {k: show(v) for k, v in bound.arguments.items() if k != "self"}
            self._log.append([name, shown])
            if name == self._fail:
                raise RuntimeError(f"stub: {name} failed")
            if name in ("open_tangent", "close_tangent"):
                self._tangent_open = name == "open_tangent"
            if name in ("open_adjoint", "close_adjoint"):
                self._adjoint_open = name == "open_adjoint"
            if name == "get_option":
                return self._options[args[0]]
            if name == "set_option":
                self._options[args[0]] = args[1]
            if name == "adjoint_checkpoints":
                return self._checkpoints
            return f"{name}({', '.join(str(x) for x in shown.values() if not isinstance(x, (dict, list)))})"

        return call


class StubIntegrator:
    def __init__(self, state, series=False, timestepper=None, time_dependent=False, windowed=False):
        self.state = state
        self.timestepper = timestepper or trm.ForwardEuler(dt=DT)
        top = trm.FieldTimeSeries(DT * np.arange(NT), np.linspace(0.0, 2.0, NT)) if series else 1.0
        # (the saturation pair: one whose value the heat-only run does not read, and no gradient is asked for)
        self.boundary_conditions = {TOP_T: ("value", top), BOTTOM_U: ("flux", 0.05), ("saturation_water_ice", "top"): ("flux", 0.0)}
        self._flags = time_dependent, windowed

    def _has_time_dependence(self):
        return self._flags[0]

    def _windowed(self):
        return self._flags[1]


def record_of(steps):
    rng = np.random.default_rng(24)
    return trm.TemperatureRecord(steps, [0, 2], rng.normal(0.0, 1.0, (len(steps), 2, NH)), weight=2.0)


U0 = np.ones((NZ, NH))
PARAMS = {"k_mineral": 1.0, "c_water": -2.0}
RECORD, TWICE = record_of([0, 3, 6]), record_of([2, 2, 5])      # (misfit_gradient takes a position twice)
# the drivers and what each takes in every form: (driver, positional arguments, boundary keyword, parameter keyword, step method)
DRIVERS = {
    "jvp": (trm.jvp, (U0, 6), "d_boundary", dict(d_params=PARAMS), "step_tangent"),
    "record_jvp": (trm.record_jvp, ([0, 3, 6], [0, 2]), "d_boundary", dict(d_params=PARAMS), "step_tangent"),
    "vjp": (trm.vjp, (6,), "wrt_boundary", dict(wrt_params=True), "step_record"),
    "misfit_gradient": (trm.misfit_gradient, (TWICE,), "wrt_boundary", dict(wrt_params=True), "step_record"),
    "record_gradient": (trm.record_gradient, (RECORD,), "wrt_boundary", dict(wrt_params=True), "step_record"),
}
TANGENT = ("jvp", "record_jvp")


def scenarios():
    """{name: (driver, args, kwargs, stub state keywords, series)}"""
    out = {}
    for name, (driver, args, boundary, params, step) in DRIVERS.items():
        tangent = name in TANGENT
        seeds = lambda series: {TOP_T: np.ones((NT, NH)) if series else 0.5, BOTTOM_U: np.ones(NH)} if tangent else True      # noqa: E731
        is_open = dict(tangent_open=True) if tangent else dict(adjoint_open=True, checkpoints=(0, 0, 6))
        out[f"{name} plain"] = (driver, args, {}, {}, False)
        out[f"{name} boundary"] = (driver, args, {boundary: seeds(False)}, {}, False)
        out[f"{name} boundary series"] = (driver, args, {boundary: seeds(True)}, {}, True)
        out[f"{name} params"] = (driver, args, params, {}, False)
        out[f"{name} params boundary series"] = (driver, args, dict(params, **{boundary: seeds(True)}), {}, True)
        if not tangent:
            out[f"{name} checkpointed"] = (driver, args, dict(checkpoint_every=4), {}, False)
            out[f"{name} checkpointed already open"] = (driver, args, dict(checkpoint_every=4), dict(adjoint_open=True, checkpoints=(4, 0, 2)), False)
            out[f"{name} already open, another tape"] = (driver, args, {}, dict(adjoint_open=True, checkpoints=(0, 2, 6)), False)
        out[f"{name} already open"] = (driver, args, {}, is_open, False)
        out[f"{name} step fails"] = (driver, args, {}, dict(fail=step), True)
        out[f"{name} step fails already open"] = (driver, args, {}, dict(is_open, fail=step), False)
    out["vjp cotangents"] = (trm.vjp, (0,), dict(temperature=U0, liquid_water_fraction=2.0), {}, False)
    out["record_jvp seeds and steps"] = (trm.record_jvp, ([0], [1]), dict(d_internal_energy=U0, steps=4), {}, False)
    out["misfit_gradient steps behind the record"] = (trm.misfit_gradient, (RECORD,), dict(steps=8, checkpoint_every=4), {}, False)
    out["record_gradient steps behind the record"] = (trm.record_gradient, (RECORD,), dict(steps=8, checkpoint_every=4), {}, False)
    return out


def record(scenario):
    """What a scenario does: {"calls": [[method, arguments], ...], "returned": ... | "raised": ...}"""
    driver, args, kwargs, state, series = scenario
    log = []
    integ = StubIntegrator(StubState(log, **state), series=series)
    try:
        return dict(calls=log, returned=show(driver(integ, *args, **kwargs)))
    except RuntimeError as e:
        return dict(calls=log, raised=f"{type(e).__name__}: {e}")


def record_all():
    return {name: record(s) for name, s in scenarios().items()}


@pytest.fixture(scope="module")
def pinned():
    with open(FIXTURE) as f:
        return json.load(f)["scenarios"]


def test_the_fixture_covers_every_scenario(pinned):
    assert set(pinned) == set(scenarios())
    for name in DRIVERS:
        forms = {k[len(name) + 1:] for k in pinned if k.startswith(name + " ")}
        assert {"plain", "boundary", "boundary series", "params", "already open", "step fails", "step fails already open"} <= forms, name
        assert ("checkpointed" in forms) == (name not in TANGENT), name


@pytest.mark.parametrize("name", sorted(scenarios()))
def test_driver_makes_the_pinned_calls_in_the_pinned_order(name, pinned):
    got = json.loads(json.dumps(record(scenarios()[name])))
    want = pinned[name]
    for n, (a, b) in enumerate(zip(got["calls"], want["calls"])):
        assert a == b, (name, f"call {n}")
    assert len(got["calls"]) == len(want["calls"]), (name, got["calls"][len(want["calls"]):], want["calls"][len(got["calls"]):])
    assert got == want, name


def test_the_way_out(pinned):
    """what the scenarios are there to show, read off the pinned calls themselves"""
    def names(key):
        return [c[0] for c in pinned[key]["calls"]]

    for name in DRIVERS:
        tangent = name in TANGENT
        close, opener = ("close_tangent", "open_tangent") if tangent else ("close_adjoint", "open_adjoint")
        assert names(f"{name} plain")[0] == opener and names(f"{name} plain")[-1] == close, name
        assert "raised" in pinned[f"{name} step fails"] and names(f"{name} step fails")[-1] == close, name
        # the options go back to what they were in front of the close, also when the step raises
        assert names(f"{name} step fails")[-2] == "set_option" and pinned[f"{name} step fails"]["calls"][-2][1]["value"] == 5, name
        assert close not in names(f"{name} already open") and close not in names(f"{name} step fails already open"), name
    assert "open_tangent" not in names("jvp already open") and names("record_jvp already open")[-1] == "detach_tangent_record"
    assert names("record_jvp step fails already open")[-1] == "detach_tangent_record"
    # vjp keeps a tape of the shape it would open; the record drivers always open theirs, and detach a record from an adjoint that was open
    assert "open_adjoint" not in names("vjp already open") and "open_adjoint" not in names("vjp checkpointed already open")
    assert names("vjp already open, another tape")[:2] == ["adjoint_checkpoints", "open_adjoint"]
    for name in ("misfit_gradient", "record_gradient"):
        assert names(f"{name} already open")[0] == "open_adjoint" and "adjoint_checkpoints" not in names(f"{name} already open"), name
    assert names("record_gradient already open")[-1] == "detach_record" and names("record_gradient step fails already open")[-1] == "detach_record"
    assert "detach_record" not in names("misfit_gradient already open")
    # misfit() is read in front of the sweep, record_misfit() behind it
    assert names("misfit_gradient plain").index("misfit") < names("misfit_gradient plain").index("adjoint_backward")
    assert names("record_gradient plain").index("record_misfit") > names("record_gradient plain").index("adjoint_backward")


@pytest.mark.parametrize("name", sorted(DRIVERS))
def test_refusals_before_the_state_is_touched(name):
    driver, args = DRIVERS[name][:2]
    for kwargs, text in ((dict(timestepper=trm.Heun(dt=DT)), f"{name}: ForwardEuler only"),
                         (dict(time_dependent=True), f"{name}: boundary conditions and inputs must be constant over the run"),
                         (dict(windowed=True), f"{name}: boundary conditions and inputs must be constant over the run")):
        log = []
        with pytest.raises(ValueError) as e:
            driver(StubIntegrator(StubState(log), **kwargs), *args)
        assert str(e.value) == text and log == []
