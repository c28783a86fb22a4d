"""What the derivative entry points of the C ABI refuse, call for call: the return code and the trm_last_error text of every refusal
that needs no allocation failure, and the answers of trm_adjoint_tape / trm_adjoint_checkpoints along a short record / backward
sequence on both tape kinds, against tests/golden/derivative_refusals.json.  The fixture was recorded once with the library of the
commit before the derivative host layer moved into a translation unit of its own (tests/golden/make_derivative_refusals_fixture.py):
the move must answer every call with the same code and the same words.  The test never regenerates it.

Contexts are 3 columns x 4 levels, heat-only fp64; the other model kinds (fp32, Richards, LandModel, vegetation) at the same size and
one of 80 levels; the series is one 5-node surface-temperature record.  (A tape recorded without the series the context holds now:
attaching the series marks a tape that holds steps stale, so that is the refusal the sequence meets.)"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import terrarium_jl_amd as trm

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derivative_refusals.json")
CAPI = trm._capi
NH, NZ, NT, DT = 3, 4, 5, 300.0
TIMES = [0.0, 300.0, 600.0, 900.0, 1200.0]
T, U_ = CAPI.BC_VAR["temperature"], CAPI.BC_VAR["internal_energy"]
SAT = CAPI.BC_VAR["saturation_water_ice"]
BOT, TOP = CAPI.SIDE["bottom"], CAPI.SIDE["top"]


def context(kind="heat", Nz=NZ, **param_overrides):
    p = CAPI.default_params()
    if kind in ("richards", "land"):
        p.flow = CAPI.FLOW["richards"]
    if kind == "land":
        p.seb = 1
    for k, v in param_overrides.items():
        setattr(p, k, v)
    thickness = trm.ExponentialSpacing(N=Nz).get_spacing()
    grid = trm.ColumnGrid(trm.PrescribedSpacing(dz=list(thickness)), NH, dtype=np.float32 if kind == "f32" else np.float64)
    d = trm.DeviceState(grid, p)
    if kind == "vegetation":
        d.set_vegetation(CAPI.default_vegetation_params(), "standalone")
    d.set("temperature", np.linspace(-2.0, 2.0, Nz))
    d.set_bc("temperature", "top", "value", 1.0)
    d.initialize()
    return d


class Calls:
    """Calls entry points by name on one context and keeps [label, code, message] of each (the message of a refusal alone)."""

    def __init__(self, d, log, prefix=""):
        self.d, self.log, self.prefix = d, log, prefix
        self.buf = np.zeros(256, dtype=np.float64)        # (every host array the calls read or write fits: 80 x 3, 5 x 3)
        self.host = self.buf.ctypes.data

    def __call__(self, name, *args, label=None):
        rc = getattr(self.d._lib, name)(self.d._ctx, *args)
        msg = self.d._lib.trm_last_error(self.d._ctx).decode() if rc else ""
        shown = [("NULL" if a is None else "ptr" if not isinstance(a, (int, float)) or (isinstance(a, int) and a > 1 << 20) else a) for a in args]
        self.log.append([self.prefix + (label or f"{name}{tuple(shown)}"), rc, msg])
        return rc

    def ok(self, name, *args):
        assert self(name, *args) == 0, self.log[-1]

    def ptr(self):
        return C.byref(C.c_void_p())

    def i64(self):
        return C.byref(C.c_int64())

    def i32(self):
        return C.byref(C.c_int32())

    def tape(self):
        """(recorded, capacity) and (interval, used, capacity) as the two getters answer"""
        n, cap, k, used, slots = (C.c_int32(-1) for _ in range(5))
        rc1 = self.d._lib.trm_adjoint_tape(self.d._ctx, C.byref(n), C.byref(cap))
        rc2 = self.d._lib.trm_adjoint_checkpoints(self.d._ctx, C.byref(k), C.byref(used), C.byref(slots))
        self.log.append([self.prefix + "tape", [rc1, rc2], [n.value, cap.value, k.value, used.value, slots.value]])

    def every_entry_point(self):
        """each entry point once, with arguments that are in order"""
        h, seeds = self.host, (C.c_double * 10)(*([1.0] * 10))
        self("trm_tangent_bc_series_upload", T, TOP, NT, h)
        self("trm_tangent_bc_upload", T, TOP, h)
        self("trm_tangent_param_set", seeds)
        self("trm_tangent_upload", 0, h)
        self("trm_tangent_download", 1, h)
        self("trm_tangent_device_ptr", 0, self.ptr(), self.i64())
        self("trm_tangent_closure")
        self("trm_step_tangent", DT, 1)
        self("trm_adjoint_checkpoints", self.i32(), self.i32(), self.i32())
        self("trm_adjoint_tape", self.i32(), self.i32())
        self("trm_adjoint_bc_open")
        self("trm_adjoint_bc_series_download", T, TOP, NT, h)
        self("trm_adjoint_bc_series_device_ptr", T, TOP, self.ptr(), self.i32())
        self("trm_adjoint_bc_download", T, TOP, h)
        self("trm_adjoint_bc_device_ptr", T, TOP, self.ptr())
        self("trm_adjoint_param_open")
        self("trm_adjoint_param_download", 0, h)
        self("trm_adjoint_param_device_ptr", 0, self.ptr())
        self("trm_adjoint_upload", 0, h)
        self("trm_adjoint_download", 0, h)
        self("trm_adjoint_device_ptr", 0, self.ptr(), self.i64())
        self("trm_step_record", DT, 1)
        self("trm_adjoint_backward")

    def steps(self):
        self("trm_step_tangent", DT, 1)
        self("trm_step_record", DT, 1)
        self("trm_adjoint_backward")

    def open_both(self, capacity=4, seed_params=False, open_params=False):
        self.ok("trm_tangent_open")
        self.ok("trm_tangent_upload", 0, self.host)
        if seed_params:
            self.ok("trm_tangent_param_set", (C.c_double * 10)(*([1.0] * 10)))
        self.ok("trm_adjoint_open", capacity)
        if open_params:
            self.ok("trm_adjoint_param_open")


def series(d, var="temperature", side="top", kind="value"):
    d.set_bc_series(var, side, kind, TIMES, np.ones((NT, NH)))


def nothing_open(log):
    c = Calls(context(), log)
    c("trm_tangent_close")
    c("trm_adjoint_close")
    c.every_entry_point()
    c.ok("trm_adjoint_open", 2)                       # the adjoint alone: its boundary and parameter gradients are not open
    c("trm_adjoint_bc_download", T, TOP, c.host)
    c("trm_adjoint_bc_device_ptr", T, TOP, c.ptr())
    c("trm_adjoint_param_download", 0, c.host)
    c("trm_adjoint_param_device_ptr", 0, c.ptr())
    c.ok("trm_adjoint_close")
    c("trm_adjoint_close")
    c.ok("trm_tangent_open")
    c.ok("trm_tangent_close")
    c("trm_tangent_close")
    c("trm_tangent_download", 0, c.host)


def bad_arguments(log):
    d = context()
    c = Calls(d, log)
    c("trm_adjoint_open", 0)
    c("trm_adjoint_open_checkpointed", 0, 4)
    c("trm_adjoint_open_checkpointed", 2, 0)
    c("trm_adjoint_open_checkpointed", 2, 33)
    c.open_both(open_params=True)
    h = c.host
    for fam in ("tangent", "adjoint"):
        for which in (-1, 3):
            c(f"trm_{fam}_upload", which, h)
            c(f"trm_{fam}_download", which, h)
            c(f"trm_{fam}_device_ptr", which, c.ptr(), c.i64())
        c(f"trm_{fam}_upload", 0, None)
        c(f"trm_{fam}_download", 0, None)
        c(f"trm_{fam}_device_ptr", 0, None, c.i64())
        c(f"trm_{fam}_device_ptr", 0, c.ptr(), None)
    for var, side, ptr in ((SAT, TOP, h), (T, 2, h), (T, -1, h), (U_, BOT, None)):
        c("trm_tangent_bc_upload", var, side, ptr)
        c("trm_adjoint_bc_download", var, side, ptr)
        c("trm_adjoint_bc_device_ptr", var, side, c.ptr() if ptr else None)
        c("trm_tangent_bc_series_upload", var, side, NT, ptr)
        c("trm_adjoint_bc_series_download", var, side, NT, ptr)
        c("trm_adjoint_bc_series_device_ptr", var, side, c.ptr() if ptr else None, c.i32())
    c("trm_adjoint_bc_series_device_ptr", T, TOP, c.ptr(), None)
    c("trm_tangent_param_set", None)
    for which, ptr in ((-1, h), (10, h), (0, None)):
        c("trm_adjoint_param_download", which, ptr)
        c("trm_adjoint_param_device_ptr", which, c.ptr() if ptr else None)
    c("trm_step_tangent", DT, -1)
    c("trm_step_record", DT, -1)
    # a pair with a series: null pointers and nt
    d.set_option("derivative_series", 1)
    series(d)
    c("trm_tangent_bc_series_upload", T, TOP, NT, None)
    c("trm_adjoint_bc_series_download", T, TOP, NT, None)
    c("trm_adjoint_bc_series_device_ptr", T, TOP, None, c.i32())
    c("trm_tangent_bc_series_upload", T, TOP, NT - 1, h)
    c("trm_tangent_bc_series_upload", T, TOP, NT + 1, h)
    c("trm_adjoint_bc_series_download", T, TOP, NT - 1, h)
    c("trm_adjoint_bc_series_download", T, TOP, NT + 1, h)
    c("trm_tangent_bc_series_upload", T, TOP, NT, h)
    c("trm_adjoint_bc_series_download", T, TOP, NT, h)
    # ... handed to the per-column calls, and a pair without one to the per-node calls
    c("trm_tangent_bc_upload", T, TOP, h)
    c("trm_adjoint_bc_download", T, TOP, h)
    c("trm_adjoint_bc_device_ptr", T, TOP, c.ptr())
    c("trm_tangent_bc_series_upload", U_, BOT, NT, h)
    c("trm_adjoint_bc_series_download", U_, BOT, NT, h)
    c("trm_adjoint_bc_series_device_ptr", U_, BOT, c.ptr(), c.i32())
    c("trm_tangent_bc_upload", U_, BOT, h)
    c("trm_adjoint_bc_download", U_, BOT, h)


def other_model_kinds(log):
    for kind, Nz in (("f32", NZ), ("richards", NZ), ("land", NZ), ("vegetation", NZ), ("heat", 80)):
        c = Calls(context(kind, Nz), log, prefix=f"{kind} x {Nz}: ")
        c("trm_tangent_open")
        c("trm_adjoint_open", 2)
        c("trm_adjoint_open_checkpointed", 2, 4)
        c.every_entry_point()
        c.d.close()


def open_average(log):
    d = context()
    c = Calls(d, log)
    c.open_both()
    handle = d.open_average("temperature")
    c.steps()
    d.close_average(handle)
    c.steps()


def series_refusals(log):
    # a series without the option; the setters say nothing there
    d = context()
    c = Calls(d, log, "no option: ")
    c.open_both()
    series(d)
    c("trm_tangent_param_set", (C.c_double * 10)(*([1.0] * 10)))
    c("trm_adjoint_param_open")
    c.steps()
    c("trm_tangent_bc_upload", T, TOP, c.host)
    # series the derivative launches do not take
    for what in ("gradient kind", "forcing", "generic boundary kinds", "windowed"):
        d = context()
        d.set_option("derivative_series", 1)
        c = Calls(d, log, what + ": ")
        c.open_both()
        if what == "gradient kind":
            series(d, "internal_energy", "top", "gradient")
        elif what == "forcing":
            d.set_forcing_series("air_temperature", TIMES, np.ones((NT, NH)))
        elif what == "generic boundary kinds":
            d.set_bc("temperature", "top", "gradient", -0.5)
            series(d, "internal_energy", "bottom", "flux")
        else:
            series(d)
            d.series_window(("temperature", "top"), 8)
        c.steps()
    # parameters with a series: refused by the setters, and by the steps when the series arrives later; taken with the second option
    d = context()
    d.set_option("derivative_series", 1)
    c = Calls(d, log, "parameters, series first: ")
    c.open_both()
    series(d)
    c("trm_tangent_param_set", (C.c_double * 10)(*([1.0] * 10)))
    c("trm_adjoint_param_open")
    c.steps()
    d = context()
    d.set_option("derivative_series", 1)
    c = Calls(d, log, "parameters, series later: ")
    c.open_both(seed_params=True, open_params=True)
    series(d)
    c.steps()
    d.set_option("derivative_series_params", 1)
    c.prefix = "parameters, both options: "
    c("trm_tangent_param_set", (C.c_double * 10)(*([1.0] * 10)))
    c("trm_adjoint_param_open")
    c.steps()
    c.tape()


def conductivity(log):
    for name in ("k_air", "k_mineral"):
        c = Calls(context(**{name: 0.0}), log, name + " = 0: ")
        c.open_both()
        c("trm_tangent_param_set", (C.c_double * 10)(*([1.0] * 10)))
        c("trm_adjoint_param_open")


def stale(log):
    d = context()
    c = Calls(d, log)
    c.open_both()
    c.ok("trm_step_tangent", DT, 1)
    c.ok("trm_step_record", DT, 2)                  # (a state-changing call for the tangent)
    c("trm_tangent_download", 0, c.host)
    c("trm_tangent_download", 1, c.host)
    c("trm_tangent_download", 2, c.host)
    c("trm_tangent_closure")
    c("trm_step_tangent", DT, 1)
    c.ok("trm_tangent_upload", 0, c.host)
    c("trm_step_tangent", DT, 1)                    # (... and this one for the tape)
    c("trm_step_record", DT, 1)
    c("trm_adjoint_backward")
    c.tape()
    c.ok("trm_adjoint_open", 4)
    c.ok("trm_step_record", DT, 1)
    d.set_bc("temperature", "top", "value", 2.0)    # a boundary condition changes under the tape
    c("trm_step_record", DT, 1)
    c("trm_adjoint_backward")
    # a tape recorded without the series the context holds now
    d.set_option("derivative_series", 1)
    c.ok("trm_adjoint_open", 4)
    c.ok("trm_step_record", DT, 2)
    series(d)
    c("trm_adjoint_backward")
    c("trm_step_record", DT, 1)
    c.tape()


def tapes(log):
    c = Calls(context(), log, "per step: ")
    c.ok("trm_adjoint_open", 3)
    c.tape()
    for n in (2, 2, 1, 1, 0):
        c("trm_step_record", DT, n)
        c.tape()
    c("trm_adjoint_backward")
    c.tape()
    c("trm_step_record", DT, 4)
    c("trm_step_record", DT, 3)
    c.tape()
    c = Calls(context(), log, "checkpointed: ")
    c.ok("trm_adjoint_open_checkpointed", 2, 4)
    c.tape()
    for dt, n in ((DT, 3), (DT, 2), (DT, 4), (2 * DT, 1), (DT, 3), (DT, 1), (DT, 0)):
        c("trm_step_record", dt, n)
        c.tape()
    c("trm_adjoint_backward")
    c.tape()
    c("trm_step_record", DT, 9)
    c("trm_step_record", DT, 1)
    c("trm_step_record", 2 * DT, 1)
    c("trm_step_record", DT, 1)
    c.tape()
    c("trm_adjoint_backward")
    c.tape()


SCENARIOS = (nothing_open, bad_arguments, other_model_kinds, open_average, series_refusals, conductivity, stale, tapes)


def record(scenario):
    log = []
    scenario(log)
    return log


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)["scenarios"]


def test_the_fixture_covers_every_scenario(golden):
    assert sorted(golden) == sorted(s.__name__ for s in SCENARIOS)


@pytest.mark.parametrize("scenario", SCENARIOS, ids=[s.__name__ for s in SCENARIOS])
def test_every_call_answers_as_the_parent_did(scenario, golden):
    got, want = record(scenario), golden[scenario.__name__]
    assert [g[0] for g in got] == [w[0] for w in want]            # (the fixture was recorded for these very calls)
    for g, w in zip(got, want):
        assert g == w, g[0]
