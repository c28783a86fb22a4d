"""The launches a trm_step call issues -- which instance, how many interior launches, how many materialisations, whether T / liq end
up stored -- over a matrix of tiny contexts, against tests/golden/step_plan_programs.json.  The fixture was recorded at the commit
before the step launch became one plan per launch (tests/golden/make_step_plan_fixture.py, run once): the plan must select, launch for
launch, what the request / outcome exchange between Ops::fused_launch and the launchers selected.  The test never regenerates it."""
import json
import os

import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_plan_programs.json")
CALLS = ((1, False), (3, True), (1, False), (7, False))      # (steps, finalize) of the four trm_step calls of every context
INFO = ("info_last_program", "info_interior_launches", "info_materializations", "info_closure_stored")


def case(name, config, Nh, Nz, dtype="f64", hydraulics="default", heun=False, steps_per_launch=1, gradient_top=False, **options):
    return dict(name=name, config=config, Nh=Nh, Nz=Nz, dtype=dtype, hydraulics=hydraulics, heun=heun, steps_per_launch=steps_per_launch,
                gradient_top=gradient_top, options=options)


# Nh = 5 (less than one wave) and 67 (more than one); Nz = 30 (32 lanes per column), 40 (64) and 100 (two levels per lane)
CASES = [
    case("heat_5x30_derive1", "heat", 5, 30, derive_closure_fields=1),
    case("heat_67x40_derive0", "heat", 67, 40, derive_closure_fields=0),
    case("heat_5x40_default_launch", "heat", 5, 40, steps_per_launch=0),
    case("richards_67x30_derive1", "richards", 67, 30, derive_closure_fields=1),
    case("richards_5x40_derive_auto", "richards", 5, 40),
    case("richards_67x30_derive0", "richards", 67, 30, derive_closure_fields=0),
    case("richards_67x30_derive1_no_interior", "richards", 67, 30, derive_closure_fields=1, interior_steps=0),
    case("richards_5x30_derive1_no_deferral", "richards", 5, 30, derive_closure_fields=1, defer_closure_stores=0),
    case("richards_67x30_default_launch", "richards", 67, 30, steps_per_launch=0, derive_closure_fields=1),
    case("richards_vg_67x40_derive1", "richards", 67, 40, hydraulics="vg", derive_closure_fields=1),
    case("richards_vg_5x30_derive0", "richards", 5, 30, hydraulics="vg", derive_closure_fields=0),
    case("richards_67x100_derive1", "richards", 67, 100, derive_closure_fields=1),
    case("richards_5x100_default_launch", "richards", 5, 100, steps_per_launch=0),
    case("land_67x30_derive1", "land", 67, 30, derive_closure_fields=1),
    case("land_5x40_derive0", "land", 5, 40, derive_closure_fields=0),
    case("land_vg_67x40_derive1", "land", 67, 40, hydraulics="vg", derive_closure_fields=1),
    case("land_5x40_surface_own_launch_derive1", "land", 5, 40, derive_closure_fields=1, surface_in_launch=0),
    case("land_67x30_surface_own_launch_derive0", "land", 67, 30, derive_closure_fields=0, surface_in_launch=0),
    case("land_5x30_default_launch", "land", 5, 30, steps_per_launch=0),
    case("f32_richards_67x30_packed_derive1", "richards", 67, 30, dtype="f32", derive_closure_fields=1),
    case("f32_richards_5x40_packed_derive0", "richards", 5, 40, dtype="f32", derive_closure_fields=0),
    case("f32_richards_67x40_unpacked_derive1", "richards", 67, 40, dtype="f32", derive_closure_fields=1, packed_f32=0),
    case("f32_heat_5x30_unpacked_derive0", "heat", 5, 30, dtype="f32", derive_closure_fields=0, packed_f32=0),
    case("f32_land_67x30_packed", "land", 67, 30, dtype="f32"),
    case("generic_richards_67x30_derive1", "richards", 67, 30, gradient_top=True, derive_closure_fields=1),
    case("generic_heat_5x40_derive0", "heat", 5, 40, gradient_top=True, derive_closure_fields=0),
    case("heun_richards_5x30_derive1", "richards", 5, 30, heun=True, derive_closure_fields=1),
    case("heun_land_67x40_derive1", "land", 67, 40, heun=True, derive_closure_fields=1),
    case("heun_heat_67x100", "heat", 67, 100, heun=True),
]


def record(c):
    """The four INFO values after each of the four calls of CALLS, on a fresh context of case `c`."""
    lat, lon = W.synthetic_columns(c["Nh"])
    w = W.make_workload(c["config"], lat, lon, c["Nz"], dtype=np.float32 if c["dtype"] == "f32" else np.float64, hydraulics=c["hydraulics"])
    if c["gradient_top"]:
        w["bcs"][("temperature", "top")] = ("gradient", np.full(c["Nh"], 0.5))
    d = W.setup_device(w, steps_per_launch=c["steps_per_launch"])
    for k, v in c["options"].items():
        d.set_option(k, v)
    out = []
    for steps, finalize in CALLS:
        (d.step_heun if c["heun"] else d.step)(w["dt"], steps, finalize=finalize)
        out.append([d.get_option(k) for k in INFO])
    assert d.status() == 0
    d.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        g = json.load(f)
    assert g["info"] == list(INFO) and g["calls"] == [[n, int(f)] for n, f in CALLS]
    return g["cases"]


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_step_calls_select_what_the_parent_selected(c, golden):
    assert golden[c["name"]]["context"] == c       # (the fixture was recorded for this very context)
    assert record(c) == golden[c["name"]]["after_each_call"], c["name"]
