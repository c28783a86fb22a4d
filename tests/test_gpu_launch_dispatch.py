"""The launches of trm_step over the contexts tests/test_gpu_step_plan.py does not reach -- the multi-step program with a series, the
time averages in its launch, four levels per lane, Heun with generic boundary kinds, the interleaved LandModel launches, every
k_column_psi signature, the packed signature instances -- against tests/golden/launch_dispatch_programs.json: per call the instance
(TRM_INFO_LAST_PROGRAM), the interior launches, the materialisations, whether T / liq end up stored, and the sha256 of the downloaded
internal energy, saturation and temperature.  The fixture was recorded at the commit before the launch files were rewritten on one
value-to-instance dispatcher (tests/golden/make_launch_dispatch_fixture.py, run once, every state checked against the oracle first): the
dispatcher must reach, launch for launch, the instance the hand-written ladders reached, and refuse what they refused with the same
text.  The test never regenerates it."""
import hashlib
import json
import os

import numpy as np
import pytest

import terrarium_jl_amd as trm
import workloads as W
from test_gpu_step_plan import CALLS, INFO

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_dispatch_programs.json")
HASHED = ("internal_energy", "saturation_water_ice", "temperature")
# the boundary conditions of the four signatures k_column_psi has (0, 2, 6, 34), on the Richards workload (its own: temperature at the top)
SIGNATURE_BCS = {0: "closed", 2: {}, 6: {("internal_energy", "bottom"): ("flux", 0.05)}, 34: {("saturation_water_ice", "top"): ("flux", -2.0e-7)}}


def case(name, config, Nz, dtype="f64", hydraulics="default", heun=False, steps_per_launch=1, gradient_top=False, series=None, average=None,
         signature=None, **options):
    return [dict(name=f"{name}_{Nh}x{Nz}", config=config, Nh=Nh, Nz=Nz, dtype=dtype, hydraulics=hydraulics, heun=heun, steps_per_launch=steps_per_launch,
                 gradient_top=gradient_top, series=series, average=average, signature=signature, options=options) for Nh in (5, 67)]      # under and over one wavefront


CASES = sum([
    # the multi-step program with a series in the launch
    case("multi_heat_series", "heat", 30, steps_per_launch=4, series="temperature_top"),
    case("multi_land_series", "land", 40, steps_per_launch=4, series="forcing"),
    # ... with an open time average (k_column_accum)
    case("accum_richards", "richards", 30, steps_per_launch=4, average="temperature"),
    case("accum_richards_series", "richards", 30, steps_per_launch=4, average="temperature", series="temperature_top"),
    case("accum_f32_heat", "heat", 40, dtype="f32", steps_per_launch=4, average="temperature"),
    case("accum_f32_heat_series", "heat", 40, dtype="f32", steps_per_launch=4, average="temperature", series="temperature_top"),
    # four levels per lane (k_column_wide)
    case("wide_richards", "richards", 200),
    case("wide_richards_heun", "richards", 200, heun=True),
    case("wide_f32_richards", "richards", 200, dtype="f32"),
    case("wide_f32_richards_heun", "richards", 200, dtype="f32", heun=True),
    # two levels per lane in fp32 off the packed kernel
    case("deep_f32_richards_unpacked", "richards", 100, dtype="f32", packed_f32=0),
    # Heun with a Gradient condition at the top (k_heun_generic)
    case("heun_generic_richards", "richards", 30, heun=True, gradient_top=True),
    case("heun_generic_heat", "heat", 40, heun=True, gradient_top=True),
    # the interleaved LandModel launches (k_land_euler / k_land_pk): the call of three steps
    case("land_interleaved", "land", 30, pipeline_parts=1),
    case("land_interleaved_f32", "land", 40, dtype="f32", pipeline_parts=1),
    # every k_column_psi signature
    case("psi_signature_0", "richards", 30, signature=0, derive_closure_fields=1),
    case("psi_signature_2", "richards", 40, signature=2, derive_closure_fields=1),
    case("psi_signature_6", "richards", 30, signature=6, derive_closure_fields=1),
    case("psi_signature_34", "richards", 40, signature=34, derive_closure_fields=1),
    case("psi_signature_6_vg", "richards", 40, hydraulics="vg", signature=6, derive_closure_fields=1),
    # the packed signature instances: the liquid fraction alone, forced
    case("packed_land_derive_liq", "land", 30, dtype="f32", derive_closure_fields=3),
    case("packed_land_own_surface_launch_derive_liq", "land", 40, dtype="f32", derive_closure_fields=3, surface_in_launch=0),      # (k_step_pk<..., sig LAND>)
    case("packed_richards_derive_liq", "richards", 40, dtype="f32", derive_closure_fields=3),
], [])


def workload(c):
    lat, lon = W.synthetic_columns(c["Nh"])
    w = W.make_workload(c["config"], lat, lon, c["Nz"], dtype=np.float32 if c["dtype"] == "f32" else np.float64, hydraulics=c["hydraulics"])
    if c["gradient_top"]:
        w["bcs"][("temperature", "top")] = ("gradient", np.full(c["Nh"], 0.5))
    if c["signature"] is not None:
        extra = SIGNATURE_BCS[c["signature"]]
        if extra == "closed":
            w["bcs"].clear()
        else:
            w["bcs"].update({k: (kind, np.full(c["Nh"], v)) for k, (kind, v) in extra.items()})
    return w


def attach_series(c, w, x):
    """The case's series on `x`, a device context or the oracle (the same calls on either)."""
    times = 150.0 * np.arange(9)      # (the twelve steps of CALLS cross several nodes)
    phase = 2 * np.pi * times[:, None] / W.DAY - w["lon"][None, :]
    if c["series"] == "temperature_top":
        x.set_bc_series("temperature", "top", "value", times, w["T0"][None, :] + 10.0 * np.sin(phase))
    elif c["series"] == "forcing":
        x.set_forcing_series("air_temperature", times, w["T0"][None, :] + 5.0 * np.sin(phase))


def device(c, w):
    d = W.setup_device(w, steps_per_launch=c["steps_per_launch"])
    for k, v in c["options"].items():
        d.set_option(k, v)
    attach_series(c, w, d)
    if c["average"]:
        d.open_average(c["average"])
    return d


def record(c):
    """Per call of CALLS on a fresh context of case `c`: the four INFO values and the sha256 of the HASHED fields, or -- a call the
    library refuses -- its return code and error text (the calls behind it are not made)."""
    w = workload(c)
    d = device(c, w)
    out = []
    for steps, finalize in CALLS:
        try:
            (d.step_heun if c["heun"] else d.step)(w["dt"], steps, finalize=finalize)
        except trm._capi.TerrariumHipError as e:
            out.append(dict(refused=e.code, error=str(e)))
            break
        out.append(dict(info=[d.get_option(k) for k in INFO], sha256={n: hashlib.sha256(np.ascontiguousarray(d.get(n)).tobytes()).hexdigest() for n in HASHED}))
    assert d.status() == 0
    d.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        g = json.load(f)
    assert g["info"] == list(INFO) and g["hashed"] == list(HASHED) and g["calls"] == [[n, int(f)] for n, f in CALLS]
    return g["cases"]


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(c["name"] for c in CASES)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_step_calls_launch_what_the_parent_launched(c, golden):
    assert golden[c["name"]]["context"] == c       # (the fixture was recorded for this very context)
    assert record(c) == golden[c["name"]]["after_each_call"], c["name"]
