"""The store forms of the interior launch (TRM_INTERIOR_STORE_THROUGH, trm_column.hpp; EXPERIMENTS R12.1): k_column_psi<PSI_INTERIOR> may
write internal_energy and saturation -- and the two direct per-column values -- through the L2 (`sc1`), while every other launch and every
copy keeps plain stores and loads (as shipped: U and sat of the direct instances; the staged instances store plain).  Nothing a caller
can observe may depend on the form: every comparison here is byte identity against a second context with interior_steps = 0 (the classic
launches, plain stores) -- every compared field, the status word, the clock and TRM_INFO_LAST_PROGRAM -- and TRM_INFO_INTERIOR_LAUNCHES
must be what the host rule predicts (a fresh context's call of n steps has max(0, n - 2) interior launches, as has the call behind an
upload of U / sat or a restore; any other call n - 1): a test that silently ran classic launches would prove nothing.

The deriving instance is forced at test sizes with derive_closure_fields = 1.  Shapes, the smallest at which a store form can go wrong:
5 columns (one workgroup; the last wave carries a clamped copy), 67 (9 workgroups: every XCD writes at least one), 523 (66 workgroups:
several per XCD, odd); 32 levels and 30 (idle lanes); both compiled hydraulics."""
import os
import subprocess
import sys

import numpy as np
import pytest

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:      # (the child process of the staged case runs this file as a script)
    sys.path.insert(0, _ROOT)

import workloads as W

pytestmark = pytest.mark.gpu

SHAPES = [(ncol, Nz) for ncol in (5, 67, 523) for Nz in (32, 30)]
HYDRAULICS = ["default", "vg"]

_WORKLOADS = {}


def _workload(hydraulics, ncol, Nz):
    """(built once per shape and shared: nothing below changes it)"""
    key = (hydraulics, ncol, Nz)
    if key not in _WORKLOADS:
        lat, lon = W.columns_from_mask("N72")
        sel = np.linspace(0, lat.size - 1, ncol).astype(int)
        _WORKLOADS[key] = W.make_workload("richards", lat[sel], lon[sel], Nz, hydraulics=hydraulics)
    return _WORKLOADS[key]


def _device(w, interior, **options):
    d = W.setup_device(w)
    d.set_option("derive_closure_fields", 1)
    d.set_option("interior_steps", interior)
    for k, v in options.items():
        d.set_option(k, v)
    return d


def _pair(w, **options):
    """(the reference context: classic launches, plain stores; the context under test), identical otherwise"""
    return _device(w, 0, **options), _device(w, 1, **options)


def count(d): return d.get_option("info_interior_launches")


def _same(w, off, on):
    assert on.status() == off.status()
    assert on.clock() == off.clock()
    assert on.last_program() == off.last_program()
    for name in W.compared_fields(w):
        x, y = off.get(name), on.get(name)
        assert x.tobytes() == y.tobytes(), name
    assert count(off) == 0


# ---- 1. call lengths ---------------------------------------------------------------------------------------------------------------
def _call_lengths(w, n, staged=None):
    for finalize in (False, True):
        for asynchronous in (0, 1):
            off, on = _pair(w, asynchronous=asynchronous)
            for s in (off, on):
                s.step(w["dt"], n, finalize=finalize)
            assert count(on) == max(0, n - 2)
            _same(w, off, on)
            if staged is not None:
                assert on.last_program()["staged"] == staged and on.last_program()["scalar_inputs"] == (not staged)
            for s in (off, on):      # (a second call: every launch but the last goes interior, over lines the first call's last launch stored plain)
                s.step(w["dt"], n, finalize=finalize)
            assert count(on) == max(0, n - 2) + n - 1
            _same(w, off, on)


@pytest.mark.parametrize("n", [2, 3, 40])
@pytest.mark.parametrize("hydraulics", HYDRAULICS)
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_call_lengths(ncol, Nz, hydraulics, n):
    _call_lengths(_workload(hydraulics, ncol, Nz), n)


# ---- 2. readers on other paths straight after a call -------------------------------------------------------------------------------
@pytest.mark.parametrize("field", ["internal_energy", "saturation_water_ice", "temperature"])
@pytest.mark.parametrize("hydraulics", HYDRAULICS)
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_a_download_straight_after_an_asynchronous_call(ncol, Nz, hydraulics, field):
    """the first thing behind an asynchronous 7-step call is the download: of U or sat (a copy on the context stream), or of the
    temperature (k_materialize_closure reads U and sat first)"""
    w = _workload(hydraulics, ncol, Nz)
    off, on = _pair(w, asynchronous=1)
    for s in (off, on):
        s.step(w["dt"], 7, finalize=False)
    x, y = off.get(field), on.get(field)
    assert x.tobytes() == y.tobytes()
    assert count(on) == 5
    _same(w, off, on)
    assert x.tobytes() != _device(w, 0).get(field).tobytes()      # (seven steps moved it)


@pytest.mark.parametrize("hydraulics", HYDRAULICS)
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_snapshot_copies_around_calls(ncol, Nz, hydraulics):
    w = _workload(hydraulics, ncol, Nz)
    off, on = _pair(w)
    for s in (off, on):
        s.step(w["dt"], 3, finalize=False)
        s.save_state()
        s.step(w["dt"], 3, finalize=False)
    assert count(on) == 1 + 2
    _same(w, off, on)
    for s in (off, on):
        s.restore_state()
    _same(w, off, on)
    for s in (off, on):      # (the restored pressure head is read as stored by the first launch: one interior launch of the three)
        s.step(w["dt"], 3, finalize=False)
    assert count(on) == 1 + 2 + 1
    _same(w, off, on)


# ---- 3. an upload over lines an interior launch has just written -------------------------------------------------------------------
@pytest.mark.parametrize("field", ["saturation_water_ice", "internal_energy"])
@pytest.mark.parametrize("hydraulics", HYDRAULICS)
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_an_upload_behind_an_interior_call_is_what_is_stepped(ncol, Nz, hydraulics, field):
    w = _workload(hydraulics, ncol, Nz)
    off, on, untouched = _device(w, 0), _device(w, 1), _device(w, 0)
    for s in (off, on, untouched):
        s.step(w["dt"], 3, finalize=False)
    assert count(on) == 1
    x = off.get(field)
    x = x * 0.97 if field == "saturation_water_ice" else x - 2.0e5 * (1.0 + np.arange(x.shape[-1]) % 3)
    for s in (off, on):
        s.set(field, x)
        s.step(w["dt"], 3, finalize=False)
    untouched.step(w["dt"], 3, finalize=False)
    assert count(on) == 1 + 1      # (the first launch behind the upload reads T / liq / psi as stored: a classic launch)
    _same(w, off, on)
    assert on.get(field).tobytes() != untouched.get(field).tobytes()      # (the upload is what was stepped)


# ---- 4. the same lines under both store forms in turn ------------------------------------------------------------------------------
def _alternating(w):
    off, on = _pair(w)
    for call in range(10):
        n = 1 if call % 2 == 0 else 3
        for s in (off, on):
            s.step(w["dt"], n, finalize=False)
    assert count(on) == 5 * 2
    _same(w, off, on)


@pytest.mark.parametrize("hydraulics", HYDRAULICS)
@pytest.mark.parametrize("ncol,Nz", SHAPES)
def test_calls_alternating_between_classic_and_interior(ncol, Nz, hydraulics):
    """ten calls, n = 1 (a classic launch, plain stores) and n = 3 (two interior launches and the call's last) in turn on one context"""
    _alternating(_workload(hydraulics, ncol, Nz))


# ---- 6. the staged + vector-input instances ----------------------------------------------------------------------------------------
def test_staged_instances_in_a_child_process():
    """TRM_STAGED_SMALL=1 TRM_SCALAR_INPUTS=0 (what HBM-resident states take) are read once per process, hence a fresh child process"""
    env = dict(os.environ, TRM_STAGED_SMALL="1", TRM_SCALAR_INPUTS="0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--staged-child"], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "staged child ok" in out.stdout


def _staged_child():
    for ncol, Nz in ((5, 30), (67, 32), (523, 32), (523, 30)):
        for hydraulics in HYDRAULICS:
            w = _workload(hydraulics, ncol, Nz)
            for n in (3, 40):
                _call_lengths(w, n, staged=True)
            _alternating(w)
    print("staged child ok")


if __name__ == "__main__":
    if "--staged-child" in sys.argv:
        _staged_child()
