"""Instruction budget of the headline column program (C3: heat + Richards, fp64, T_TOP signature), checked on the gfx950 device
assembly -- no GPU needed.  The marker build (-DTRM_PHASE_MARKERS) splits the kernel into its phases; profiles/tools/isa_phases.py
counts the vector instructions of the common path.  The shipped build must keep the register budget that gives 8 waves per SIMD
and must not spill."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "terrarium.jl_amd", "csrc")
SOURCE = "trm_launch_column_sig_f64_rich_a"
# k_column<double, RICHARDS, HYD_BC_LINEAR, 32 lanes, DERIVE_T_LIQ, PROG_EULER, no SEB, no series, direct stores, scalar inputs, T_TOP>
SYMBOL = "_ZN3trm8k_columnIdLb1ELi0ELi32ELi1ELi0ELb0ELb0ELb0ELb1ELi2E"
VALU_BUDGET = 240          # common path of the marker build (305 before the glue was cut: DESIGN 4.1)
VGPR_BUDGET = 64           # 8 waves per SIMD


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


pytestmark = pytest.mark.skipif(_hipcc() is None or shutil.which("make") is None, reason="hipcc / make not available")


def _asm(tmp_path, name, extra, source=SOURCE):
    out = tmp_path / name
    subprocess.run(["make", "-s", "-C", CSRC, "asm", f"F={source}", f"OBJDIR={out}", f"EXTRA={extra}", f"HIPCC={_hipcc()}"],
                   check=True, capture_output=True, text=True)
    return str(out / f"{source}.s")


def _resources(txt, symbol):
    m = re.search(r"^" + symbol + r"\w*:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", txt, re.S | re.M)
    assert m, f"kernel {symbol} or its resource summary not found"
    return tuple(int(x) for x in m.groups())


def test_c3_common_path_valu_budget(tmp_path):
    path = _asm(tmp_path, "markers", "-DTRM_PHASE_MARKERS")
    js = str(tmp_path / "phases.json")
    subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "tools", "isa_phases.py"), path, SYMBOL, "--json", js],
                   check=True, capture_output=True, text=True)
    res = json.load(open(js))
    assert res["kernel"] and res["kernel"].startswith(SYMBOL)
    phases = {p["phase"] for p in res["phases"]}
    assert {"tendencies", "advance", "closure", "stores"} <= phases, phases     # the markers are in place
    valu = res["total"]["common"]["VALU"]
    assert valu <= VALU_BUDGET, f"common-path VALU per wave {valu} > {VALU_BUDGET}"


def test_c3_registers_and_scratch(tmp_path):
    txt = open(_asm(tmp_path, "shipped", "")).read()
    vgprs, scratch, occupancy = _resources(txt, SYMBOL)
    assert scratch == 0
    assert vgprs <= VGPR_BUDGET
    assert occupancy == 8


# Columns of 65 ... 128 levels (k_column_deep, two levels per lane, fp64 heat + Richards, reference-default hydraulics, T / liq
# derived): no scratch, and the waves per SIMD of the shipped instances (78 VGPRs / 6 waves for Euler, 100 / 4 for the multi-step
# program; EXPERIMENTS 4.7)
DEEP_SOURCE = "trm_launch_deep_f64"
DEEP_CASES = [("_ZN3trm13k_column_deepIdLb1ELi0ELb1ELi0ELb0E", 6),      # <double, RICHARDS, HYD_BC_LINEAR, DERIVE, PROG_EULER, no GENERIC>
              ("_ZN3trm13k_column_deepIdLb1ELi0ELb1ELi2ELb0E", 4)]      # <double, RICHARDS, HYD_BC_LINEAR, DERIVE, PROG_MULTI, no GENERIC>


def test_deep_column_registers_and_scratch(tmp_path):
    txt = open(_asm(tmp_path, "deep", "", DEEP_SOURCE)).read()
    for symbol, min_occupancy in DEEP_CASES:
        vgprs, scratch, occupancy = _resources(txt, symbol)
        assert scratch == 0, symbol
        assert occupancy >= min_occupancy, (symbol, vgprs, occupancy)
