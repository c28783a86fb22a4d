"""Instruction and register budget of the interior form of the headline column program (C3: heat + Richards, fp64, T_TOP signature,
32 lanes per column, direct stores, scalar inputs), on the gfx950 device assembly -- no GPU needed.  k_column_psi<PSI_INTERIOR> carries
the time of a multi-step call (TRM_OPT_INTERIOR_STEPS): it must keep 8 waves per SIMD without scratch, and the power it adds at entry
(the pressure head) must not outweigh the exit closure it drops -- its marker-build common path is held against the classic
instance's count from the same build.  k_column_psi<PSI_LAST> runs once per call: no scratch."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "terrarium.jl_amd", "csrc")
PSI_SOURCE = "trm_launch_column_psi_f64_b"
CLASSIC_SOURCE = "trm_launch_column_sig_f64_rich_a"
# k_column_psi<HYD_BC_LINEAR, 32 lanes, direct stores, scalar inputs, T_TOP, PSI_INTERIOR | PSI_LAST>
INTERIOR = "_ZN3trm12k_column_psiILi0ELi32ELb0ELb1ELi2ELi2EE"
LAST = "_ZN3trm12k_column_psiILi0ELi32ELb0ELb1ELi2ELi1EE"
# k_column<double, RICHARDS, HYD_BC_LINEAR, 32 lanes, DERIVE_T_LIQ, PROG_EULER, no SEB, no series, direct stores, scalar inputs, T_TOP>
CLASSIC = "_ZN3trm8k_columnIdLb1ELi0ELi32ELi1ELi0ELb0ELb0ELb0ELb1ELi2E"
VGPR_BUDGET = 64           # 8 waves per SIMD


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


pytestmark = pytest.mark.skipif(_hipcc() is None or shutil.which("make") is None, reason="hipcc / make not available")


def _asm(tmp_path, name, extra, source):
    out = tmp_path / name
    subprocess.run(["make", "-s", "-C", CSRC, "asm", f"F={source}", f"OBJDIR={out}", f"EXTRA={extra}", f"HIPCC={_hipcc()}"],
                   check=True, capture_output=True, text=True)
    return str(out / f"{source}.s")


def _resources(txt, symbol):
    m = re.search(r"^" + symbol + r"\w*:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", txt, re.S | re.M)
    assert m, f"kernel {symbol} or its resource summary not found"
    return tuple(int(x) for x in m.groups())


def _common_valu(tmp_path, path, symbol, tag):
    js = str(tmp_path / f"phases_{tag}.json")
    subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "tools", "isa_phases.py"), path, symbol, "--json", js],
                   check=True, capture_output=True, text=True)
    res = json.load(open(js))
    assert res["kernel"] and res["kernel"].startswith(symbol)
    phases = {p["phase"] for p in res["phases"]}
    assert {"tendencies", "advance", "stores"} <= phases, phases     # the markers are in place
    return res["total"]["common"]["VALU"], phases


def test_interior_common_path_is_not_above_the_classic_instance(tmp_path):
    interior, phases = _common_valu(tmp_path, _asm(tmp_path, "markers", "-DTRM_PHASE_MARKERS", PSI_SOURCE), INTERIOR, "interior")
    classic, _ = _common_valu(tmp_path, _asm(tmp_path, "markers", "-DTRM_PHASE_MARKERS", CLASSIC_SOURCE), CLASSIC, "classic")
    print(f"common-path VALU per wave, marker build: interior {interior}, classic {classic}")
    assert interior <= classic, f"common-path VALU per wave: interior {interior} > classic {classic}"


def test_interior_and_last_registers_and_scratch(tmp_path):
    txt = open(_asm(tmp_path, "shipped", "", PSI_SOURCE)).read()
    vgprs, scratch, occupancy = _resources(txt, INTERIOR)
    print(f"interior: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}")
    assert scratch == 0
    assert vgprs <= VGPR_BUDGET
    assert occupancy == 8
    vgprs, scratch, occupancy = _resources(txt, LAST)
    print(f"last: {vgprs} VGPRs, scratch {scratch}, occupancy {occupancy}")
    assert scratch == 0
