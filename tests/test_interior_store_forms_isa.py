"""Store forms of the interior launch on the gfx950 device assembly -- no GPU needed.  TRM_INTERIOR_STORE_THROUGH (trm_column.hpp) selects
at compile time how k_column_psi<PSI_INTERIOR> stores: 0 plain, 1 internal_energy and saturation written through the L2
(`global_store_dwordx2 ... sc1`, an agent-scope relaxed store), 2 the two direct per-column stores (surface_excess_water, water table) as
well.  The expectation is stated from the macro's shipped value, so this file holds whichever default the measurement selected
(EXPERIMENTS R12.1).  Every other launch -- here k_column_psi<PSI_LAST> and the classic C3 k_column instance -- keeps plain stores, and
the interior store block stays straight-line: no cache write-back or invalidate instruction in it."""
import os
import re

import pytest

from test_interior_isa_budget import CLASSIC, CLASSIC_SOURCE, CSRC, INTERIOR, LAST, PSI_SOURCE, _asm, pytestmark      # noqa: F401

THROUGH = "sc1"


def _shipped_value():
    src = open(os.path.join(CSRC, "trm_column.hpp")).read()
    m = re.search(r"#ifndef TRM_INTERIOR_STORE_THROUGH\s*\n#define TRM_INTERIOR_STORE_THROUGH (\d)\s*\n#endif", src)
    assert m, "the default of TRM_INTERIOR_STORE_THROUGH not found in trm_column.hpp"
    return int(m.group(1))


def _body(txt, symbol):
    m = re.search(r"^(" + symbol + r"\w*):[^\n]*\n(.*?)^\s*\.size\s+\1,", txt, re.S | re.M)
    assert m, f"kernel {symbol} not found"
    return [line.strip() for line in m.group(2).splitlines()]


def _stores(body):
    return [line for line in body if line.startswith("global_store_")]


def _modifiers(line):
    return line.split(";")[0].split()[1:]


@pytest.fixture(scope="module")
def shipped(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("store_forms")
    return open(_asm(tmp, "shipped", "", PSI_SOURCE)).read(), open(_asm(tmp, "shipped", "", CLASSIC_SOURCE)).read()


def test_interior_stores_follow_the_shipped_macro(shipped):
    value = _shipped_value()
    assert value in (0, 1, 2)
    body = _body(shipped[0], INTERIOR)
    stores = _stores(body)
    print(f"TRM_INTERIOR_STORE_THROUGH = {value}; interior stores:", *stores, sep="\n  ")
    # the direct instance: U, sat, then (top lane) surface_excess_water and the water table -- four 8-byte stores, in this order of issue
    # for the fields (the per-column pair sits in the top-lane block behind them)
    assert len(stores) == 4 and all(s.startswith("global_store_dwordx2") for s in stores), stores
    through = [THROUGH in _modifiers(s) for s in stores]
    expected = {0: [False] * 4, 1: [True, True, False, False], 2: [True] * 4}[value]
    assert through == expected, (value, stores)
    # straight-line: nothing that writes back or invalidates a cache, whatever the macro says
    assert not [line for line in body if re.match(r"(buffer_wbl2|buffer_inv|buffer_wbinvl1|s_dcache_inv)\b", line)]


def test_every_other_launch_keeps_plain_stores(shipped):
    for name, txt, symbol in (("PSI_LAST", shipped[0], LAST), ("classic k_column", shipped[1], CLASSIC)):
        stores = _stores(_body(txt, symbol))
        assert stores, name
        written_through = [s for s in stores if THROUGH in _modifiers(s) or "sc0" in _modifiers(s) or "nt" in _modifiers(s)]
        assert not written_through, (name, written_through)
