"""Header / binding agreement of the option and the info keys of TRM_OPT_DEFER_CLOSURE_STORES (append-only: the ABI version stays)."""
import os
import re

import abi_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_later_options_agree_with_the_header():
    """(the whole table, its one id space and the ABI version: tests/test_abi_tables.py)"""
    from terrarium_jl_amd import _capi
    enum = abi_header.enums()
    assert enum["TRM_OPT_DEFER_CLOSURE_STORES"] == 12 == _capi.OPTION["defer_closure_stores"]
    assert enum["TRM_INFO_CLOSURE_STORED"] == 106 == _capi.OPTION["info_closure_stored"]
    assert enum["TRM_INFO_MATERIALIZATIONS"] == 107 == _capi.OPTION["info_materializations"]


def test_column_args_layout_unchanged():
    """store_closure sits in the padding behind nseries: the stage pointers keep their offsets (kernarg_reload)"""
    src = open(os.path.join(ROOT, "terrarium.jl_amd", "csrc", "trm_column.hpp")).read()
    body = src[src.index("template <class NF> struct ColumnArgs {"):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("};")])
    decls = [d.strip() for d in body.split(";") if d.strip()][0:]
    assert decls[-3:] == ["int nseries", "int store_closure", "NF *stage_sat, *stage_liq, *stage_T, *stage_S"], decls
