"""Header / binding agreement of the option and the info keys of TRM_OPT_DEFER_CLOSURE_STORES (append-only: the ABI version stays)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enum():
    header = open(os.path.join(ROOT, "include", "terrarium_hip.h")).read()
    return header, {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(TRM_[A-Z0-9_]+)\s*=\s*(\d+)", header)}


def test_later_options_agree_with_the_header():
    from terrarium_jl_amd import _capi
    _, enum = _enum()
    names = {"defer_closure_stores": "TRM_OPT_DEFER_CLOSURE_STORES", "info_closure_stored": "TRM_INFO_CLOSURE_STORED",
             "info_materializations": "TRM_INFO_MATERIALIZATIONS"}
    assert set(_capi.OPTION_LATER) == set(names)
    for name, key in names.items():
        assert enum[key] == _capi.OPTION_LATER[name] == _capi.option_id(name), name
    assert (enum["TRM_OPT_DEFER_CLOSURE_STORES"], enum["TRM_INFO_CLOSURE_STORED"], enum["TRM_INFO_MATERIALIZATIONS"]) == (12, 106, 107)
    # one id space: no value is used twice, no name sits in both tables
    assert not set(_capi.OPTION) & set(_capi.OPTION_LATER)
    ids = list(_capi.OPTION.values()) + list(_capi.OPTION_LATER.values())
    assert len(ids) == len(set(ids))
    for name, oid in _capi.OPTION.items():
        assert _capi.option_id(name) == oid


def test_abi_version_unchanged():
    header, _ = _enum()
    assert int(re.search(r"#define\s+TRM_ABI_VERSION\s+(\d+)", header).group(1)) == 20


def test_column_args_layout_unchanged():
    """store_closure sits in the padding behind nseries: the stage pointers keep their offsets (kernarg_reload)"""
    src = open(os.path.join(ROOT, "terrarium.jl_amd", "csrc", "trm_column.hpp")).read()
    body = src[src.index("template <class NF> struct ColumnArgs {"):]
    body = re.sub(r"//[^\n]*", "", body[:body.index("};")])
    decls = [d.strip() for d in body.split(";") if d.strip()][0:]
    assert decls[-3:] == ["int nseries", "int store_closure", "NF *stage_sat, *stage_liq, *stage_T, *stage_S"], decls
