"""Every enum table of terrarium.jl_amd/_capi.py against the header, in both directions: a table equals the dict the naming rule of
tests/abi_header.py gives for its prefix, so a name or a value that only one side has fails here, whichever side it is on."""
import pytest

import abi_header as H
from terrarium_jl_amd import _capi


def _constants(prefix, strip=0) -> dict:
    """the module-level integer constants `prefix`* of _capi, by their names without the first `strip` characters"""
    return {name[strip:]: value for name, value in vars(_capi).items() if name.startswith(prefix) and type(value) is int}


def _upper(table) -> dict:
    return {name.upper(): value & 0xffffffff for name, value in table.items()}     # (TRM_PROGRAM_PARAMETERS, bit 31 of a C int, is negative there)


def _positions(names, **more) -> dict:
    return {**{name: at for at, name in enumerate(names)}, **more}


# name: (the Python side, the header side), each built when its row runs; a *_COUNT enumerator is held to the table's length as `count`
ROWS = {
    "FIELD": (lambda: {**_capi.FIELD, "count": len(_capi.FIELD)}, lambda: H.table("TRM_FIELD_", dict(STEM_AREA_INDEX="SAI", CO2="CO2"))),
    "OPTION": (lambda: _capi.OPTION, lambda: {**H.table("TRM_OPT_", dict(ASYNC="asynchronous")), **{"info_" + n: v for n, v in H.table("TRM_INFO_").items()}}),
    "TANGENT": (lambda: _capi.TANGENT, lambda: H.table("TRM_TANGENT_", exclude=("RECORD_",))),
    "ADJOINT": (lambda: _capi.ADJOINT, lambda: H.table("TRM_ADJOINT_")),
    "TANGENT_RECORD": (lambda: _capi.TANGENT_RECORD, lambda: H.table("TRM_TANGENT_RECORD_")),
    "THERMAL_PARAMS": (lambda: _positions(_capi.THERMAL_PARAMS, count=len(_capi.THERMAL_PARAMS)), lambda: H.table("TRM_THERMAL_PARAM_")),
    "PROGRAM": (lambda: _positions(_capi.PROGRAM), lambda: H.table("TRM_PROGRAM_", exclude=("AVERAGES_", "PARAMETERS"))),
    "PROGRAM_*": (lambda: _constants("PROGRAM_", strip=8), lambda: _upper({n: v for n, v in H.table("TRM_PROGRAM_").items() if n.startswith(("averages_", "parameters"))})),
    "BC_KIND": (lambda: _capi.BC_KIND, lambda: H.table("TRM_BC_")),
    "SIDE": (lambda: _capi.SIDE, lambda: dict(bottom=H.enums()["TRM_BOTTOM"], top=H.enums()["TRM_TOP"])),
    "BC_VAR": (lambda: {**_capi.BC_VAR, "count": len(_capi.BC_VAR)}, lambda: H.table("TRM_BCV_")),
    "FLOW": (lambda: _capi.FLOW, lambda: H.table("TRM_FLOW_")),
    "SWRC": (lambda: _capi.SWRC, lambda: H.table("TRM_SWRC_")),
    "UNSATK": (lambda: _capi.UNSATK, lambda: H.table("TRM_UNSATK_")),
    "HALO": (lambda: _capi.HALO, lambda: H.table("TRM_HALO_")),
    "VEGETATION": (lambda: _capi.VEGETATION, lambda: H.table("TRM_VEGETATION_")),
    "REDUCE": (lambda: _capi.REDUCE, lambda: H.table("TRM_REDUCE_")),
    "KERNEL": (lambda: _capi.KERNEL, lambda: H.table("TRM_KERNEL_")),
    "TIME_INDEXING": (lambda: _capi.TIME_INDEXING, lambda: H.table("TRM_TIME_")),
    "error codes": (lambda: {**_constants("TRM_OK"), **_constants("TRM_E")}, lambda: {n: v for n, v in H.enums().items() if n == "TRM_OK" or n.startswith("TRM_E")}),
    "STATUS_*": (lambda: _constants("STATUS_", strip=7), lambda: _upper(H.table("TRM_STATUS_", dict(COMPOSITION_OUT_OF_RANGE="composition")))),
    "TRM_F64, TRM_F32": (lambda: _constants("TRM_F"), lambda: {n: v for n, v in H.enums().items() if n in ("TRM_F64", "TRM_F32")}),
}


@pytest.mark.parametrize("what", ROWS)
def test_table_is_the_header_enum(what):
    python, header = (side() for side in ROWS[what])
    assert python and python == header, (f"{what}: _capi alone has {sorted(set(python.items()) - set(header.items()))}, "
                                         f"the header alone has {sorted(set(header.items()) - set(python.items()))}")


def test_options_are_one_id_space():
    ids = list(_capi.OPTION.values())
    assert len(ids) == len(set(ids))


def test_abi_version_and_the_adjoint_intervals():
    define = H.defines()
    assert define["TRM_ABI_VERSION"] == 20 == _capi.lib().trm_abi_version()
    assert define["TRM_ADJOINT_MAX_INTERVAL"] == _capi.ADJOINT_MAX_INTERVAL and define["TRM_ADJOINT_DEFAULT_INTERVAL"] == _capi.ADJOINT_DEFAULT_INTERVAL
    assert 1 <= _capi.ADJOINT_DEFAULT_INTERVAL <= _capi.ADJOINT_MAX_INTERVAL


def test_binding_covers_the_declared_entry_points():
    assert H.functions() == sorted(_capi.EXPORTS) and len(H.functions()) == len(_capi.EXPORTS)


def test_the_parser_on_a_known_string():
    source = """
        #define TRM_X_VERSION 7   /* a comment */
        #define TRM_X_MASK 0x10u
        #define TRM_X_NAME "text"
        enum { TRM_A_ONE = 1, /* TRM_A_GONE = 2, */ TRM_A_HEX = 0x1F,
               TRM_A_BIT = 1u << 3   // TRM_A_LINE = 9
               ,TRM_A_NEXT };
        enum { TRM_B_LOW = (-2147483647 - 1) }; enum trm_named { TRM_B_ZERO, TRM_B_RECORD_ONE };
        int trm_first(int a);   /* int trm_commented(void); */
        const char* trm_second (void);
    """
    assert H.enums(source) == dict(TRM_A_ONE=1, TRM_A_HEX=31, TRM_A_BIT=8, TRM_A_NEXT=9, TRM_B_LOW=-2 ** 31, TRM_B_ZERO=0, TRM_B_RECORD_ONE=1)
    assert H.defines(source) == dict(TRM_X_VERSION=7, TRM_X_MASK=16)
    assert H.functions(source) == ["trm_first", "trm_second"]
    assert H.table("TRM_B_", dict(LOW="lowest"), exclude=("RECORD_",), source=source) == dict(lowest=-2 ** 31, zero=0)
    with pytest.raises(AssertionError):
        H.enums("enum { TRM_A_ONE = 1 }; enum { TRM_A_ONE = 2 };")
