"""TRM_OPT_INTERIOR_STEPS / TRM_INFO_INTERIOR_LAUNCHES: appended to the ABI (version unchanged), the header and the Python table agree."""
import abi_header
import terrarium_jl_amd as trm


def test_header_and_python_agree_on_the_two_ids():
    """(the whole table, its one id space and the ABI version: tests/test_abi_tables.py)"""
    enum, option = abi_header.enums(), trm._capi.OPTION
    assert enum["TRM_OPT_INTERIOR_STEPS"] == 13 == option["interior_steps"]
    assert enum["TRM_INFO_INTERIOR_LAUNCHES"] == 108 == option["info_interior_launches"]
