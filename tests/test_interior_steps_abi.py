"""TRM_OPT_INTERIOR_STEPS / TRM_INFO_INTERIOR_LAUNCHES: appended to the ABI (version unchanged), the header and the Python table agree."""
import os
import re

import terrarium_jl_amd as trm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "terrarium_hip.h")).read()


def _enum(name):
    m = re.search(r"\b" + name + r"\s*=\s*(\d+)", HEADER)
    assert m, name
    return int(m.group(1))


def test_header_and_python_agree_on_the_two_ids():
    capi = trm._capi
    assert _enum("TRM_OPT_INTERIOR_STEPS") == 13 == capi.OPTION_INTERIOR["interior_steps"] == capi.option_id("interior_steps")
    assert _enum("TRM_INFO_INTERIOR_LAUNCHES") == 108 == capi.OPTION_INTERIOR["info_interior_launches"] == capi.option_id("info_interior_launches")
    # one id space: the tables pinned by earlier tests (OPTION, OPTION_LATER) stay as they are, no name or value is used twice
    tables = (capi.OPTION, capi.OPTION_LATER, capi.OPTION_INTERIOR)
    names = [n for t in tables for n in t]
    ids = [v for t in tables for v in t.values()]
    assert len(names) == len(set(names)) and len(ids) == len(set(ids))
    for t in tables:
        for name, oid in t.items():
            assert capi.option_id(name) == oid


def test_abi_version_is_unchanged():
    assert int(re.search(r"#define\s+TRM_ABI_VERSION\s+(\d+)", HEADER).group(1)) == 20
