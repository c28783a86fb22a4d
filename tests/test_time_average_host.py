"""Time averages without a GPU: the AveragedTimeInterval schedule and the C ABI of the accumulators."""
import ctypes

import pytest

import abi_header
import terrarium_jl_amd as trm


def test_window_starts_and_ends_are_event_times():
    s = trm.AveragedTimeInterval(3 * 3600.0, window=3600.0)
    s.first = 0.0
    assert s.next_time(0.0) == 7200.0 and s.steps_until_next(0.0, 0, 600.0) == 12 and not s.actuates(3600.0, 6)
    assert s.actuates(7200.0, 12) and s.due(7200.0) == [("start", 1)]
    assert s.next_time(7200.0) == 10800.0 and s.steps_until_next(7200.0, 12, 600.0) == 6
    assert s.due(9000.0) == [] and s.due(10800.0) == [("end", 1)]
    assert s.next_time(10800.0) == 18000.0 and s.due(18000.0) == [("start", 2)] and s.due(21600.0) == [("end", 2)]


def test_back_to_back_windows():
    s = trm.AveragedTimeInterval(1800.0)
    assert s.window == 1800.0
    s.first = 100.0
    assert s.due(100.0) == [("start", 1)]                       # the first window starts at initialisation
    assert s.next_time() == 1900.0 and s.steps_until_next(100.0, 0, 700.0) == 3
    assert s.due(1900.0) == [("end", 1), ("start", 2)]          # an end, then the next start at the same time
    assert s.next_time() == 3700.0


@pytest.mark.parametrize("interval,window", [(3600.0, 7200.0), (3600.0, 0.0), (3600.0, -1.0), (0.0, None)])
def test_bad_windows_are_refused(interval, window):
    with pytest.raises(ValueError):
        trm.AveragedTimeInterval(interval, window=window)


def test_library_exports_the_average_entry_points():
    lib = ctypes.CDLL(trm._capi.LIB_PATH)
    for name in ("trm_average_open", "trm_average_reset", "trm_average_read", "trm_average_close"):
        assert name in abi_header.functions(), name
        assert hasattr(lib, name) and name in trm._capi.EXPORTS, name
    assert lib.trm_average_open(None, 2, None) == trm._capi.TRM_EINVAL       # no context: refused, no GPU needed
    assert trm._capi.decode_program(3 | trm._capi.PROGRAM_AVERAGES_IN_LAUNCH)["averages"] == "in_launch"
    assert "averages" not in trm._capi.decode_program(3)
