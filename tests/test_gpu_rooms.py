"""GPU: the units' and the snapshot levels' device calls at rooms that are no multiple of the block (tests/roomslib.py),
held to the host twins byte for byte as the decision tables of test_gpu_units.py and test_gpu_levels.py are."""
import pytest

import roomslib as R
from test_gpu_levels import SHARE, Tally, device_checked, yard  # noqa: F401  (yard is a fixture)
from test_gpu_units import device_vs_host, st  # noqa: F401  (st is a fixture)

pytestmark = pytest.mark.gpu


def test_units_on_the_device_at_rooms_off_the_block(ro, torch_cuda, st):
    R.units_case_rooms_off_the_block(ro, device_vs_host(ro, torch_cuda, st))


def test_levels_on_the_device_at_rooms_off_the_block(ro, torch_cuda, st, yard):
    tally = Tally()
    R.levels_case_rooms_off_the_block(ro, device_checked(ro, torch_cuda, st, yard, tally))
    assert tally.images >= 1 and tally.share() < SHARE, tally.share()
