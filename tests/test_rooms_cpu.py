"""CPU-only: the host twins of the units and of the snapshots' levels at rooms that are no multiple of the block
(tests/roomslib.py), against the emulator and the oracle as the decision tables of test_units_cpu.py and test_levels_cpu.py
are."""
import levelslib as L
import roomslib as R
import unitslib as U


def test_units_twins_at_rooms_off_the_block(ro):
    R.units_case_rooms_off_the_block(ro, U.host_vs_emu(ro))


def test_levels_twin_at_rooms_off_the_block(ro, oracle):
    R.levels_case_rooms_off_the_block(ro, L.host_vs_oracle(ro, oracle))
