"""GPU check of the event snapshots on the device (csrc/ro_snapshots.hip) across slots: what snap_plan_kernel carries from
one slot's tiles into the next slot's -- the directory index and the packed rows, which are the bases the shared plan code
(csrc/ro_pack_plan.h) adds its tile prefixes to -- against ro_snapshots_host byte for byte.  The harness is
tests/test_gpu_snapshots.py's.  Nothing here has a tolerance."""
import numpy as np
import pytest

from snapshotslib import Case, image_of
from test_gpu_snapshots import TILE, device_vs_host, handle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("room", ["everything", "out in the second slot's second tile"])
def test_two_slots_of_300_events_carry_the_prefixes_from_slot_to_slot(ro, torch_cuda, room):
    """300 capturable events in each of two slots, cols = 8, snapshot_rows = 2, a ring that holds every row: the directory
    index and the packed rows that slot 0's two tiles leave are the bases of slot 1's two tiles.  With the short arena the
    room ends in front of slot 1's candidate 270, inside its second tile"""
    torch = torch_cuda
    head, ring_rows, cols, snap, n, last = 2000, 1024, 8, 2, 300, 270
    # images of one or two rows, so that the packed rows are not the directory index times a constant
    spans = {s: [(head - ring_rows + (7 * i + 3 * s) % (ring_rows - snap), 1 + (i + s) % 3) for i in range(n)] for s in (0, 1)}
    rows = {s: [min(length, snap) for _, length in spans[s]] for s in (0, 1)}
    fit = sum(rows[0]) + sum(rows[1]) if room == "everything" else sum(rows[0]) + sum(rows[1][:last])
    case = Case(ro, spans, snap, ring_rows, cols, head, fit * cols, pcap=40)
    assert case.mask == 0b11 and case.capacity == n and last > TILE
    with handle(ro) as st:
        r = device_vs_host(ro, torch, st)(case)
    s = r.summary
    captured = 2 * n if room == "everything" else n + last
    assert (int(s["captured"]), int(s["resolved"]), int(s["arena_floats"])) == (captured, captured, fit * cols), s
    assert int(s["empty"]) == int(s["lost"]) == int(s["pending_dropped"]) == 0
    assert r.pending_count.tolist() == [0, 2 * n - captured] and int(s["pending"]) == 2 * n - captured
    # slot 1 starts behind all of slot 0, in the directory and in the arena; its last entry is the last one that fits
    assert r.dir["slot"].tolist() == [0] * n + [1] * (captured - n)
    assert int(r.dir[n]["offset"]) == sum(rows[0]) * cols and r.dir[n]["event"].tobytes() == case.events[1, 0].tobytes()
    assert r.dir[-1]["event"].tobytes() == case.events[1, captured - n - 1].tobytes()
    assert int(r.dir[-1]["offset"]) + int(r.dir[-1]["rows"]) * cols == fit * cols
    for i in (0, TILE, n - 1, n, n + TILE, captured - 1):
        assert np.array_equal(r.image(i, cols), image_of(int(r.dir[i]["first_row"]), int(r.dir[i]["rows"]), cols)), i
