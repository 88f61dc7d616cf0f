"""The row march's schedule (``mmx_fused4.hip``: ``zx4_rows_rule`` and the flat grid made from it), through the host entry
``mmx_zx_rows_schedule``: rows per wave of every block of a launch, and which wave of the grid owns which row.  No GPU.
"""
import ctypes

import numpy as np
import pytest

SLOTS = 2048            # 256 CUs x 2 workgroups of 4 waves: the pair kernel on an MI355X


@pytest.fixture(scope="module")
def sched():
    from magellanmapper_amd import _native as nat
    L = ctypes.CDLL(nat.LIB_PATH)
    f = L.mmx_zx_rows_schedule
    i32p = ctypes.POINTER(ctypes.c_int32)
    f.argtypes = [ctypes.c_int, i32p, i32p, ctypes.c_int, ctypes.c_int, i32p, i32p]
    f.restype = ctypes.c_int

    def run(rows, wpr, slots=SLOTS, forced=0, cover=True):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        wpr = np.ascontiguousarray(wpr, dtype=np.int32)
        nr = np.zeros(len(rows), dtype=np.int32)
        cov = np.full(int((rows.astype(np.int64) * wpr).sum()), -7, dtype=np.int32) if cover else None
        wgs = f(len(rows), rows.ctypes.data_as(i32p), wpr.ctypes.data_as(i32p), slots, forced, nr.ctypes.data_as(i32p),
                cov.ctypes.data_as(i32p) if cover else None)
        return wgs, nr, cov
    return run


# (rows, waves per row) per block: the headline batches (261 rows, 17 column tiles in 9 pairs) at the sizes of its taper,
# small launches, ragged blocks, one block
LAUNCHES = {
    "c3_22": [(261, 9)] * 22, "c3_16": [(261, 9)] * 16, "c3_10": [(261, 9)] * 10, "c3_6": [(261, 9)] * 6, "c3_4": [(261, 9)] * 4,
    "one": [(261, 9)], "tiny": [(13, 2), (13, 1), (20, 2)],
    "ragged": [(261, 9)] * 9 + [(100, 5), (261, 3), (17, 9)] * 3 + [(261, 9)] * 5,
    "many_small": [(40, 3)] * 400,
}


@pytest.mark.parametrize("name", sorted(LAUNCHES))
def test_rule_tapers_and_covers_every_row_once(sched, name):
    rows, wpr = (np.array(v) for v in zip(*LAUNCHES[name]))
    wgs, nr, cov = sched(rows, wpr)
    assert wgs > 0 and wgs % 8 == 0
    assert (nr >= 1).all() and (nr <= 2).all()
    assert (np.diff(nr) <= 0).all(), nr                                   # never grows from block to block
    assert nr[-1] == 1
    # one row per wave for at least the last resident slots' worth of wave-rows (or the whole launch)
    work = rows.astype(np.int64) * wpr
    first_one = int(np.flatnonzero(nr == 1)[0])
    assert work[first_one:].sum() >= min(SLOTS, work.sum()), (nr, work)
    # a block with n rows per wave has n slot counts of wave-rows behind it: its waves end before the launch does
    behind = work.sum() - np.cumsum(work)
    assert (behind[nr > 1] >= nr[nr > 1].astype(np.int64) * SLOTS).all()
    assert (cov == 1).all(), (name, np.unique(cov, return_counts=True))


def test_small_launches_keep_one_row_per_wave(sched):
    for name in ("c3_4", "c3_6", "one", "tiny"):
        rows, wpr = (np.array(v) for v in zip(*LAUNCHES[name]))
        assert (sched(rows, wpr)[1] == 1).all(), name
    # ... and so does any launch on a device whose slots are unknown
    rows, wpr = (np.array(v) for v in zip(*LAUNCHES["c3_22"]))
    assert (sched(rows, wpr, slots=0)[1] == 1).all()


def test_large_launches_march_several_rows(sched):
    rows, wpr = (np.array(v) for v in zip(*LAUNCHES["c3_22"]))
    wgs, nr, _ = sched(rows, wpr)
    assert nr[0] == 2 and set(nr.tolist()) == {1, 2}
    # fewer workgroups than one row per wave takes
    assert wgs < sched(rows, wpr, forced=1)[0]


@pytest.mark.parametrize("forced", [1, 2, 3, 4, 8, 15])
@pytest.mark.parametrize("name", ["tiny", "ragged", "c3_4"])
def test_forced_rows_cover_every_row_once(sched, name, forced):
    rows, wpr = (np.array(v) for v in zip(*LAUNCHES[name]))
    wgs, nr, cov = sched(rows, wpr, forced=forced)
    assert wgs > 0 and (nr == forced).all() and (cov == 1).all()


def test_arguments_are_checked(sched):
    assert sched([0], [1])[0] < 0 and sched([4], [0])[0] < 0
    assert sched([4], [1], forced=16)[0] < 0 and sched([4], [1], forced=-1)[0] < 0
