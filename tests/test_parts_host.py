"""CPU checks of ``blob_log.split_oversized``: the pure function that cuts a block too large for one workspace slot into
overlapping parts.  Its properties over a sweep of shapes, limits, halos and alignments: the cores
partition the block, a box is its core plus the halo (out to the alignment, clipped to the block), every box stays under
the limit, faces that are not faces of the block lie on the alignment, and a block that cannot be cut is refused."""
import itertools

import numpy as np
import pytest

SHAPES = [(40, 48, 52), (70, 72, 80), (33, 65, 129), (7, 200, 31), (1, 90, 300), (64, 64, 64), (101, 37, 53)]
HALOS = [0, 1, 5, 9, 31]
ALIGNS = [(1, 1, 1), (8, 8, 8), (25, 25, 25), (4, 16, 32), (64, 64, 64)]
#: the limit as a fraction of the unsplit block's own slot (1.0: the block just does not fit)
FRACTIONS = [1.0, 0.75, 0.5, 0.3, 0.12]


def _slot(shape):
    nz, ny, nx = (int(v) for v in shape)
    return nz * ny * (-(-nx // 32) * 32)


def _sweep():
    return list(itertools.product(SHAPES, HALOS, ALIGNS, FRACTIONS))


def _try_split(shape, limit, halo, align):
    from magellanmapper_amd import _native as nat, blob_log as bl
    try:
        return bl.split_oversized(shape, limit, halo, align)
    except nat.MmxError:
        return None


def test_slot_elems_is_the_padded_row_count():
    from magellanmapper_amd import blob_log as bl
    for shape in SHAPES:
        assert int(bl._slot_elems(shape)) == _slot(shape)
    assert bl.MAX_SLOT_ELEMS == 1 << 29 and bl._slot_limit() == 1 << 29


def test_the_limit_cannot_be_raised_above_the_librarys(monkeypatch):
    from magellanmapper_amd import blob_log as bl
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", 1 << 40, raising=True)
    assert bl._slot_limit() == 1 << 29
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", 12345, raising=True)
    assert bl._slot_limit() == 12345


def test_sweep_splits_most_cases():
    """The sweep is worth something: most of its cases split, into grids of every kind."""
    splits = [_try_split(s, int(_slot(s) * f), h, a) for s, h, a, f in _sweep()]
    done = [sp for sp in splits if sp is not None]
    assert len(done) > 0.6 * len(splits)
    assert any(min(sp.grid) > 1 for sp in done) and any(sorted(sp.grid)[:2] == [1, 1] for sp in done)
    assert len(done) < len(splits)          # ... and some are refused (their properties: the test below)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_properties_of_the_split(shape):
    n_split = 0
    for halo, align, frac in itertools.product(HALOS, ALIGNS, FRACTIONS):
        limit = int(_slot(shape) * frac)
        sp = _try_split(shape, limit, halo, align)
        if sp is None:
            continue
        n_split += 1
        ctx = (shape, halo, align, limit, sp.grid)
        n = len(sp)
        assert n == int(np.prod(sp.grid)) >= 2 and sp.cores.shape == sp.boxes.shape == (n, 2, 3), ctx
        # the cores partition the parent: every voxel in exactly one
        owner = np.zeros(shape, dtype=np.int32)
        for lo, hi in sp.cores:
            assert (hi > lo).all(), ctx
            owner[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 1
        assert (owner == 1).all(), ctx
        # ... as the grid of the cut planes
        for ax in range(3):
            cuts = sp.cuts[ax]
            assert cuts[0] == 0 and cuts[-1] == shape[ax] and (np.diff(cuts) > 0).all() and len(cuts) == sp.grid[ax] + 1, ctx
            assert set(sp.cores[:, 0, ax]) | {shape[ax]} == set(cuts) == set(sp.cores[:, 1, ax]) | {0}, ctx
        for (clo, chi), (blo, bhi) in zip(sp.cores, sp.boxes):
            for ax in range(3):
                a = align[ax]
                # box = core +- halo, out to the alignment, clipped to the parent
                want_lo = max(0, clo[ax] - halo) // a * a
                want_hi = min(shape[ax], -(-(chi[ax] + halo) // a) * a)
                assert (blo[ax], bhi[ax]) == (want_lo, want_hi), ctx
                # so it holds the core and its halo wherever the parent has voxels there ...
                assert blo[ax] <= max(0, clo[ax] - halo) and bhi[ax] >= min(shape[ax], chi[ax] + halo), ctx
                # ... and its faces are faces of the parent or lie on the alignment
                assert blo[ax] == 0 or blo[ax] % a == 0, ctx
                assert bhi[ax] == shape[ax] or bhi[ax] % a == 0, ctx
                if a == 1:
                    assert blo[ax] == max(0, clo[ax] - halo) and bhi[ax] == min(shape[ax], chi[ax] + halo), ctx
            # every box is under the limit
            assert _slot(bhi - blo) < limit, ctx
        # the part records speak part coordinates
        rec = sp.records(3)
        assert (rec["parent"] == 3).all()
        np.testing.assert_array_equal(rec["off"], sp.boxes[:, 0])
        np.testing.assert_array_equal(rec["off"] + rec["core_lo"], sp.cores[:, 0])
        np.testing.assert_array_equal(rec["off"] + rec["core_hi"], sp.cores[:, 1])
    assert n_split >= 10, n_split


def test_as_few_parts_as_possible_longest_axis_first():
    """No grid of fewer parts stays under the limit, and where one cut is enough it goes across the longest axis whose
    cut saves a padded row."""
    from magellanmapper_amd import blob_log as bl
    for shape, halo, frac in itertools.product(SHAPES[:4], (1, 5, 9), (0.75, 0.5, 0.3)):
        limit = int(_slot(shape) * frac)
        sp = _try_split(shape, limit, halo, (1, 1, 1))
        if sp is None:
            continue
        for grid in itertools.product(range(1, 9), repeat=3):
            if int(np.prod(grid)) >= len(sp) or any(g > n for g, n in zip(grid, shape)):
                continue
            with pytest.raises(Exception):
                bl.split_oversized(shape, limit, halo, grid=grid)
    assert bl.split_oversized((40, 48, 300), int(_slot((40, 48, 300)) * 0.8), 5).grid == (1, 1, 2)
    assert bl.split_oversized((40, 300, 64), int(_slot((40, 300, 64)) * 0.8), 5).grid == (1, 2, 1)
    assert bl.split_oversized((300, 40, 64), int(_slot((300, 40, 64)) * 0.8), 5).grid == (2, 1, 1)


def test_the_grids_the_gpu_tests_rely_on():
    from magellanmapper_amd import blob_log as bl
    assert bl.split_oversized((40, 48, 52), 30000, 6).grid == (2, 2, 2)
    assert bl.split_oversized((40, 48, 52), 70000, 7).grid == (1, 1, 3)
    forced = bl.split_oversized((70, 72, 80), 460000, 31, grid=(1, 2, 2))
    assert forced.grid == (1, 2, 2) and len(forced) == 4


def test_unsplittable_parents_are_refused_with_the_reason():
    from magellanmapper_amd import _native as nat, blob_log as bl
    # the halo alone fills a slot: (2 * 31 + 1)^2 rows of 64 elements
    with pytest.raises(nat.MmxError, match=r"block too large for one workspace slot.*halo of 31 voxels.*segment_size"):
        bl.split_oversized((200, 200, 200), 63 * 63 * 64, 31)
    assert len(bl.split_oversized((200, 200, 200), 131 * 131 * 160 + 1, 31)) == 8      # (cores of 100, boxes of 131)
    # with the default limit the message is the one the unsplit path has always raised, and the reason
    with pytest.raises(nat.MmxError, match=r"block too large for one workspace slot \(>= 2\^29 voxels\)"):
        bl.split_oversized((4000, 4000, 4000), 1 << 29, 600)
    # an alignment coarser than the room the limit leaves
    with pytest.raises(nat.MmxError, match="cannot be cut"):
        bl.split_oversized((100, 100, 100), 40 * 40 * 64, 3, (64, 64, 64))
    # a forced grid whose boxes do not fit
    with pytest.raises(nat.MmxError, match="1 x 2 x 2 grid"):
        bl.split_oversized((70, 72, 80), 400000, 31, grid=(1, 2, 2))
    with pytest.raises(ValueError):
        bl.split_oversized((70, 72), 400000, 31)


def test_the_default_profile_at_fine_resolutions_splits():
    """The blocks the issue names: 843^3 (0.6 um/px) and 1009^3 (0.5 um/px) under the library's own limit."""
    from magellanmapper_amd import blob_log as bl
    for n, halo in ((843, 35), (1009, 41)):
        shape = (n, n, n)
        assert int(bl._slot_elems(shape)) >= 1 << 29
        sp = bl.split_oversized(shape, 1 << 29, halo)
        assert 2 <= len(sp) <= 4
        assert int(bl._slot_elems(sp.box_shapes).max()) < 1 << 29
    assert int(bl._slot_elems((778, 778, 778))) < 1 << 29


def test_plan_isolates_blocks_in_parts():
    from magellanmapper_amd import blob_log as bl
    splits = {2: object(), 5: object()}
    assert bl._isolate_parents([[0, 1, 2, 3], [4], [5, 6]], splits) == [[0, 1], [2], [3], [4], [5], [6]]
    assert bl._isolate_parents([[0, 1]], {}) == [[0, 1]]
