"""CPU checks of ``batch_plan``: the typed plan of a call's batches, the one ``mmx_block`` record filler and the text a
block too large for a workspace slot is refused with -- each against a restatement written here."""
import numpy as np
import pytest

from magellanmapper_amd import _native as nat
from magellanmapper_amd import batch_plan as bp
from magellanmapper_amd import blob_log as bl

ALIGN = nat.MMX_ROW_ALIGN


def _px(nx):
    return (int(nx) + ALIGN - 1) // ALIGN * ALIGN


def _slot(shape):
    return int(shape[0]) * int(shape[1]) * _px(shape[2])


def _stacked(shapes):
    """Origins of the blocks laid one behind the other along z in the C-contiguous volume that just holds them, and
    that volume's element strides."""
    ny, nx = max(s[1] for s in shapes), max(s[2] for s in shapes)
    z = np.concatenate(([0], np.cumsum([s[0] for s in shapes])))
    return [(int(z[i]), 0, 0) for i in range(len(shapes))], (ny * nx, nx, 1)


CASES = {
    "benchmark": ([(261, 261, 261)] * 256, 5, 16 << 30, None),
    "small": ([(44, 44, 44)] * 48, 3, 96 << 20, None),
    "mixed": ([(50, 60, 70)] * 3 + [(20, 20, 20)] * 4, 5, 64 << 20, None),
    "in_parts": ([(40, 40, 40), (90, 90, 90), (40, 40, 40)], 3, 1 << 30, 9),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_against_a_restatement(case, monkeypatch):
    shapes, ns, budget, halo = CASES[case]
    splits = {}
    if halo is not None:
        monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", int(bl._slot_elems((90, 90, 90))), raising=True)
        assert bl._slot_limit() == 90 * 90 * 96
        splits = {i: bl.split_oversized(s, bl._slot_limit(), halo) for i, s in enumerate(shapes)
                  if _slot(s) >= bl._slot_limit()}
        assert list(splits) == [1] and len(splits[1]) > 1
    origins, strides = _stacked(shapes)
    batches = bl._isolate_parents(bl.plan_batches(shapes, ns, budget), splits)
    plan = bp.make_plan(origins, shapes, batches, splits, strides)
    assert isinstance(plan, bp.BatchPlan) and plan.origins is origins and plan.shapes is shapes
    assert [b.indices for b in plan.batches] == batches
    assert sorted(i for b in batches for i in b) == list(range(len(shapes)))
    n_split = 0
    for b in plan.batches:
        assert isinstance(b, bp.PlannedBatch) and b.d_records is None
        if len(b.indices) == 1 and b.indices[0] in splits:
            sp = splits[b.indices[0]]
            n_split += 1
            assert b.split is sp and b.records is None          # (made when the block is enqueued)
            assert b.n_blocks == len(sp.boxes)
            assert b.slot == max(_slot(hi - lo) for lo, hi in sp.boxes)
            continue
        assert b.split is None
        assert b.n_blocks == len(b.indices)
        assert b.slot == max(_slot(shapes[i]) for i in b.indices)
        rec = b.records
        assert rec.dtype == nat.BLOCK_DTYPE and len(rec) == len(b.indices)
        for j, i in enumerate(b.indices):
            nz, ny, nx = shapes[i]
            assert int(rec["src_off"][j]) == sum(o * s for o, s in zip(origins[i], strides))
            assert (int(rec["nz"][j]), int(rec["ny"][j]), int(rec["nx"][j])) == (nz, ny, nx)
            assert int(rec["slot"][j]) == j and int(rec["px"][j]) == _px(nx)
    assert n_split == len(splits)
    # lanes that preprocess: the same batches, no records anywhere
    bare = bp.make_plan(origins, shapes, batches, splits)
    assert [(b.indices, b.n_blocks, b.slot, b.records) for b in bare.batches] == \
        [(b.indices, b.n_blocks, b.slot, None) for b in plan.batches]


def test_block_records_of_blocks_and_of_parts():
    shapes = [(1, 1, 1), (3, 5, 31), (3, 5, 32), (3, 5, 33)]
    offs = [7, 0, 1 << 40, 12345]
    rec, slot = bp.block_records(offs, shapes)
    assert rec.dtype == nat.BLOCK_DTYPE and rec["src_off"].tolist() == offs
    assert [tuple(int(v) for v in r) for r in zip(rec["nz"], rec["ny"], rec["nx"])] == shapes
    assert rec["slot"].tolist() == [0, 1, 2, 3]
    assert rec["px"].tolist() == [32, 32, 32, 64]
    assert slot == 3 * 5 * 64
    none, slot0 = bp.block_records([], [])
    assert len(none) == 0 and slot0 == 1
    # the parts of a block: offsets from the parent's, rows padded as the BOX is wide
    sp = bl.split_oversized((41, 41, 41), int(bl._slot_elems((41, 41, 41))), 5, grid=(1, 2, 2))
    assert isinstance(sp, bp.PartSplit) and len(sp) == 4
    strides = (100 * 64, 64, 1)
    parent_off = 3 * strides[0] + 2 * strides[1] + 1
    parts, pslot = sp.block_records(parent_off, strides)
    for j in range(4):
        lo, hi = sp.boxes[j]
        assert int(parts["src_off"][j]) == parent_off + sum(int(a) * s for a, s in zip(lo, strides))
        assert (int(parts["nz"][j]), int(parts["ny"][j]), int(parts["nx"][j])) == tuple(int(v) for v in hi - lo)
        assert int(parts["slot"][j]) == j
        assert int(parts["px"][j]) == _px(hi[2] - lo[2])
    assert set(parts["px"].tolist()) == {32} and _px(41) == 64          # (the box's row, not the parent's)
    assert pslot == max(_slot(hi - lo) for lo, hi in sp.boxes)


def test_slot_refusal_text(monkeypatch):
    lib = "block too large for one workspace slot (>= 2^29 voxels)"
    assert bp.slot_refusal(1 << 29) == lib and bp.slot_refusal(1 << 40) == lib
    assert bp.slot_refusal(12345) == "block too large for one workspace slot (>= 12345 elements)"
    assert bp.slot_refusal(bl._slot_limit()) == lib
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", 777, raising=True)
    assert bp.slot_refusal(bl._slot_limit()) == "block too large for one workspace slot (>= 777 elements)"
    with pytest.raises(nat.MmxError) as exc:
        bl.split_oversized((200, 200, 200), 63 * 63 * 64, 31)
    assert str(exc.value).startswith(bp.slot_refusal(63 * 63 * 64) + " and it cannot be cut into parts")
    with pytest.raises(nat.MmxError) as exc:
        bl.split_oversized((4000, 4000, 4000), 1 << 29, 600)
    assert str(exc.value).startswith(lib + " and it cannot be cut into ")
