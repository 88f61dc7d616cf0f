"""The integer geometry of a ``blob_log`` call: workspace slots, blocks cut into parts, the batches of a block list, the
``mmx_block`` records and the typed plan the pipeline of :mod:`blob_log` runs (:class:`BatchPlan`).  Pure functions of
their arguments -- no torch, no library call, no GPU -- that take every tunable as an argument: the settings themselves
(``MAX_SLOT_ELEMS``, ``TAPER``, ``RAMP``, ...) are attributes of :mod:`blob_log`, which passes them down."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat

#: the library refuses a workspace slot of this many elements itself (its kernels address a slot with 32-bit byte offsets)
LIB_MAX_SLOT_ELEMS = 1 << 29
#: most parts one block is cut into (the search for the smallest grid stops there)
MAX_PARTS = 4096


def _row_elems(nx):
    """Elements of a workspace row that holds ``nx`` voxels: rows are ``MMX_ROW_ALIGN`` elements (128 bytes) aligned."""
    return -(-nx // nat.MMX_ROW_ALIGN) * nat.MMX_ROW_ALIGN


def _slot_elems(shapes):
    """Workspace elements a block of ``(nz, ny, nx)`` voxels takes, its rows padded (:func:`_row_elems`).  One shape
    gives one number, an ``(n, 3)`` list of shapes an array of ``n``."""
    shp = np.asarray(shapes, dtype=np.int64)
    return shp[..., 0] * shp[..., 1] * _row_elems(shp[..., 2])


def slot_limit(max_slot_elems: int) -> int:
    """The slot size from which a block is detected in parts: the setting, at most what the library takes."""
    return max(1, min(int(max_slot_elems), LIB_MAX_SLOT_ELEMS))


def slot_refusal(limit: int) -> str:
    """How a block whose slot reaches ``limit`` is refused: the library's own limit, or a lowered one."""
    return "block too large for one workspace slot (>= 2^29 voxels)" if limit >= LIB_MAX_SLOT_ELEMS else \
        f"block too large for one workspace slot (>= {limit} elements)"


def batch_slot(shapes) -> int:
    """The slot size a batch of blocks of ``shapes`` needs: that of its largest block."""
    return max(1, int(_slot_elems(np.asarray(shapes, dtype=np.int64).reshape(-1, 3)).max(initial=0)))


def block_records(src_offsets, shapes) -> Tuple[np.ndarray, int]:
    """``mmx_block`` records of blocks of ``shapes`` whose first voxels lie ``src_offsets`` elements into their volume
    (block i owns slot i), and the workspace slot size they need."""
    shp = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    blocks = np.zeros(len(shp), dtype=nat.BLOCK_DTYPE)
    blocks["src_off"] = src_offsets
    blocks["nz"], blocks["ny"], blocks["nx"] = shp[:, 0], shp[:, 1], shp[:, 2]
    blocks["slot"] = np.arange(len(shp))
    blocks["px"] = _row_elems(shp[:, 2])
    return blocks, batch_slot(shp)


@dataclass
class PartSplit:
    """One block (the *parent*) cut into parts: ``grid`` parts per axis, ``cuts[axis]`` the ``grid[axis] + 1`` planes
    between the cores (0 and the extent included), and per part, in C order of the grid, ``cores`` and ``boxes`` as
    ``[lo, hi)`` corners in parent coordinates, shape ``(n, 2, 3)``.  The cores partition the parent; a box is its core
    extended by the halo on every side, out to the next multiple of ``align`` where one is asked for, clipped to the
    parent."""
    shape: Tuple[int, int, int]
    halo: int
    grid: Tuple[int, int, int]
    cuts: Tuple[np.ndarray, np.ndarray, np.ndarray]
    cores: np.ndarray
    boxes: np.ndarray

    def __len__(self) -> int:
        return len(self.cores)

    @property
    def box_shapes(self) -> np.ndarray:
        return self.boxes[:, 1] - self.boxes[:, 0]

    def records(self, parent: int = 0) -> np.ndarray:
        """The ``mmx_part`` records (``mmx_fold_parts``): cores in part coordinates."""
        rec = np.zeros(len(self), dtype=nat.PART_DTYPE)
        rec["parent"] = parent
        rec["off"] = self.boxes[:, 0]
        rec["core_lo"] = self.cores[:, 0] - self.boxes[:, 0]
        rec["core_hi"] = self.cores[:, 1] - self.boxes[:, 0]
        return rec

    def block_records(self, parent_off: int, strides) -> Tuple[np.ndarray, int]:
        """:func:`block_records` of the parts of a parent that lies ``parent_off`` elements into a volume of element
        ``strides`` (z, y, x)."""
        return block_records(int(parent_off) + self.boxes[:, 0] @ np.asarray(strides, dtype=np.int64), self.box_shapes)


def _axis_pieces(n: int, g: int, halo: int, a: int):
    """``g`` cores along an axis of ``n`` voxels and their boxes: ``(cuts, box_lo, box_hi)``, or None when ``n`` voxels
    do not make ``g`` cores."""
    if g > n:
        return None
    cuts = (np.arange(g + 1, dtype=np.int64) * n) // g
    lo = np.maximum(cuts[:-1] - halo, 0) // a * a
    hi = np.minimum(-(-(cuts[1:] + halo) // a) * a, n)
    return cuts, lo, hi


def split_oversized(shape: Sequence[int], max_slot_elems: int, halo: int, align: Sequence[int] = (1, 1, 1),
                    grid: Optional[Sequence[int]] = None) -> PartSplit:
    """Cut a block of ``shape`` whose workspace slot would reach ``max_slot_elems`` elements into the fewest parts whose
    slots stay below it (:class:`PartSplit`).  A pure function of its arguments.

    The cores are a grid of near-equal boxes that partition the block; every part's box is its core plus ``halo``
    voxels on every side (``halo`` = largest kernel radius of the ladder + 1: a LoG value needs the voxels within the
    radius, and the 3^4 NMS needs valid values one voxel around the core), clipped to the block.  With ``align`` (the
    profile's ``denoise_max_shape`` when the blocks are preprocessed tile by tile) box faces that are not faces of the
    block are moved outwards to the next multiple of ``align`` from the block's origin, so that a part's tile grid is
    the block's.  Among the grids with the fewest parts the one whose largest box is smallest is taken -- the longest
    axis is cut first, since that adds the least halo -- and of equals the one that cuts the later axes.  ``grid``
    (experiments): that ``(gz, gy, gx)`` grid and no other.
    ``MmxError`` when no such grid exists: the halo alone fills a slot."""
    shape = tuple(int(v) for v in shape)
    align = tuple(max(1, int(v)) for v in align)
    halo, limit = int(halo), int(max_slot_elems)
    if len(shape) != 3 or min(shape) < 1 or halo < 0 or len(align) != 3:
        raise ValueError("split_oversized takes a (z, y, x) extent, a halo >= 0 and a per-axis alignment")
    refuse = slot_refusal(limit)
    # the smallest box any grid can give: a core of one voxel and its halo, rounded out to the alignment
    least = [min(n, -(-(1 + 2 * halo) // a) * a) for n, a in zip(shape, align)]
    if int(_slot_elems(least)) >= limit:
        raise nat.MmxError(f"{refuse} and it cannot be cut into parts: a part's halo of {halo} voxels on every side "
                           f"(largest kernel radius + 1) alone takes {int(_slot_elems(least))} elements; detect with a "
                           "smaller segment_size")
    only = None if grid is None else tuple(int(v) for v in grid)
    if only is not None and (len(only) != 3 or min(only) < 1):
        raise ValueError("a grid of parts is (gz, gy, gx), each at least 1")
    # per axis the piece counts worth trying -- those that make the largest box (along x: its padded row) smaller than
    # every smaller count does -- and what they make it; the grids are their combinations
    counts, sizes, pieces = [], [], {}
    for ax in range(3):
        tries = range(1, min(shape[ax], MAX_PARTS) + 1) if only is None else [only[ax]]
        gs, es, least_e = [], [], None
        for g in tries:
            pc = _axis_pieces(shape[ax], g, halo, align[ax])
            if pc is None:
                continue
            e = int((pc[2] - pc[1]).max())
            e = int(_row_elems(e)) if ax == 2 else e
            if least_e is None or e < least_e:
                gs.append(g)
                es.append(e)
                pieces[(ax, g)] = pc
                least_e = e
            if e <= least[ax]:          # (it gets no smaller)
                break
        counts.append(np.asarray(gs, dtype=np.int64))
        sizes.append(np.asarray(es, dtype=np.int64))
    if all(len(c) for c in counts):
        n_parts = counts[0][:, None, None] * counts[1][None, :, None] * counts[2][None, None, :]
        worst = sizes[0][:, None, None] * sizes[1][None, :, None] * sizes[2][None, None, :]
        ok = (worst < limit) & (n_parts <= MAX_PARTS)
        if ok.any():
            # fewest parts, then the smallest largest box, then the grid that cuts the later axes (C order of the grids)
            key = np.where(ok, n_parts, np.iinfo(np.int64).max)
            cand = np.argwhere(key == key.min())
            cand = cand[np.argsort(worst[tuple(cand.T)], kind="stable")]
            iz, iy, ix = (int(v) for v in cand[0])
            grid3 = (int(counts[0][iz]), int(counts[1][iy]), int(counts[2][ix]))
            axes = [pieces[(ax, g)] for ax, g in enumerate(grid3)]
            idx = np.stack(np.meshgrid(*(np.arange(g) for g in grid3), indexing="ij"), axis=-1).reshape(-1, 3)
            cores = np.empty((len(idx), 2, 3), dtype=np.int64)
            boxes = np.empty_like(cores)
            for ax in range(3):
                cuts, lo, hi = axes[ax]
                cores[:, 0, ax], cores[:, 1, ax] = cuts[idx[:, ax]], cuts[idx[:, ax] + 1]
                boxes[:, 0, ax], boxes[:, 1, ax] = lo[idx[:, ax]], hi[idx[:, ax]]
            return PartSplit(shape, halo, grid3, tuple(a_[0] for a_ in axes), cores, boxes)
    how = f"{MAX_PARTS} parts or fewer" if only is None else f"a {only[0]} x {only[1]} x {only[2]} grid of parts"
    raise nat.MmxError(f"{refuse} and it cannot be cut into {how} with a halo of {halo} voxels; detect with a smaller "
                       "segment_size")


def _isolate_parents(batches: List[List[int]], splits: Dict[int, PartSplit]) -> List[List[int]]:
    """``batches`` with every block that is detected in parts in a batch of its own (its parts are that batch's blocks)."""
    out: List[List[int]] = []
    for b in batches:
        cur: List[int] = []
        for i in b:
            if i in splits:
                if cur:
                    out.append(cur)
                out.append([i])
                cur = []
            else:
                cur.append(i)
        if cur:
            out.append(cur)
    return out


def thin_signature(shapes, thin_below: int) -> np.ndarray:
    """Per block the set of axes it is *thin* along -- extent ``< thin_below`` -- as bits: 1 = z, 2 = y, 4 = x."""
    shp = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    return ((shp < int(thin_below)) * np.array([1, 2, 4], dtype=np.int64)).sum(axis=1)


def _fill_batches(order: Sequence[int], slots, per_vox: int, budget_bytes: int, max_batch: int) -> List[List[int]]:
    """The blocks ``order`` in batches, in that order: a batch is closed when one more block -- every block in a slot of
    the largest -- would exceed the budget or ``max_batch`` blocks."""
    batches: List[List[int]] = []
    cur: List[int] = []
    cur_slot = 0
    for i in order:
        slot = max(cur_slot, slots[i])
        if cur and ((len(cur) + 1) * slot * per_vox > budget_bytes or len(cur) >= max_batch):
            batches.append(cur)
            cur, slot = [], slots[i]
        cur.append(i)
        cur_slot = slot
    if cur:
        batches.append(cur)
    return batches


def plan_batches(shapes: Sequence[Tuple[int, int, int]], num_sigma: int, budget_bytes: int,
                 extra_bytes_per_voxel: int = 0, *, taper: int, ramp: int, max_batch: int = 1 << 30,
                 forced_sizes: Sequence[int] = (), thin_below: int = 0, thin_min_voxels: int = 64 << 20,
                 never_thin: Sequence[int] = ()) -> List[List[int]]:
    """Group block indices into batches whose workspace fits ``budget_bytes``.

    ``thin_below`` > 0: blocks with an extent below it (:func:`thin_signature`; a ragged stack's remainders, shorter
    than the kernels) leave the list -- one of them in a batch takes the whole batch off the fast kernels, whose path is
    chosen from the batch's smallest extents.  The other blocks are planned as if they did not exist, and the thin ones
    follow in batches of their own, one signature each, under the same budget rule.  Only when the regular blocks hold
    real work (more than ``thin_min_voxels`` voxels, the taper's measure) and there are blocks of both kinds; the blocks
    ``never_thin`` (detected in parts) count as regular whatever their extents.  0: no block leaves.

    Workspace = (4 + num_sigma) float32 arrays of ``n_blocks * slot`` voxels, slot = the
    largest block of the batch (+ ``extra_bytes_per_voxel`` for the preprocessed copies).
    Blocks keep their order (z-major grid order).  ``max_batch`` caps the blocks of a batch; the tail of the list is
    re-split into batches that shrink towards ``taper`` blocks and the first batch into a ramp that starts at ``ramp``
    (0: not); ``forced_sizes`` (experiments): batches of exactly these sizes when they add up to the number of blocks.
    """
    per_vox = (4 + num_sigma) * 4 + (num_sigma + 1) // 2 + extra_bytes_per_voxel     # + the NMS bit masks
    if not len(shapes):
        return []
    if forced_sizes and sum(forced_sizes) == len(shapes):       # (experiments: bench.py --batches)
        cuts = np.concatenate(([0], np.cumsum(forced_sizes)))
        return [list(range(int(a), int(b))) for a, b in zip(cuts[:-1], cuts[1:])]
    slots = _slot_elems(np.asarray(shapes).reshape(-1, 3)).tolist()
    if thin_below > 0:
        sig = thin_signature(shapes, thin_below)
        sig[np.asarray(list(never_thin), dtype=np.int64)] = 0
        regular = np.nonzero(sig == 0)[0].tolist()
        if 0 < len(regular) < len(shapes) and \
                sum(int(shapes[i][0]) * int(shapes[i][1]) * int(shapes[i][2]) for i in regular) > thin_min_voxels:
            planned = plan_batches([shapes[i] for i in regular], num_sigma, budget_bytes, extra_bytes_per_voxel, taper=taper,
                                   ramp=ramp, max_batch=max_batch)
            batches = [[regular[k] for k in b] for b in planned]
            for which in sorted(set(sig.tolist()) - {0}):
                batches += _fill_batches(np.nonzero(sig == which)[0].tolist(), slots, per_vox, budget_bytes, max_batch)
            return batches
    batches = _fill_batches(range(len(slots)), slots, per_vox, budget_bytes, max_batch)
    # The host finishes batch k (candidates -> peaks -> per-block prune -> tables: ~0.45 ms per block of the
    # benchmark volume) while the GPU runs batch k + 1 (~0.46 ms per block with the tiled kernels), so it trails the
    # GPU by the host time of one batch, and nothing hides that of the LAST batches: the tail of the block list is
    # re-split into batches that shrink geometrically towards the end (... 18 / 11 / 7 / 4 blocks) -- each still
    # gives the GPU about as much work as the host has left from the batch before.  Measured (tools/steptrace.py):
    # 89 / 89 / 59 / 19 blocks left the host 8 ms behind the GPU at the end and 18 ms of tail, 89 / 89 / 39 / 20 /
    # 10 / 5 / 4 did not; with 22-block batches a tail of 22 / 7 / 7 against 18 / 18 / 11 / 7 / 4.
    vox = [int(s_[0]) * int(s_[1]) * int(s_[2]) for s_ in shapes]

    def fits(batch):
        return len(batch) == 1 or (len(batch) * max(slots[i] for i in batch) * per_vox <= budget_bytes and len(batch) <= max_batch)

    full = max(len(b_) for b_ in batches)
    tail = batches.pop()
    while batches and len(tail) < 2 * full and max_batch >= (1 << 30):      # (a capped batch size: no re-merging)
        tail = batches.pop() + tail
    # (only where there is real work: below ~64 Mvoxel a batch is a few hundred microseconds of kernels)
    if taper > 0 and len(tail) > taper and sum(vox[i] for i in tail) > (64 << 20):
        sizes, step = [], float(taper)
        while sum(sizes) + int(step) <= len(tail) and int(step) < full:
            sizes.append(int(step))
            step *= 1.6
        rest = len(tail) - sum(sizes)
        n_front = -(-rest // full) if rest else 0
        front = [rest // n_front + (1 if j < rest % n_front else 0) for j in range(n_front)] if n_front else []
        at, pieces = 0, []
        for n in front + sizes[::-1]:
            pieces.append(tail[at:at + n])
            at += n
        tail_batches = []
        for piece in pieces:                    # (blocks of different sizes: a piece may exceed the budget its count suggests)
            while not fits(piece):
                cut = len(piece) // 2
                tail_batches.append(piece[:cut])
                piece = piece[cut:]
            tail_batches.append(piece)
        batches.extend(tail_batches)
    else:
        stack = [tail]
        while stack:                             # (the merged tail of small batches must still fit the budget)
            piece = stack.pop(0)
            if fits(piece):
                batches.append(piece)
            else:
                stack[0:0] = [piece[:len(piece) // 2], piece[len(piece) // 2:]]
    # ... and nothing hides the GPU time of the FIRST batch from the host, which has nothing to do until its
    # candidates arrive: with the tiled kernels the host work per block (~0.5 ms) is as long as the kernels'
    # (~0.55 ms), so a first batch of 89 blocks put the host 50 ms behind for the whole step (tail after the last
    # kernel 24 - 38 ms).  The first batch is therefore split into a ramp of ``ramp``, 2 x, 4 x ... blocks.
    first = batches[0]
    if ramp > 0 and len(batches) > 1 and len(first) > 2 * ramp and sum(vox[i] for i in first) > (64 << 20):
        head = []
        while len(first) > 2 * ramp:
            head.append(first[:ramp])
            first = first[ramp:]
            ramp *= 2
        batches[0:1] = head + [first]
    return batches


@dataclass
class PlannedBatch:
    """One batch of a :class:`BatchPlan`: the places ``indices`` of its blocks in the call's lists, and what the library
    will see of it -- ``n_blocks`` blocks in slots of ``slot`` elements: the parts of ``split`` when its one block is
    detected in parts, the blocks themselves otherwise.  ``records``: its host ``mmx_block`` array, or None where that
    is made when the batch is enqueued (a block in parts, a lane that preprocesses); ``d_records``: its slice of the
    plan's one uploaded table, or None.  ``zx_mode``: the ``mmx_zx_mode`` this batch asks for under ``MMX_ZX_AUTO`` --
    ``MMX_ZX_THIN`` when every one of its blocks is thin along some axis -- or None: the lane's mode."""
    indices: List[int]
    split: Optional[PartSplit]
    n_blocks: int
    slot: int
    records: Optional[np.ndarray] = None
    d_records: object = None
    zx_mode: Optional[int] = None


@dataclass
class BatchPlan:
    """The batches of one call, in the order they run, over the checked ``origins`` / ``shapes`` lists."""
    batches: List[PlannedBatch]
    origins: List[Tuple[int, int, int]]
    shapes: List[Tuple[int, int, int]]


def make_plan(origins, shapes, batches: List[List[int]], splits: Dict[int, PartSplit], strides=None,
              thin_below: int = 0) -> BatchPlan:
    """The plan of ``batches`` (block indices; a block of ``splits`` alone in its batch).  ``strides``: the element
    strides (z, y, x) of the volume the batches read raw -- they then carry their records; None: no batch does.
    ``thin_below`` > 0: a batch whose every block has an extent below it (never the parts of a block) asks for
    ``MMX_ZX_THIN``."""
    thin = thin_signature(shapes, thin_below) != 0 if thin_below > 0 and len(shapes) else None
    if strides is not None:
        src_offsets = np.asarray(origins, dtype=np.int64).reshape(-1, 3) @ np.asarray(strides, dtype=np.int64)
    planned = []
    for b in batches:
        split = splits.get(b[0]) if len(b) == 1 else None
        shp = split.box_shapes if split is not None else [shapes[i] for i in b]
        records = block_records(src_offsets[b], shp)[0] if split is None and strides is not None else None
        zx_mode = nat.MMX_ZX_THIN if thin is not None and split is None and bool(thin[b].all()) else None
        planned.append(PlannedBatch(b, split, len(shp), batch_slot(shp), records, zx_mode=zx_mode))
    return BatchPlan(planned, origins, shapes)
