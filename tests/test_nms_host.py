"""The references and inputs of tests/test_gpu_nms.py, checked on the CPU: a brute-force NumPy statement of what the
NMS kernels (``peaks_kernel``, ``peaks_sparse_kernel``: csrc/mmx_peaks.hip) and ``expand_probes_kernel``
(csrc/mmx_rescore.hip) owe their callers by include/mmx.h, the 16-byte NMS entries of both layouts as mmx.h states
them, and synthetic cubes that put a near-tie at every place where those kernels take another branch.

Exact arithmetic.  Every cube value is a multiple of 2**-16 in [-0.5, 2), the band is ``EPS`` = 2**-12 and the
thresholds are 0.125 and 0: ``v +- eps``, ``m +- eps`` and ``thr +- eps`` are then exact in float32, the kernels' early
rejections agree with their final test, and a voxel can be put exactly ON an edge of a rule.  So the GPU tests compare
for equality, bit for bit; there is no tolerance in this file or in theirs.

The cases.  A case is one batch: several blocks of different extents, one scale count, one threshold.  Per block the
cube is a random fill (a stated share of voxels above ``thr - eps``) into which "sites" are planted: a voxel ``p`` whose
3^4 neighbourhood is cleared to values far below it, with at most one rival ``q`` among the neighbours, the pair put on
one of the knife edges (``PLANTS``).  Sites lie on a lattice of spacing 3, so no site sees another's rival; where the
ladder is long enough the rival of a site at scale 7 / 8 / 15 / 16 is the same voxel one scale across the seam between
two sigma chunks of ``peaks_kernel``.  A block takes up to 16 sites at those seams, 8 at the two ends of its rows (candidates
all: the quad tail and the pitch columns beside it) and 8 more, the kinds in turn, so a block with room for eight sites
holds every edge and a 1 x 1 x 1 block holds what fits; rows of more than 64 quads also hold lone candidates in the last
column of lane 63 and the first of lane 0 of a wave, with a larger value elsewhere in their quad.  The tests at the end
of this file prove from the reference alone that every
planted voxel has the status its kind states and that every case holds what the GPU test of it relies on (candidate
counts, stored and unstored segments, more than 1024 candidate bits in one workgroup round of the sparse kernel),
so that no GPU test can pass vacuously."""
import functools

import numpy as np
import pytest

EPS = 2.0 ** -12                        # the nomination band of every case (the product's 16-bit band is 2.5e-4)
Q = 2.0 ** -16                          # the grid every cube value lies on
ROWS, QUADS = 1, 2                      # MMX_MASK_ROWS, MMX_MASK_QUADS
CONTESTED, BAND, PROBE = 1, 2, 4        # MMX_CAND_*
#: the 80 neighbours in the order of the band bits: C order of (ds, dz, dy, dx) over {-1, 0, 1}^4, the centre left out
OFFSETS = np.array([(ds, dz, dy, dx) for ds in (-1, 0, 1) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                    if (ds, dz, dy, dx) != (0, 0, 0, 0)], dtype=np.int64)
QUEUE = 1024                            # set bits one workgroup round of peaks_sparse_kernel can queue (kQ)
ROUND_WORDS = 2048                      # entry words of one workgroup round (MMX_WG 256 lanes x kW 8 words)
MAX_DELTA = 3 * Q                       # the largest |exact - nominated| of the closed loop: below EPS / 4


# ---------------------------------------------------------------------------------------------------- the references
def _views(padded, shape):
    ns, nz, ny, nx = shape
    for o in OFFSETS:
        yield padded[1 + o[0]:1 + o[0] + ns, 1 + o[1]:1 + o[1] + nz, 1 + o[2]:1 + o[2] + ny, 1 + o[3]:1 + o[3] + nx]


def face_kind(shape):
    """Per voxel of a ``[ns, nz, ny, nx]`` cube the set of axes on whose first or last index it lies, as bits
    (1: sigma, 2: z, 4: y, 8: x): 0 inside, 15 at the 4-D corners -- the 16 kinds of place a voxel can have."""
    kind = np.zeros(shape, dtype=np.int64)
    for ax, n in enumerate(shape):
        on = np.zeros(n, dtype=np.int64)
        on[0] = on[-1] = 1 << ax
        kind |= on.reshape([-1 if a == ax else 1 for a in range(4)])
    return kind


def nominate_ref(cube, stored, thr, eps):
    """What ``mmx_peaks_batch`` owes for one block: ``cube`` [ns, nz, ny, nx] float32, ``stored`` which voxels exist
    (all of them for the dense kernel; the others count as -inf).  M = the largest of the in-cube neighbours, and 0 when
    the voxel lies on any of the 8 faces of the cube (zero padding, the two ends of the ladder included).  A candidate
    has ``v > thr - eps`` and ``v >= M - eps``.  Returned in (s, z, y, x) order: the coordinates, ``v``, ``nbr_max``,
    ``contested`` and the 80-bit band (``band``: neighbours 0..63, ``band_hi``: 64..79), all computed in float32."""
    cube = np.asarray(cube, dtype=np.float32)
    stored = np.broadcast_to(np.asarray(stored, dtype=bool), cube.shape)
    shape = cube.shape
    thr, eps, ninf = np.float32(thr), np.float32(eps), np.float32(-np.inf)
    eff = np.where(stored, cube, ninf)
    padded = np.full(tuple(n + 2 for n in shape), ninf, dtype=np.float32)
    padded[1:-1, 1:-1, 1:-1, 1:-1] = eff
    m = np.full(shape, ninf, dtype=np.float32)
    for u in _views(padded, shape):
        m = np.maximum(m, u)
    m = np.where(face_kind(shape) != 0, np.maximum(m, np.float32(0)), m).astype(np.float32)
    mask = stored & (eff > thr - eps) & (eff >= m - eps)
    idx = np.nonzero(mask)
    v, mm = eff[idx], m[idx]
    band, band_hi = np.zeros(len(v), dtype=np.uint64), np.zeros(len(v), dtype=np.uint32)
    for j, u in enumerate(_views(padded, shape)):
        inb = u[idx] >= v - eps                                       # (an unstored or outside neighbour is -inf: never)
        if j < 64:
            band |= inb.astype(np.uint64) << np.uint64(j)
        else:
            band_hi |= inb.astype(np.uint32) << np.uint32(j - 64)
    return dict(s=idx[0].astype(np.int32), z=idx[1].astype(np.int32), y=idx[2].astype(np.int32), x=idx[3].astype(np.int32),
                v=v, nbr_max=mm, contested=~(v > mm + eps) | ~(v > thr + eps), band=band, band_hi=band_hi, mask=mask)


def probes_ref(cands, shapes, ns):
    """Every neighbour ``mmx_expand_probes`` must append for a candidate table (fields slot, s, z, y, x, flags, band):
    of a contested candidate its in-cube neighbours -- with MMX_CAND_BAND only those in its band --, of any other none.
    Rows ``(slot, s, z, y, x, index of the candidate)``, sorted."""
    dims = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)[cands["slot"]]
    flags = cands["flags"].astype(np.int64)
    contested, banded = (flags & CONTESTED) != 0, (flags & BAND) != 0
    rows = []
    for j, o in enumerate(OFFSETS):
        ss, zz, yy, xx = (cands[f].astype(np.int64) + d for f, d in zip("szyx", o))
        inside = ((ss >= 0) & (ss < ns) & (zz >= 0) & (zz < dims[:, 0]) & (yy >= 0) & (yy < dims[:, 1]) & (xx >= 0) &
                  (xx < dims[:, 2]))
        inb = (cands["band"] >> np.uint64(j)) & np.uint64(1) if j < 64 else (flags >> (16 + j - 64)) & 1
        take = contested & inside & (~banded | (inb != 0))
        rows.append(np.stack([cands["slot"].astype(np.int64), ss, zz, yy, xx, np.arange(len(cands))], axis=1)[take])
    rows = np.concatenate(rows) if rows else np.zeros((0, 6), dtype=np.int64)
    return sort_rows(rows)


def sort_rows(rows):
    rows = np.asarray(rows)
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows


# ---------------------------------------------------------------------------------------------------- the entries
def pitch(nx):
    return -(-nx // 32) * 32


def entry_map(nz, nx, layout):
    """Where include/mmx.h puts voxel (z, x) of a row y: ``(entry within the row [nz, nx], bit [nz, nx], entries per
    row)``.  MMX_MASK_ROWS: entry c >> 6, bit c & 63 of c = z px + x, ceil(nz px / 64) entries; MMX_MASK_QUADS: entry
    (z >> 2) ceil(nx / 16) + (x >> 4), bit ((z & 3) << 4) | (x & 15), ceil(nz / 4) ceil(nx / 16) entries."""
    z, x = np.meshgrid(np.arange(nz), np.arange(nx), indexing="ij")
    if layout == ROWS:
        c = z * pitch(nx) + x
        return c >> 6, c & 63, (nz * pitch(nx) + 63) >> 6
    ntx = (nx + 15) >> 4
    return (z >> 2) * ntx + (x >> 4), ((z & 3) << 4) | (x & 15), ((nz + 3) >> 2) * ntx


def entry_voxels(nz, nx, layout, w, b):
    """The inverse, as the kernels decode it: voxel (z, x) of bit ``b`` of entry ``w`` of a row (possibly outside the
    block: a pitch column, a plane past the last)."""
    if layout == ROWS:
        col = (w << 6) + b
        return col // pitch(nx), col % pitch(nx)
    ntx = (nx + 15) >> 4
    return 4 * (w // ntx) + (b >> 4), 16 * (w % ntx) + (b & 15)


def words_of(bits, layout):
    """``bits`` [ns, nz, ny, nx] bool -> the words [ns, ny, entries per row] uint64 that hold them."""
    ns, nz, ny, nx = bits.shape
    ent, bit, nwords = entry_map(nz, nx, layout)
    words = np.zeros((ns, ny, nwords), dtype=np.uint64)
    vals = np.moveaxis(bits, 1, 2).reshape(ns, ny, nz * nx).astype(np.uint64) << bit.ravel().astype(np.uint64)
    np.add.at(words, (slice(None), slice(None), ent.ravel()), vals)       # (distinct bits: the sum is the union)
    return words


def bits_of(words, nz, nx, layout):
    """The inverse of ``words_of`` for in-block voxels: [ns, ny, entries per row] -> [ns, nz, ny, nx] bool."""
    ent, bit, _ = entry_map(nz, nx, layout)
    got = (words[:, :, ent.ravel()] >> bit.ravel().astype(np.uint64)) & np.uint64(1)
    return np.moveaxis(got.reshape(words.shape[0], words.shape[1], nz, nx), 2, 1).astype(bool)


def stored_of(words1, nz, nx, layout):
    """Which in-block voxels lie in a segment whose word 1 is not zero (the others are not written to ``d_log``)."""
    ent, _, _ = entry_map(nz, nx, layout)
    got = words1[:, :, ent.ravel()] != 0
    return np.moveaxis(got.reshape(words1.shape[0], words1.shape[1], nz, nx), 2, 1)


def entries_from(cube, thr, eps, layout, word0):
    """The entries of one block as mmx.h states them, ``[ns, ny, entries per row, 2]`` uint64, and the ``stored`` mask.
    Word 1: ``v > thr - eps``.  Word 0: ``"same"`` = word 1, the largest legal superset; ``"faces"`` = word 1 and no
    y / x face neighbour exceeds the voxel by more than eps, the smallest set the text allows."""
    cube = np.asarray(cube, dtype=np.float32)
    thr, eps = np.float32(thr), np.float32(eps)
    above = cube > thr - eps
    cand = above
    if word0 == "faces":
        padded = np.pad(cube, ((0, 0), (0, 0), (1, 1), (1, 1)), constant_values=-np.inf)
        rival = np.maximum(np.maximum(padded[:, :, :-2, 1:-1], padded[:, :, 2:, 1:-1]),
                           np.maximum(padded[:, :, 1:-1, :-2], padded[:, :, 1:-1, 2:]))
        cand = above & ~(rival > cube + eps)
    else:
        assert word0 == "same"
    w1 = words_of(above, layout)
    return np.stack([words_of(cand, layout), w1], axis=-1), stored_of(w1, cube.shape[1], cube.shape[3], layout)


def round_bits(entries):
    """Set bits of word 0 per workgroup round of ``peaks_sparse_kernel``: the words in the order the kernel indexes them
    (scale, row, entry), 2048 at a time."""
    w0 = np.ascontiguousarray(entries[..., 0]).ravel()
    pop = np.unpackbits(w0.view(np.uint8)).reshape(len(w0), 64).sum(axis=1)
    pad = -len(pop) % ROUND_WORDS
    return np.concatenate([pop, np.zeros(pad, dtype=pop.dtype)]).reshape(-1, ROUND_WORDS).sum(axis=1), pop


# ---------------------------------------------------------------------------------------------------- the workspace
def poison(n):
    """NaN and 1e30 in turn: what every float of a workspace holds that is nobody's (pitch columns, slot tails,
    unstored segments).  Either would out-vote any real value or make every comparison false."""
    out = np.full(n, np.nan, dtype=np.float32)
    i = np.arange(n)
    out[((i + i // 7) & 1) == 1] = 1e30                 # (in turn, the turn shifted every 7: either kind in every column)
    return out


def pack_log(cubes, slot_elems, stored=None):
    """``d_log`` of a batch, [ns][n blocks][slot_elems] float32 as one array: poison everywhere, then the voxels of
    block i in slot i, rows ``pitch(nx)`` apart -- only the stored ones where ``stored`` (per block) is given."""
    ns, nb = cubes[0].shape[0], len(cubes)
    log = poison(ns * nb * slot_elems).reshape(ns, nb, slot_elems)
    for i, cube in enumerate(cubes):
        _, nz, ny, nx = cube.shape
        px = pitch(nx)
        assert nz * ny * px <= slot_elems
        rows = log[:, i, :nz * ny * px].reshape(ns, nz, ny, px)
        if px > nx:                     # the pitch column beside the last voxel of a row: 1e30 in three rows of four
            beside = np.add.outer(np.arange(ns), np.arange(nz * ny)).reshape(ns, nz, ny) % 4
            rows[..., nx] = np.where(beside != 0, np.float32(1e30), np.float32(np.nan))
        view = rows[..., :nx]
        keep = np.ones(cube.shape, dtype=bool) if stored is None else stored[i]
        view[keep] = cube[keep]
    return log


def pack_entries(entries, slot_elems):
    """``d_nms_mask`` of a batch, [ns][(n blocks slot_elems) >> 5][2] uint64: block i's entries from entry
    (i slot_elems) >> 5 of every scale on, all bits set in the entries that are nobody's."""
    ns, nb = entries[0].shape[0], len(entries)
    out = np.full((ns, (nb * slot_elems) >> 5, 2), ~np.uint64(0), dtype=np.uint64)
    for i, e in enumerate(entries):
        n = e.shape[1] * e.shape[2]
        assert n <= (slot_elems >> 5) - 1, "the library's fit rule (mmx_batch_geom_make)"
        out[:, (i * slot_elems) >> 5:][:, :n] = e.reshape(ns, n, 2)
    return out


# ---------------------------------------------------------------------------------------------------- the cases
#: kind -> (value of the rival q or None, value of the site p, is p a candidate, is it contested); `T` stands for thr
PLANTS = {
    "edge_in": (1.0, 1.0 - EPS, True, True),                  # v == M - eps
    "edge_out": (1.0, 1.0 - EPS - Q, False, None),            # v == M - eps - 2^-16
    "thr_out": (None, "T-e", False, None),                    # v == thr - eps
    "thr_in": (None, "T-e+q", True, True),                    # v == thr - eps + 2^-16
    "edge_contested": (0.75, 0.75 + EPS, True, True),         # v == M + eps
    "clear_win": (0.75, 0.75 + EPS + Q, True, False),         # v == M + eps + 2^-16
    "plateau2": (1.5, 1.5, True, True),                       # a two-voxel plateau
    "beaten": (1.5, 1.0, False, None),                        # only the rival beats it
    "neg_border": (None, -4 * Q, None, True),                 # thr = 0 cases: a border voxel just below zero
}
_CYCLE = ("edge_in", "edge_out", "plateau2", "beaten", "clear_win", "edge_contested", "thr_out", "thr_in")
SEAM_SCALES = (7, 8, 15, 16)            # either side of the seams between the sigma chunks of peaks_kernel (kSigmaChunk 8)

_DENSE_SHAPES = [(3, 4, 1), (4, 3, 2), (3, 5, 3), (5, 4, 4), (4, 6, 5), (6, 3, 31), (3, 4, 32), (5, 5, 33), (4, 3, 63),
                 (3, 6, 64), (6, 5, 65), (4, 4, 257), (1, 5, 9), (5, 1, 33), (1, 1, 1), (5, 6, 7)]
_SPARSE_SHAPES = [(3, 4, 1), (1, 5, 15), (4, 3, 16), (5, 6, 17), (9, 5, 33), (3, 5, 65), (5, 1, 33), (6, 6, 64), (4, 4, 33),
                  (3, 4, 80)]
#: name -> dict(ns, thr, density: share of voxels above thr - eps, shapes, sparse: the cube has regions below thr - eps)
CASES = {
    "dense_ns1": dict(ns=1, thr=0.125, density=0.4, shapes=_DENSE_SHAPES),
    "dense_ns2": dict(ns=2, thr=0.125, density=0.01, shapes=_DENSE_SHAPES),
    "dense_ns3_thr0": dict(ns=3, thr=0.0, density=0.3, shapes=_DENSE_SHAPES),
    "dense_ns8": dict(ns=8, thr=0.125, density=0.5, shapes=_DENSE_SHAPES),
    "dense_ns9": dict(ns=9, thr=0.125, density=0.3, shapes=_DENSE_SHAPES),
    "dense_ns16": dict(ns=16, thr=0.125, density=0.01, shapes=_DENSE_SHAPES),
    "dense_ns17": dict(ns=17, thr=0.125, density=0.6, shapes=_DENSE_SHAPES),
    "sparse_ns1": dict(ns=1, thr=0.125, density=0.4, shapes=_SPARSE_SHAPES, sparse=True),
    "sparse_ns2_thr0": dict(ns=2, thr=0.0, density=0.3, shapes=_SPARSE_SHAPES, sparse=True),
    "sparse_ns9": dict(ns=9, thr=0.125, density=0.4, shapes=_SPARSE_SHAPES, sparse=True),
    # the last block holds a plateau of more than 1024 voxels in rows of differing length: the LDS queue overflows
    "sparse_queue": dict(ns=2, thr=0.125, density=0.4, shapes=[(5, 6, 17), (4, 4, 33), (6, 6, 64)], sparse=True, queue=True),
}
DENSE = sorted(n for n, c in CASES.items() if not c.get("sparse"))
SPARSE = sorted(n for n, c in CASES.items() if c.get("sparse"))
PLATEAU_SHAPE = (5, 6, 7)               # dense cases: this block holds the 3 x 3 x 3 x 2 plateau
SIGMA_ONLY_SHAPE = (4, 4, 33)           # sparse cases: one scale of this block stored throughout, its neighbours not at all
#: sparse cases: this block holds nothing but four voxels per scale, each the last or first of its entry in x (columns
#: 63 | 64 of plane 0: a seam of both layouts; 15 | 16 of plane 2: of the quads) with nothing stored across that seam
SEAM_SHAPE = (3, 4, 80)
SEAM_VOXELS = ((0, 0, 63), (0, 1, 64), (2, 2, 15), (2, 3, 16))


def _grid(rng, shape, lo, hi):
    return (rng.integers(int(round(lo / Q)), int(round(hi / Q)), size=shape) * Q).astype(np.float32)


def _lattice(n, phase):
    return list(range(phase, n, 3)) if phase < n else [0]


def _lattice_x(n, phase):
    """Along a row: its two ends always, the lattice of this phase between them."""
    out = [0]
    for c in list(range(phase, n - 3, 3)) + [n - 1]:
        if c >= out[-1] + 3:
            out.append(c)
    return out


def _nbhd(shape, p, reach=1):
    return tuple(slice(max(0, c - reach), min(n, c + reach + 1)) for c, n in zip(p, shape))


class Case:
    """One batch: ``cubes[i]`` [ns, nz, ny, nx] float32 per block (the true values everywhere), ``plants``: the sites
    as ``(block, kind, p, q or None)``, ``plateaus``: ``(block, box of slices)``."""

    def __init__(self, name):
        spec = CASES[name]
        self.name, self.ns, self.thr, self.shapes = name, spec["ns"], spec["thr"], list(spec["shapes"])
        self.sparse, self.queue = bool(spec.get("sparse")), bool(spec.get("queue"))
        self.eps = EPS
        self.slot_elems = max(s[0] * s[1] * pitch(s[2]) for s in self.shapes) + 96     # (larger than the largest block)
        rng = np.random.default_rng(sorted(CASES).index(name) + 1000)
        self.cubes, self.plants, self.plateaus, self.wave_plants = [], [], [], []
        for i, shp in enumerate(self.shapes):
            self.cubes.append(self._block(rng, i, (self.ns,) + tuple(shp), spec["density"]))
        self._ref, self._entries = {}, {}

    # -- one block
    def _block(self, rng, i, shape, density):
        ns, thr = self.ns, self.thr
        low = lambda shp: _grid(rng, shp, -0.5, thr - 0.02)                            # noqa: E731  (far below thr - eps)
        cube = low(shape)
        if self.sparse and shape[1:] == SEAM_SHAPE:
            for z, y, x in SEAM_VOXELS:
                cube[:, z, y, x] = 1.0
            return cube
        pick = rng.random(shape) < density
        if self.sparse:
            pick &= self._active(rng, shape)
        cube[pick] = _grid(rng, shape, thr, 2.0)[pick]
        taken = np.zeros(shape, dtype=bool)                                            # voxels a plant owns
        # a plateau: equal values, everything around them cleared, so that every voxel of it is a contested candidate
        box = None
        if self.queue and i == len(self.shapes) - 1:
            on = np.zeros(shape, dtype=bool)
            for z in range(1, 5):
                for y in range(1, 5):
                    on[:, z, y, y:60 - 3 * z] = True                                    # (rows of differing length)
            box = (slice(0, ns), slice(1, 5), slice(1, 5), slice(1, 57))
        elif not self.sparse and shape[1:] == PLATEAU_SHAPE:
            on = np.zeros(shape, dtype=bool)
            box = (slice(max(0, ns - 2), ns), slice(0, 3), slice(1, 4), slice(2, 5))
            on[box] = True
        if box is not None:
            around = tuple(slice(max(0, b.start - 1), min(n, b.stop + 1)) for b, n in zip(box, shape))
            cube[around] = low(cube[around].shape)
            cube[on] = 1.75
            taken[tuple(slice(max(0, b.start - 2), min(n, b.stop + 2)) for b, n in zip(box, shape))] = True
            self.plateaus.append((i, on))
        # the ends of a wave of peaks_kernel (a lane holds 4 columns, lane = quad index mod 64; rows of more than 64 quads
        # only): a lone voxel in the last column of lane 63 / the first of lane 0 with a larger value three columns
        # away in the same quad -- no neighbour of it, but what a shuffle past the end of the wave hands back
        qrow = pitch(shape[3]) // 4
        for row in range(shape[1] * shape[2] if not self.sparse and qrow > 64 else 0):
            z, y = divmod(row, shape[2])
            for lane, kind in (((63, "wave_right"),) if row % 2 else ((0, "wave_left"),)):      # (they would be side by side)
                x0 = 4 * ((lane - row * qrow) % 64)
                p, far = (row % ns, z, y, x0 + 3), (row % ns, z, y, x0)
                if lane == 0:
                    p, far = far, p
                if x0 == 0 or x0 + 4 >= shape[3] or taken[_nbhd(shape, p, 2)].any():
                    continue
                cube[_nbhd(shape, p)] = low(cube[_nbhd(shape, p)].shape)
                cube[p], cube[far] = 1.0, 1.9
                taken[_nbhd(shape, p, 2)] = taken[_nbhd(shape, far)] = True
                self.wave_plants.append((i, kind, p, far))
        # the sites: a lattice of spacing 3 whose phase differs from block to block; those at the sigma seams first
        # (in the block of the sparse cases whose one scale is stored alone, sites and rivals stay on that scale)
        alone = ns // 2 if self.sparse and not self.queue and shape[1:] == SIGMA_ONLY_SHAPE and ns >= 3 else None
        sites = [(s, z, y, x) for s in ([alone] if alone is not None else _lattice(ns, i % 3))
                 for z in _lattice(shape[1], i % 2) for y in _lattice(shape[2], (i // 2) % 2)
                 for x in _lattice_x(shape[3], i % 3)]
        sites = [p for p in sites if not taken[_nbhd(shape, p)].any()]
        order = rng.permutation(len(sites))
        seam = [sites[k] for k in order if sites[k][0] in SEAM_SCALES and 0 < sites[k][0] < ns - (sites[k][0] in (7, 15))]
        ends = [sites[k] for k in order if sites[k] not in seam and sites[k][3] in (0, shape[3] - 1)]
        rest = [sites[k] for k in order if sites[k] not in seam and sites[k] not in ends]
        chosen = seam[:16] + ends[:8] + rest[:8]
        for p in chosen:
            cube[_nbhd(shape, p)] = low(cube[_nbhd(shape, p)].shape)
        for n, p in enumerate(chosen):
            kind = _CYCLE[(n + i) % len(_CYCLE)]
            if p in ends[:8]:                                                          # the ends of a row: candidates all
                kind = ("edge_in", "clear_win", "plateau2", "edge_contested")[(n + i) % 4]
            if thr == 0.0 and n % 5 == 4 and face_kind(shape)[p]:
                kind = "neg_border"
            qv, pv, _, _ = PLANTS[kind]
            q = None
            if qv is not None:
                if p in seam:                                                          # the rival across the chunk seam
                    d = (1 if p[0] in (7, 15) else -1, 0, 0, 0)
                else:
                    inside = [o for o in OFFSETS if all(0 <= c + e < m for c, e, m in zip(p, o, shape))
                              and (alone is None or o[0] == 0)]
                    if not inside:
                        continue                                                       # (a 1 x 1 x 1 x 1 cube)
                    d = tuple(inside[(7 * n + i) % len(inside)])
                q = tuple(c + e for c, e in zip(p, d))
                cube[q] = qv
            cube[p] = {"T-e": thr - EPS, "T-e+q": thr - EPS + Q}.get(pv, pv)
            self.plants.append((i, kind, p, q))
        return cube

    def _active(self, rng, shape):
        """Sparse cases: where the cube may hold values above thr - eps -- a few random 4-D boxes; in the 4 x 4 x 33
        block one whole scale and nothing of the scales beside it."""
        ns = shape[0]
        active = np.zeros(shape, dtype=bool)
        for _ in range(4):
            lo = [int(rng.integers(0, n)) for n in shape]
            box = tuple(slice(a, a + 1 + int(rng.integers(0, max(1, n - a)))) for a, n in zip(lo, shape))
            active[box] = True
        if shape[1:] == SIGMA_ONLY_SHAPE and not self.queue:
            mid = ns // 2
            active[max(0, mid - 1):mid + 2] = False
            active[mid] = True
        return active

    # -- what the tests share
    def entries(self, layout, word0):
        """Per block ``(entries, stored)`` of ``entries_from`` (once per layout and word-0 choice)."""
        key = (layout, word0)
        if key not in self._entries:
            self._entries[key] = [entries_from(c, self.thr, self.eps, layout, word0) for c in self.cubes]
        return self._entries[key]

    def stored(self, layout):
        return None if layout is None else [st for _, st in self.entries(layout, "same")]

    def reference(self, layout=None):
        """``nominate_ref`` per block: on the whole cube (``layout`` None, the dense kernel) or on the cube a layout's
        entries store."""
        if layout not in self._ref:
            st = self.stored(layout)
            self._ref[layout] = [nominate_ref(c, True if st is None else st[i], self.thr, self.eps)
                                 for i, c in enumerate(self.cubes)]
        return self._ref[layout]

    def table(self, layout=None):
        """The reference's candidate table of the batch, sorted by (slot, s, z, y, x): a record array with the fields of
        ``mmx_cand`` that the kernels owe (``v64`` and the order of the rows are nobody's)."""
        refs = self.reference(layout)
        n = sum(len(r["v"]) for r in refs)
        t = np.zeros(n, dtype=[("slot", "<i4"), ("s", "<i4"), ("z", "<i4"), ("y", "<i4"), ("x", "<i4"), ("flags", "<u4"),
                               ("v", "<f4"), ("nbr_max", "<f4"), ("band", "<u8")])
        at = 0
        for i, r in enumerate(refs):
            m = len(r["v"])
            row = t[at:at + m]
            row["slot"] = i
            for f in ("s", "z", "y", "x", "v", "nbr_max"):
                row[f] = r[f]
            row["flags"] = r["contested"].astype(np.uint32) * CONTESTED
            if layout is not None:
                row["flags"] |= np.uint32(BAND) | (r["band_hi"] << np.uint32(16))
                row["band"] = r["band"]
            at += m
        return t

    def delta(self, pattern):
        """The closed loop's deviation per block, multiples of 2^-16 up to 3 x 2^-16 in either direction (float64):
        ``pattern`` 0 is none, 1 a hash of the coordinates, -1 its negative -- equal nominated values one apart in any
        direction differ in the exact cube, one way under 1 and the other under -1."""
        out = []
        for c in self.cubes:
            s, z, y, x = np.indices(c.shape)
            out.append(pattern * Q * (((3 * s + 5 * z + 2 * y + x) % 7) - 3.0))
        return out

    def exact(self, pattern):
        return [c.astype(np.float64) + d for c, d in zip(self.cubes, self.delta(pattern))]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def oracle_peaks(exact_cube, thr):
    """``peak_local_max`` as the oracle states it, on one block's exact [ns, nz, ny, nx] cube: the (z, y, x, scale) rows
    by descending value -- ``np.argsort(-values)`` of the ``np.nonzero`` rows, the reference's own call -- and values."""
    from oracle import blob_log_oracle as blo
    cube = np.ascontiguousarray(np.moveaxis(exact_cube, 0, -1))
    rows = np.transpose(np.nonzero(blo.peak_mask(cube, thr)))
    vals = cube[tuple(rows.T)]
    rank = np.argsort(-vals)
    return rows[rank].astype(np.int64).reshape(-1, 4), vals[rank]


# ---------------------------------------------------------------------------------------------------- real producers
#: the volume whose LoG the real producers of NMS entries run on (tests/test_gpu_nms.py, part 5): uint16, three scales of
#: kernel radius 4, 6 and 8, the threshold of the wide-row tests.  The ragged blocks: 13 rows (below 16), 21 and 30 (no
#: multiple of 16), 13 / 10 / 14 planes (no multiple of 4), 37 / 50 / 77 columns (no multiple of 16); the wide block, for
#: the tiled producers alone: 530 columns (the panel seam of their voxel copy at 512) and 26 planes.
PRODUCER_SHAPE, PRODUCER_SEED = (30, 44, 600), 23
PRODUCER_SIGMAS, PRODUCER_RADII, PRODUCER_THR = (1.0, 1.5, 2.0), (4, 6, 8), 0.05
RAGGED_BLOCKS = [((0, 0, 0), (13, 13, 37)), ((3, 5, 40), (10, 21, 50)), ((7, 2, 95), (14, 30, 77))]
WIDE_BLOCK = ((2, 9, 33), (26, 21, 530))
PRODUCER_MIN = dict(stored=20, unstored=20, candidates=10)            # per block, or the case is too easy


@functools.lru_cache(maxsize=None)
def producer_volume():
    """``synth.make_volume`` with blobs of sigma 1.2 at stated centres: a crowd inside every ragged block, a looser one
    along the wide block, so that every block has segments with and without a response above the threshold."""
    from magellanmapper_amd import synth
    rng = np.random.default_rng(PRODUCER_SEED)
    centres = []
    for (o, shp), n in zip(RAGGED_BLOCKS + [WIDE_BLOCK], (26, 24, 40, 90)):
        centres.append(rng.uniform(np.array(o) + 1.0, np.array(o) + np.array(shp) - 2.0, (n, 3)))
    return synth.make_volume(PRODUCER_SEED, PRODUCER_SHAPE, blob_sigma=1.2, centres=np.concatenate(centres))


def block_stats(cube, layout, thr, eps):
    """Stored and unstored segments and reference candidates of one block's [ns, nz, ny, nx] cube under a layout."""
    ent, stored = entries_from(cube, thr, eps, layout, "faces")
    seg = ent[..., 1] != 0
    return int(seg.sum()), int((~seg).sum()), len(nominate_ref(cube, stored, thr, eps)["v"])


# ---------------------------------------------------------------------------------------------------- CPU tests
def _plateau_cube(rng, shape):
    cube = _grid(rng, shape, -0.5, 2.0)
    cube[1:3, 0:2, 1:4, 2:4] = 1.9375
    cube[0, :, 0, :] = 1.0
    cube[-1, -1, -1, -1] = cube[-1, -1, -1, -2] = 1.96875
    return cube


@pytest.mark.parametrize("thr", [0.0, 0.125, 1.0])
def test_reference_with_no_band_is_the_oracles_peak_mask(thr):
    """``eps = 0`` and ``thr >= 0``: the candidates are exactly ``oracle.blob_log_oracle.peak_mask`` -- random cubes,
    plateaus inside and along faces and corners, extents of 1, few values (ties everywhere)."""
    from oracle import blob_log_oracle as blo
    rng = np.random.default_rng(7)
    cubes = [_grid(rng, shp, -0.5, 2.0) for shp in [(3, 4, 5, 6), (1, 3, 4, 5), (2, 1, 1, 7), (9, 2, 3, 1), (1, 1, 1, 1)]]
    cubes += [_plateau_cube(rng, (4, 3, 5, 6)), (rng.integers(0, 3, size=(3, 4, 4, 5)) * 0.5).astype(np.float32)]
    seen = 0
    for cube in cubes:
        assert cube.size == 1 or cube.min() != cube.max()
        want = np.moveaxis(blo.peak_mask(np.moveaxis(cube, 0, -1), thr), -1, 0)
        got = nominate_ref(cube, True, thr, 0.0)
        np.testing.assert_array_equal(got["mask"], want)
        np.testing.assert_array_equal(got["contested"], (got["v"] <= got["nbr_max"]) | (got["v"] <= thr))
        seen += int(want.sum())
    assert seen > 20


def test_band_bits_decode_to_the_80_offsets():
    """Bit j of the band is neighbour (ds, dz, dy, dx) in C order with the centre left out: a cube whose one neighbour
    in the band is at offset j sets exactly bit j; the kernel's own index arithmetic decodes to the same offsets."""
    assert len(OFFSETS) == 80 and len({tuple(o) for o in OFFSETS}) == 80
    for j, o in enumerate(OFFSETS):
        lin = ((o[0] + 1) * 3 + (o[1] + 1)) * 3 * 3 + (o[2] + 1) * 3 + (o[3] + 1)
        assert lin != 40 and j == lin - (lin > 40)
        cube = np.full((3, 3, 3, 3), -0.25, dtype=np.float32)
        cube[1, 1, 1, 1] = 1.0
        cube[tuple(1 + o)] = 1.0 - EPS
        r = nominate_ref(cube, True, 0.125, EPS)
        k = int(np.nonzero((r["s"] == 1) & (r["z"] == 1) & (r["y"] == 1) & (r["x"] == 1))[0][0])
        bits = int(r["band"][k]) | (int(r["band_hi"][k]) << 64)
        assert bits == 1 << j and r["contested"][k] and r["nbr_max"][k] == np.float32(1.0 - EPS)
        # ... and the probe of that candidate is that neighbour
        t = np.zeros(1, dtype=[("slot", "<i4"), ("s", "<i4"), ("z", "<i4"), ("y", "<i4"), ("x", "<i4"), ("flags", "<u4"),
                               ("band", "<u8")])
        t["s"] = t["z"] = t["y"] = t["x"] = 1
        t["flags"] = CONTESTED | BAND | ((bits >> 64) << 16)
        t["band"] = bits & (2 ** 64 - 1)
        np.testing.assert_array_equal(probes_ref(t, [(3, 3, 3)], 3), [[0, *(1 + o), 0]])
    t["flags"] = CONTESTED
    assert len(probes_ref(t, [(3, 3, 3)], 3)) == 80 and len(probes_ref(t, [(3, 3, 3)], 2)) == 53
    t["flags"] = BAND
    t["band"] = 2 ** 64 - 1
    assert len(probes_ref(t, [(3, 3, 3)], 3)) == 0


@pytest.mark.parametrize("layout", [ROWS, QUADS])
def test_entry_layouts_round_trip(layout):
    """Every voxel of a row maps to one (entry, bit), no two voxels share one, the kernels' decoding inverts it, and
    ``bits_of(words_of(.))`` is the identity -- at widths and depths on either side of every entry boundary."""
    rng = np.random.default_rng(3)
    for nz in (1, 3, 4, 5, 9):
        for nx in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257):
            ent, bit, nwords = entry_map(nz, nx, layout)
            assert ent.min() == 0 and ent.max() == nwords - 1 and bit.min() >= 0 and bit.max() < 64
            assert len(np.unique(ent * 64 + bit)) == nz * nx
            z, x = entry_voxels(nz, nx, layout, ent, bit)
            zz, xx = np.meshgrid(np.arange(nz), np.arange(nx), indexing="ij")
            np.testing.assert_array_equal(z, zz)
            np.testing.assert_array_equal(x, xx)
            bits = rng.random((2, nz, 3, nx)) < 0.5
            words = words_of(bits, layout)
            assert words.shape == (2, 3, nwords)
            np.testing.assert_array_equal(bits_of(words, nz, nx, layout), bits)
            assert int(np.unpackbits(words.view(np.uint8)).sum()) == int(bits.sum())      # (nothing beyond nx / nz)


def test_entries_say_what_the_header_says():
    """Word 1 is ``v > thr - eps`` to the bit (a voxel AT thr - eps is out), both word-0 choices lie between the
    candidates and word 1, and a segment is stored exactly when one of its voxels is above."""
    c = case("sparse_ns2_thr0")
    for layout in (ROWS, QUADS):
        refs = c.reference(layout)
        for i, cube in enumerate(c.cubes):
            same, stored = c.entries(layout, "same")[i]
            faces, stored2 = c.entries(layout, "faces")[i]
            nz, nx = cube.shape[1], cube.shape[3]
            above = cube > np.float32(c.thr) - np.float32(EPS)
            np.testing.assert_array_equal(bits_of(same[..., 1], nz, nx, layout), above)
            np.testing.assert_array_equal(same[..., 1], faces[..., 1])
            np.testing.assert_array_equal(stored, stored2)
            assert not (above & ~stored).any()
            w0 = bits_of(faces[..., 0], nz, nx, layout)
            assert not (w0 & ~above).any() and not (refs[i]["mask"] & ~w0).any()
    assert any(kind == "thr_out" for _, kind, _, _ in c.plants)


def test_workspace_packing():
    c = case("sparse_ns1")
    stored = c.stored(ROWS)
    log = pack_log(c.cubes, c.slot_elems, stored)
    assert log.shape == (1, len(c.cubes), c.slot_elems)
    for i, cube in enumerate(c.cubes):
        _, nz, ny, nx = cube.shape
        rows = log[:, i, :nz * ny * pitch(nx)].reshape(1, nz, ny, pitch(nx))
        np.testing.assert_array_equal(rows[..., :nx][stored[i]], cube[stored[i]])
        rest = np.concatenate([rows[..., :nx][~stored[i]], rows[..., nx:].ravel(), log[0, i, nz * ny * pitch(nx):]])
        assert (np.isnan(rest) | (rest == np.float32(1e30))).all()
    ent = pack_entries([e for e, _ in c.entries(QUADS, "same")], c.slot_elems)
    assert ent.shape == (1, (len(c.cubes) * c.slot_elems) >> 5, 2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_plant_has_the_status_its_kind_states(name):
    """By the reference alone: each site is a candidate or not, contested or not, as ``PLANTS`` says -- on the whole cube
    and on the stored cube of either layout."""
    c = case(name)
    kinds = {}
    for layout in ([None] if not c.sparse else [ROWS, QUADS]):
        refs = c.reference(layout)
        for i, kind, p, q in c.plants:
            _, pv, is_cand, is_contested = PLANTS[kind]
            r = refs[i]
            assert c.cubes[i][p] == np.float32({"T-e": c.thr - EPS, "T-e+q": c.thr - EPS + Q}.get(pv, pv))
            if is_cand is not None:
                assert bool(r["mask"][p]) == is_cand, (name, layout, i, kind, p, q)
            if r["mask"][p] and is_contested is not None:
                k = int(np.nonzero((r["s"] == p[0]) & (r["z"] == p[1]) & (r["y"] == p[2]) & (r["x"] == p[3]))[0][0])
                assert bool(r["contested"][k]) == is_contested, (name, layout, i, kind, p, q)
                if kind == "neg_border":
                    assert r["nbr_max"][k] == 0 and r["v"][k] < 0
            kinds[kind] = kinds.get(kind, 0) + 1
    print(name, kinds)
    for kind in _CYCLE:
        assert kinds.get(kind, 0) >= 4, (name, kind)
    if c.thr == 0.0:
        assert kinds.get("neg_border", 0) >= 4


@pytest.mark.parametrize("name", DENSE)
def test_dense_cases_hold_what_their_gpu_tests_rely_on(name):
    """Candidates in every block that has room for one, every width of the quad tail and the wave ends, the share of
    voxels above the threshold the case states, pairs across the sigma-chunk seams of all three outcomes, the 3 x 3 x 3 x
    2 plateau whole, and a table of which a third is still a crowd."""
    c = case(name)
    refs = c.reference()
    assert {s[2] for s in c.shapes} >= {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 257}
    assert (1, 1, 1) in c.shapes and any(s[0] == 1 for s in c.shapes) and any(s[1] == 1 for s in c.shapes)
    assert c.slot_elems > max(s[0] * s[1] * pitch(s[2]) for s in c.shapes)
    total = sum(len(r["v"]) for r in refs)
    above = np.concatenate([(cube > c.thr - EPS).ravel() for cube in c.cubes]).mean()
    print("%s: %d candidates, %d contested, %.1f %% of voxels above thr - eps" % (
        name, total, sum(int(r["contested"].sum()) for r in refs), 100 * above))
    assert total >= 150 and total // 3 >= 50
    density = CASES[name]["density"]
    assert (0.2 <= above <= 0.6) if density >= 0.2 else (above <= 0.06)
    assert sum(len(r["v"]) > 0 for r in refs) >= len(refs) - 2
    # every width's last quad holds a candidate in its last column, and every width beyond one quad one in its first
    # ... and where the row does not fill its last quad, one of them has 1e30 in the pitch column beside it
    log = pack_log(c.cubes, c.slot_elems)
    for i, (r, shp) in enumerate(zip(refs, c.shapes)):
        if shp[2] >= 4 and shp[0] * shp[1] >= 9 and shp != PLATEAU_SHAPE:
            last = r["x"] == shp[2] - 1
            assert last.any() and (r["x"] == 0).any(), (name, shp)
            if shp[2] % 4:
                at = (r["z"][last] * shp[1] + r["y"][last]) * pitch(shp[2]) + shp[2]
                assert (log[r["s"][last], i, at] == np.float32(1e30)).any(), (name, shp)
    # the seams between the sigma chunks: a site on either side of each, with a rival across it of every outcome
    outcomes = {}
    for i, kind, p, q in c.plants:
        if q is not None and p[0] in SEAM_SCALES and q[1:] == p[1:] and {p[0], q[0]} in ({7, 8}, {15, 16}):
            outcomes.setdefault(p[0], set()).add(kind)
    for s in SEAM_SCALES:
        if s < c.ns - (s in (7, 15)):
            assert outcomes.get(s, set()) >= {"beaten", "edge_out", "plateau2", "edge_in", "clear_win"}, (name, s, outcomes)
    assert (len(outcomes) > 0) == (c.ns >= 9)
    # the ends of a wave: lone candidates with a larger value elsewhere in their quad
    for kind in ("wave_right", "wave_left"):
        mine = [(i, p, far) for i, k, p, far in c.wave_plants if k == kind]
        assert len(mine) >= 3, (name, kind)
        for i, p, far in mine:
            ny, px = c.shapes[i][1], pitch(c.shapes[i][2])
            quad = ((p[1] * ny + p[2]) * px + p[3]) // 4
            assert quad % 64 == (63 if kind == "wave_right" else 0) and ((far[1] * ny + far[2]) * px + far[3]) // 4 == quad
            assert refs[i]["mask"][p] and c.cubes[i][far] > c.cubes[i][p] + np.float32(EPS) and abs(far[3] - p[3]) == 3
    # the plateau
    assert len(c.plateaus) == 1
    i, on = c.plateaus[0]
    assert int(on.sum()) == 27 * min(c.ns, 2) and refs[i]["mask"][on].all()
    k = refs[i]["mask"][on.nonzero()]
    assert k.all() and refs[i]["contested"][np.isin(refs[i]["v"], np.float32(1.75))].all()


def test_dense_candidates_cover_the_16_kinds_of_place():
    """Inside, on each kind of face, edge and corner of the 4-D cube -- the 16 subsets of the axes -- some dense case has
    a contested and an uncontested candidate whose value the zero padding does not decide alone."""
    seen = {}
    for name in DENSE:
        c = case(name)
        for r, cube in zip(c.reference(), c.cubes):
            kinds = face_kind(cube.shape)[r["s"], r["z"], r["y"], r["x"]]
            for k, cont in zip(kinds, r["contested"]):
                seen.setdefault(int(k), set()).add(bool(cont))
    assert sorted(seen) == list(range(16)) and all(v == {True, False} for v in seen.values()), seen


@pytest.mark.parametrize("layout", [ROWS, QUADS], ids=["rows", "quads"])
@pytest.mark.parametrize("name", SPARSE)
def test_sparse_cases_hold_what_their_gpu_tests_rely_on(name, layout):
    """The library's fit rule, stored and unstored segments, entries whose last bits lie past the block, candidates
    with an unstored neighbour on every side and across an entry seam in x, a scale whose neighbours are not stored at
    all, and (the queue case) more than 1024 candidate bits in one workgroup round in words of differing popcount."""
    c = case(name)
    refs, whole = c.reference(layout), c.reference(None)
    shapes = set(c.shapes)
    if not c.queue:
        assert {s[2] for s in shapes} >= {1, 15, 16, 17, 33, 65} and {s[0] for s in shapes} >= {1, 3, 4, 5, 9}
        assert any((s[0] * pitch(s[2])) % 64 for s in shapes) and any(pitch(s[2]) % 64 for s in shapes)
    n_stored = n_unstored = n_seam = 0
    unstored_side = np.zeros(8, dtype=np.int64)                       # -s +s -z +z -y +y -x +x
    sigma_only = 0
    for i, (cube, r) in enumerate(zip(c.cubes, refs)):
        ns, nz, ny, nx = cube.shape
        for word0 in ("same", "faces"):
            ent, stored = c.entries(layout, word0)[i]
            assert ent.shape[1] * ent.shape[2] <= (c.slot_elems >> 5) - 1              # mmx_batch_geom_make's rule
            assert not (r["mask"] & ~bits_of(ent[..., 0], nz, nx, layout)).any()
        seg = ent[..., 1] != 0
        n_stored, n_unstored = n_stored + int(seg.sum()), n_unstored + int((~seg).sum())
        # the true values of unstored voxels are at most thr - eps: storing them could not change a decision ...
        assert (cube[~stored] <= np.float32(c.thr) - np.float32(EPS)).all()
        # ... so the stored cube nominates what the whole cube does, with the same flags (nbr_max may differ)
        np.testing.assert_array_equal(r["mask"], whole[i]["mask"])
        np.testing.assert_array_equal(r["contested"], whole[i]["contested"])
        padded = np.pad(stored, 1, constant_values=True)                               # (outside the cube: not "unstored")
        idx = (r["s"] + 1, r["z"] + 1, r["y"] + 1, r["x"] + 1)
        faces = [(-1, 0, 0, 0), (1, 0, 0, 0), (0, -1, 0, 0), (0, 1, 0, 0), (0, 0, -1, 0), (0, 0, 1, 0), (0, 0, 0, -1),
                 (0, 0, 0, 1)]
        for k, o in enumerate(faces):
            unstored_side[k] += int((~padded[tuple(a + d for a, d in zip(idx, o))]).sum())
        ent_of, _, _ = entry_map(nz, nx, layout)
        for dx in (-1, 1):
            xx = r["x"] + dx
            ok = (xx >= 0) & (xx < nx)
            n_seam += int((ent_of[r["z"][ok], r["x"][ok]] != ent_of[r["z"][ok], xx[ok]]).sum())
        if (nz, ny, nx) == SEAM_SHAPE and not c.queue:
            assert len(r["v"]) == 4 * ns and int(seg.sum()) == 4 * ns
        if (nz, ny, nx) == SIGMA_ONLY_SHAPE and ns >= 3 and not c.queue:
            mid = ns // 2
            assert stored[mid].mean() > 0.9 and not stored[mid - 1].any() and not stored[mid + 1].any()
            sigma_only += int((r["s"] == mid).sum())
    print("%s layout %d: %d candidates, %d stored / %d unstored segments, unstored face neighbours %s, %d across an entry"
          " seam, %d at the scale stored alone" % (name, layout, sum(len(r["v"]) for r in refs), n_stored, n_unstored,
                                                   unstored_side.tolist(), n_seam, sigma_only))
    assert sum(len(r["v"]) for r in refs) >= 60 and n_stored >= 20 and n_unstored >= 20
    if not c.queue:
        assert (unstored_side[2:] > 0).all() and n_seam > 0
        assert (unstored_side[:2] > 0).all() == (c.ns > 1)
        assert (sigma_only >= 3) == (c.ns >= 3)
    else:
        i, on = c.plateaus[0]
        assert i == len(c.cubes) - 1 and int(on.sum()) > QUEUE and refs[i]["mask"][on].all()
        for word0 in ("same", "faces"):
            per_round, pop = round_bits(c.entries(layout, word0)[i][0])
            print("  word 0 = %s: %s bits per round, popcounts %s" % (word0, per_round.tolist(), sorted(set(pop.tolist()))))
            assert len(per_round) == 1 and per_round[0] > QUEUE and len(set(pop[pop > 0].tolist())) >= 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_loop_on_the_references_own_tables(name):
    """DESIGN.md section 2 on the reference's tables, no kernel involved: nominate, expand and the rules of the host
    resolve, on exact values up to 3 x 2^-16 off the nominated ones in patterns that turn every tie both ways, give
    ``peak_mask`` of the exact cube per block; and a candidate carries the largest deviation, so that the resolve's
    ``max_f32_error`` can be told exactly."""
    c = case(name)
    flipped = 0
    for layout in ([None] if not c.sparse else [ROWS, QUADS]):
        t = c.table(layout)
        probes = probes_ref(t, c.shapes, c.ns)
        kept = {}
        for pattern in (0, 1, -1):
            exact = c.exact(pattern)
            v64 = np.concatenate([exact[i][r["s"], r["z"], r["y"], r["x"]] for i, r in enumerate(c.reference(layout))])
            assert pattern == 0 or np.abs(t["v"] - v64).max() == MAX_DELTA
            rival = np.full(len(t), -np.inf)
            pv = np.array([exact[r[0]][r[1], r[2], r[3], r[4]] for r in probes])
            if len(probes):
                np.maximum.at(rival, probes[:, 5], pv)
            at = 0
            for i, r in enumerate(c.reference(layout)):
                m = len(r["v"])
                border = face_kind(c.cubes[i].shape)[r["s"], r["z"], r["y"], r["x"]] != 0
                rv = np.where(border, np.maximum(rival[at:at + m], 0.0), rival[at:at + m])
                keep = (v64[at:at + m] > c.thr) & (~r["contested"] | (v64[at:at + m] >= rv))
                want, _ = oracle_peaks(exact[i], c.thr)
                got = np.stack([r[f][keep] for f in "zyxs"], axis=1).astype(np.int64)
                if len(got) == c.cubes[i].size > 1:
                    got = got[:0]
                np.testing.assert_array_equal(sort_rows(got), sort_rows(want))
                kept.setdefault(pattern, []).append(keep)
                at += m
        # (contested candidates that are peaks under one pattern and not under its negative: the ties turned)
        flipped += int((np.concatenate(kept[1]) != np.concatenate(kept[-1])).sum())
    assert flipped > 20


@pytest.mark.parametrize("eps", [2e-5, 2.5e-4])
def test_producer_volume_is_hard_enough_by_the_oracle(eps):
    """The float64 oracle's LoG of every block of part 5, each as an image of its own: at least twice the segments
    with and without a response above ``thr - eps`` and twice the candidates the GPU test demands of the device's own
    output, under either layout and band; and the ladder has the radii the producers are chosen by."""
    from magellanmapper_amd import kernels1d as k1
    from oracle import blob_log_oracle as blo
    assert tuple(k1.kernel_radius(sg) for sg in PRODUCER_SIGMAS) == PRODUCER_RADII
    vol = producer_volume()
    assert vol.shape == PRODUCER_SHAPE and vol.dtype == np.uint16
    for o, shp in RAGGED_BLOCKS + [WIDE_BLOCK]:
        assert all(a + n <= m for a, n, m in zip(o, shp, PRODUCER_SHAPE))
        img = blo.img_as_float(vol[o[0]:o[0] + shp[0], o[1]:o[1] + shp[1], o[2]:o[2] + shp[2]]).astype(np.float64)
        cube = np.moveaxis(blo.log_cube(img, np.array([[sg] * 3 for sg in PRODUCER_SIGMAS])), -1, 0).astype(np.float32)
        for layout in (ROWS, QUADS):
            n_st, n_un, n_c = block_stats(cube, layout, PRODUCER_THR, eps)
            print("block %s layout %d: %d stored, %d unstored, %d candidates" % (shp, layout, n_st, n_un, n_c))
            assert n_st >= 2 * PRODUCER_MIN["stored"] and n_un >= 2 * PRODUCER_MIN["unstored"]
            assert n_c >= 2 * PRODUCER_MIN["candidates"]
    assert any(shp[1] < 16 for _, shp in RAGGED_BLOCKS) and all(shp[1] % 16 for _, shp in RAGGED_BLOCKS)
    assert all(shp[0] % 4 and shp[2] % 16 for _, shp in RAGGED_BLOCKS)
