"""GPU tests of the tail of a batch after its kernels were rewritten to keep their loads in flight:
``rescore_kernel`` (csrc/mmx_rescore.hip: every column a thread owns marches through the taps together, the number of
columns compiled in by class, z planes by arithmetic for interior points and from the reflect table otherwise) bit for
bit against the plain-C oracle, and ``peaks_sparse_kernel`` (csrc/mmx_peaks.hip: a pre-check stage and a stage of
32-lane groups, either queue worked off in rounds) against the brute-force reference of tests/test_nms_host.py.
Every comparison is for equality.  Needs a real MI355X (``-m gpu``)."""
import ctypes
import functools

import numpy as np
import pytest

import test_nms_host as H
from test_nms_host import QUADS, ROWS
from gpu_support import cand_key, gpu, rescore_strip, stream_ptr  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WG = 256                                # MMX_WG
RESCORE_GRID = 8192                     # workgroups of one re-score launch


# ---------------------------------------------------------------- 1. the exact re-score
#: radius -> the sigma that has it (radius = int(4 sigma + 0.5)); 30 is the first radius of two strips
RADII = (1, 8, 12, 20, 24, 30)
SIGMAS = tuple((r + 0.2) / 4.0 for r in RADII)
#: (radius index, origin, shape): extents 2R + 3 .. 2R + 5 per radius, and one block of exactly R + 1 (R = 20), where every
#: window reflects on both sides of every axis
RS_BLOCKS = [(0, (0, 0, 0), (5, 6, 7)), (1, (0, 0, 8), (19, 20, 21)), (2, (0, 0, 30), (27, 28, 29)),
             (3, (0, 0, 60), (43, 44, 45)), (4, (0, 0, 106), (51, 52, 53)), (5, (0, 0, 160), (63, 64, 65)),
             (3, (0, 0, 226), (21, 21, 21))]
RS_VOLUME = (64, 66, 250)
#: the long table: this many random rows on the smallest block, at these radius indices
LONG_ROWS, LONG_SCALES = RESCORE_GRID + 300, (0, 1, 2)
#: (name, voxel type, store_f32)
RS_VARIANTS = [("u8", np.uint8, 0), ("u16", np.uint16, 0), ("f32", np.float32, 1), ("f32_f64", np.float32, 0),
               ("f64", np.float64, 0)]


def _col_class(radius, rmax):
    """Columns per thread and pass of a point of this radius (rescore_col_class of csrc/mmx_rescore.hip), and the passes."""
    n = 2 * radius + 1
    cols = -(-(n * min(rescore_strip(rmax), n)) // WG)
    passes = -(-cols // 4)
    per = -(-cols // passes)
    return (1 if per <= 1 else 2 if per <= 2 else 4), passes


def _rs_volume(dtype):
    rng = np.random.default_rng(20)
    v16 = rng.integers(0, 65536, RS_VOLUME, dtype=np.uint16)
    if dtype == np.uint16:
        return v16
    if dtype == np.uint8:
        return (v16 >> 8).astype(np.uint8)
    return (v16 / 65535.0).astype(dtype)


def _block_points(shape, radius, rng):
    """Every corner, one point per face, the planes either side of where the interior z path begins and ends (the
    same along y and x, which have no fast path), random points, and random points whose z window is interior."""
    n = np.asarray(shape)
    mid = n // 2
    pts = [[z, y, x] for z in (0, n[0] - 1) for y in (0, n[1] - 1) for x in (0, n[2] - 1)]
    for ax in range(3):
        for side in (0, n[ax] - 1):
            p = list(mid)
            p[ax] = side
            pts.append(p)
        for at in (radius - 1, radius, n[ax] - radius - 1, n[ax] - radius):
            p = list(mid + 1)
            p[ax] = int(np.clip(at, 0, n[ax] - 1))
            pts.append(p)
    pts += np.stack([rng.integers(0, k, 8) for k in n], axis=1).tolist()
    if n[0] > 2 * radius:
        inner = np.stack([rng.integers(radius, n[0] - radius, 4), rng.integers(0, n[1], 4), rng.integers(0, n[2], 4)], axis=1)
        pts += inner.tolist()
    return np.asarray(pts, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _rs_table():
    """The rows of the one table every variant re-scores: (slot, s, z, y, x), the same for every voxel type."""
    rng = np.random.default_rng(21)
    rows = []
    for b, (si, _, shape) in enumerate(RS_BLOCKS):
        p = _block_points(shape, RADII[si], rng)
        rows.append(np.column_stack((np.full(len(p), b), np.full(len(p), si), p)))
    shape0 = RS_BLOCKS[0][2]
    long_rows = np.column_stack((np.zeros(LONG_ROWS, dtype=np.int64), rng.choice(LONG_SCALES, LONG_ROWS),
                                 *[rng.integers(0, k, LONG_ROWS) for k in shape0]))
    # rows that are nobody's: no slot, a slot past the batch, a scale below and past the ladder
    bad = np.array([[-1, 0, 1, 1, 1], [len(RS_BLOCKS), 0, 1, 1, 1], [0, -1, 1, 1, 1], [0, 64, 1, 1, 1], [0, 1000, 1, 1, 1]])
    rows = np.concatenate(rows + [long_rows, bad])
    rows = rows[rng.permutation(len(rows))]             # (mixed across radii: neighbouring workgroups differ in class)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _rs_expected(name):
    """``v64`` of every row of the table by the oracle (NaN for the rows that are nobody's)."""
    from oracle import blob_log_oracle as blo
    _, dtype, store_f32 = next(v for v in RS_VARIANTS if v[0] == name)
    vol = _rs_volume(dtype)
    rows = _rs_table()
    want = np.full(len(rows), np.nan)
    for b, (_, o, shp) in enumerate(RS_BLOCKS):
        sub = blo.img_as_float(vol[o[0]:o[0] + shp[0], o[1]:o[1] + shp[1], o[2]:o[2] + shp[2]])
        if dtype == np.float32 and not store_f32:
            sub = sub.astype(np.float64)                # (float32 voxels, float64 intermediates)
        mine = (rows[:, 0] == b) & (rows[:, 1] >= 0) & (rows[:, 1] < len(RADII))
        for si in np.unique(rows[mine, 1]):
            m = mine & (rows[:, 1] == si)
            cube = blo.log_cube(sub, np.array([[SIGMAS[si]] * 3]))[..., 0]
            want[m] = cube[rows[m, 2], rows[m, 3], rows[m, 4]].astype(np.float64)
    want.setflags(write=False)
    return want


def _ladder():
    from magellanmapper_amd import blob_log as bl
    sp = [bl.ScaleSpace.make(s, s, 1) for s in SIGMAS]
    return (np.ascontiguousarray(np.concatenate([s.w0_tab for s in sp])),
            np.ascontiguousarray(np.concatenate([s.w2_tab for s in sp])),
            np.ascontiguousarray(np.concatenate([s.radii for s in sp]).astype(np.int32)),
            np.ascontiguousarray(np.concatenate([s.norms for s in sp])))


def _cand_rows(rows):
    from magellanmapper_amd import _native as nat
    pts = np.zeros(len(rows), dtype=nat.CAND_DTYPE)
    for k, f in enumerate(("slot", "s", "z", "y", "x")):
        pts[f] = rows[:, k]
    pts["v64"] = np.nan
    return pts


def test_the_rescore_table_holds_what_its_test_relies_on():
    """Every compiled column class (1, 2 and 4 columns a thread) in one to four passes, the strip loop, both z paths at their first and last plane, more rows than a launch
    has workgroups -- from the table alone (no GPU is used; the mark is the module's)."""
    rmax = max(RADII)
    assert [_col_class(r, rmax) for r in RADII] == [(1, 1), (2, 1), (4, 1), (4, 2), (4, 3), (4, 4)]
    assert rescore_strip(rmax) < 2 * rmax + 1 and rescore_strip(24) == 49
    rows = _rs_table()
    assert len(rows) > RESCORE_GRID
    for b, (si, _, shp) in enumerate(RS_BLOCKS):
        z = rows[(rows[:, 0] == b) & (rows[:, 1] == si), 2]
        r = RADII[si]
        inner = (z - r >= 0) & (z + r < shp[0])
        if shp[0] > 2 * r:
            assert {r - 1, r, shp[0] - r - 1, shp[0] - r} <= set(z.tolist()) and inner.any() and (~inner).any()
        else:
            assert not inner.any()


@pytest.mark.parametrize("name", [v[0] for v in RS_VARIANTS])
def test_rescore_interleaved_columns_bit_exact(gpu, name):
    """One launch per voxel type over blocks of about 2R + 3 voxels an axis for radii 1, 8, 12 (the three column
    classes in one pass), 20, 24 (two and three passes) and 30 (four passes, two strips) and one block of R + 1: corners, faces, the planes z = R - 1, R, nz - R - 1, nz - R
    either side of the interior path (and the same along y and x), random points; 8492 rows of mixed radii on the
    smallest block, so that workgroups walk several points of different classes; rows without a slot or a scale keep
    their NaN.  ``v64`` equals the oracle's cube bit for bit."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    _, dtype, store_f32 = next(v for v in RS_VARIANTS if v[0] == name)
    dvol = bl.DeviceVolume(_rs_volume(dtype))
    w0, w2, radii, norms = _ladder()
    assert tuple(int(r) for r in radii) == RADII
    blocks, _ = bl._make_blocks(dvol, 0, [o for _, o, _ in RS_BLOCKS], [s for _, _, s in RS_BLOCKS])
    d_blocks = bl._to_device_bytes(blocks, gpu)
    pts = _cand_rows(_rs_table())
    d_pts = bl._to_device_bytes(pts, gpu)
    d_w0, d_w2 = torch.from_numpy(w0).to(gpu), torch.from_numpy(w2).to(gpu)
    vol = dvol.view(0, False)
    nat.check(nat.lib().mmx_rescore_f64(
        ctypes.byref(vol), d_blocks.data_ptr(), len(blocks), d_pts.data_ptr(), len(pts), None, d_w0.data_ptr(),
        d_w2.data_ptr(), nat.as_int32_ptr(radii), nat.as_double_ptr(norms), len(radii), store_f32, stream_ptr()),
        "mmx_rescore_f64")
    got = d_pts.cpu().numpy().view(nat.CAND_DTYPE)
    want = _rs_expected(name)
    assert np.isnan(want).sum() == 5
    np.testing.assert_array_equal(got["v64"], want)
    for f in ("slot", "s", "z", "y", "x", "flags", "band"):
        np.testing.assert_array_equal(got[f], pts[f])


def test_rescore_rows_two_gibibytes_apart(gpu):
    """A view whose rows lie 2^29 voxels apart: the (y, x) offsets of the block no longer fit 32 bits of bytes, and the
    kernel takes 64-bit element offsets instead.  uint8 voxels, radius 1 and 8 on a 5 x 5 x 7 block: bit for bit."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    from oracle import blob_log_oracle as blo
    nz, ny, nx = 5, 5, 7
    sy, sz = 1 << 29, 64
    assert (ny - 1) * sy * 1 >= 1 << 31
    rng = np.random.default_rng(22)
    sub = rng.integers(0, 256, (nz, ny, nx), dtype=np.uint8)
    buf = torch.zeros((ny - 1) * sy + (nz - 1) * sz + nx, dtype=torch.uint8, device=gpu)
    view = torch.as_strided(buf, (nz, ny, nx), (sz, sy, 1))
    view.copy_(torch.from_numpy(sub).to(gpu))
    vol = nat.Volume(buf.data_ptr(), nat.MMX_U8, 255.0, sz, sy, 1)
    blocks = np.zeros(1, dtype=nat.BLOCK_DTYPE)
    blocks[0] = (0, nz, ny, nx, 0, H.pitch(nx), 0)
    w0, w2, radii, norms = _ladder()
    g = np.indices((nz, ny, nx)).reshape(3, -1).T
    rows = np.concatenate([np.column_stack((np.zeros(len(g), dtype=np.int64), np.full(len(g), si), g)) for si in (0, 1)])
    pts = _cand_rows(rows)
    d_pts, d_blocks = bl._to_device_bytes(pts, gpu), bl._to_device_bytes(blocks, gpu)
    d_w0, d_w2 = torch.from_numpy(w0).to(gpu), torch.from_numpy(w2).to(gpu)
    nat.check(nat.lib().mmx_rescore_f64(
        ctypes.byref(vol), d_blocks.data_ptr(), 1, d_pts.data_ptr(), len(pts), None, d_w0.data_ptr(), d_w2.data_ptr(),
        nat.as_int32_ptr(radii), nat.as_double_ptr(norms), len(radii), 0, stream_ptr()), "mmx_rescore_f64")
    got = d_pts.cpu().numpy().view(nat.CAND_DTYPE)["v64"]
    cube = blo.log_cube(blo.img_as_float(sub), np.array([[SIGMAS[0]] * 3, [SIGMAS[1]] * 3]))
    want = cube[rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 1]].astype(np.float64)
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- 2. the sparse NMS kernel
NMS_SHAPE = (20, 37, 70)
NMS_THR, NMS_EPS = 0.125, H.EPS
SURVIVOR_QUEUE = 512                    # kQ2 of peaks_sparse_kernel
RAMP = ((1, 13), (1, 13), (1, 13))      # z, y, x ranges: 1728 voxels rising with z by 2^-8 a plane
FLAT = ((6, 15), (20, 29), (30, 39))    # 729 voxels of one value
GUARD = 64
CAP = 1 << 15


def _site_offsets(ns):
    """The neighbours the planted sites use, by what the ladder has: (first, last) of the in-cube neighbours in C order
    of a voxel with a scale either side where there are three, and the offsets of band bits 63, 64 and 79."""
    first, last = H.OFFSETS[0], H.OFFSETS[79]
    if ns < 3:
        first, last = np.array([0, -1, -1, -1]), np.array([0, 1, 1, 1])
    return first, last


@functools.lru_cache(maxsize=None)
def _nms_cube(ns):
    """[ns, 20, 37, 70] float32 on the 2^-16 grid: 3 % of the voxels above the threshold at random, a lone voxel on
    every corner, edge and face of the cube at its first, middle and last scale, the ramp and the flat plateau in scale 0, and the planted sites."""
    rng = np.random.default_rng(30 + ns)
    nz, ny, nx = NMS_SHAPE
    cube = rng.integers(-8192, 4096, (ns, nz, ny, nx)).astype(np.float32) * np.float32(H.Q)    # < thr - eps
    hot = rng.random(cube.shape) < 0.03
    cube[hot] = rng.integers(13000, 58000, int(hot.sum())).astype(np.float32) * np.float32(H.Q)
    for box in (RAMP, FLAT):            # nothing random beside, above or one scale above either plateau
        cube[:2, box[0][0] - 1:box[0][1] + 1, box[1][0] - 1:box[1][1] + 1, box[2][0] - 1:box[2][1] + 1] = -0.25
    cube[0, slice(*RAMP[0]), slice(*RAMP[1]), slice(*RAMP[2])] = (
        np.float32(0.25) + np.arange(RAMP[0][1] - RAMP[0][0], dtype=np.float32)[:, None, None] * np.float32(2.0 ** -8))
    cube[0, slice(*FLAT[0]), slice(*FLAT[1]), slice(*FLAT[2])] = 0.75
    for z in (0, nz // 2, nz - 1):
        for y in (0, ny // 2, ny - 1):
            for x in (0, nx // 2, nx - 1):
                for s in {0, ns // 2, ns - 1}:
                    cube[s, z, y, x] = 1.5
    first, last = _site_offsets(ns)
    s0 = 1 if ns >= 3 else 0
    sites = {}

    def plant(name, p, neighbours):
        p = np.asarray(p)
        lo = np.maximum(p - 1, 0)
        cube[lo[0]:p[0] + 2, lo[1]:p[1] + 2, lo[2]:p[2] + 2, lo[3]:p[3] + 2] = -0.25
        cube[tuple(p)] = 1.0
        for o, val in neighbours:
            cube[tuple(p + o)] = val
        sites[name] = tuple(int(k) for k in p)

    beat, edge = 1.0 + NMS_EPS + H.Q, 1.0 + NMS_EPS
    plant("beaten_by_last", (s0, 16, 4, 50), [(last, beat)])
    plant("beaten_by_first", (s0, 16, 8, 50), [(first, beat)])
    plant("edge_with_last", (s0, 16, 12, 50), [(last, edge)])
    plant("edge_with_first", (s0, 16, 16, 50), [(first, edge)])
    if ns >= 2:
        plant("band_63_64_79", (s0, 16, 30, 60), [(H.OFFSETS[j], 1.0 - NMS_EPS) for j in (63, 64, 79)])
    cube.setflags(write=False)
    return cube, sites


@functools.lru_cache(maxsize=None)
def _nms_reference(ns, layout):
    cube, _ = _nms_cube(ns)
    ent, stored = H.entries_from(cube, NMS_THR, NMS_EPS, layout, "same")
    ref = H.nominate_ref(cube, stored, NMS_THR, NMS_EPS)
    n = len(ref["v"])
    t = np.zeros(n, dtype=[("slot", "<i4"), ("s", "<i4"), ("z", "<i4"), ("y", "<i4"), ("x", "<i4"), ("flags", "<u4"),
                           ("v", "<f4"), ("nbr_max", "<f4"), ("band", "<u8")])
    for f in ("s", "z", "y", "x", "v", "nbr_max", "band"):
        t[f] = ref[f]
    t["flags"] = ref["contested"].astype(np.uint32) * H.CONTESTED | np.uint32(H.BAND) | (ref["band_hi"] << np.uint32(16))
    return ent, stored, t, ref["mask"]


def _survivors(cube, stored, word0_bits):
    """Set bits that pass the kernel's pre-check: no stored z +- 1 or sigma +- 1 neighbour above v + eps."""
    eff = np.where(stored, cube, np.float32(-np.inf))
    pad = np.pad(eff, ((1, 1), (1, 1), (0, 0), (0, 0)), constant_values=-np.inf)
    rival = np.maximum(np.maximum(pad[1:-1, :-2], pad[1:-1, 2:]), np.maximum(pad[:-2, 1:-1], pad[2:, 1:-1]))
    return word0_bits & ~(rival > cube + np.float32(NMS_EPS))


def _slot_elems():
    nz, ny, nx = NMS_SHAPE
    return -(-(nz * ny * H.pitch(nx) + 64) // 32) * 32 + 2048


def _nms_run(dev, ns, layout, cap):
    from magellanmapper_amd import _native as nat, blob_log as bl
    cube, _ = _nms_cube(ns)
    ent, stored, _, _ = _nms_reference(ns, layout)
    slot = _slot_elems()
    blocks = np.zeros(1, dtype=nat.BLOCK_DTYPE)
    blocks[0] = (0, *NMS_SHAPE, 0, H.pitch(NMS_SHAPE[2]), 0)
    d_blocks = bl._to_device_bytes(blocks, dev)
    log = torch.from_numpy(H.pack_log([cube], slot, [stored])).to(dev)
    masks = torch.from_numpy(H.pack_entries([ent], slot).view(np.int64)).to(dev)
    item = nat.CAND_DTYPE.itemsize
    table = torch.full(((cap + GUARD) * item,), 0xA5, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.check(nat.lib().mmx_peaks_batch(log.data_ptr(), masks.data_ptr(), layout, ns, d_blocks.data_ptr(),
                                        blocks.ctypes.data, 1, slot, NMS_THR, NMS_EPS, table.data_ptr(), cap,
                                        count.data_ptr(), stream_ptr()), "mmx_peaks_batch")
    torch.cuda.synchronize()
    return int(count.item()), table.cpu().numpy().view(nat.CAND_DTYPE)


def _sorted(rows):
    return rows[np.lexsort(cand_key(rows).T[::-1])]


def _assert_same_rows(got, want):
    np.testing.assert_array_equal(cand_key(got), cand_key(want))
    for f in ("v", "nbr_max"):
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32))
    np.testing.assert_array_equal(got["flags"], want["flags"])
    np.testing.assert_array_equal(got["band"], want["band"])
    assert np.isnan(got["v64"]).all()


@pytest.mark.parametrize("layout", [ROWS, QUADS], ids=["rows", "quads"])
@pytest.mark.parametrize("ns", [1, 2, 5])
def test_the_nms_cube_holds_what_its_test_relies_on(ns, layout):
    """From the reference alone (no GPU is used; the mark is the module's).  Scale 0 of the block lies in the first
    workgroup round (2048 entry words; a scale has 1110 row entries or 925 quad entries).  Its word 0 holds the 1728
    voxels of the ramp, the 729 of the flat plateau and the random 3 %: more than the 1024 bits the first queue takes.
    The pre-check passes the top plane of the ramp (144) and all 729 of the plateau: more than the 512 the survivor
    queue takes.  The planted sites have the status their names state."""
    cube, sites = _nms_cube(ns)
    ent, stored, table, mask = _nms_reference(ns, layout)
    per_round, _ = H.round_bits(ent)
    assert ent.shape[1] * ent.shape[2] <= H.ROUND_WORDS and per_round[0] > H.QUEUE + 1728
    bits0 = H.bits_of(ent[..., 0], NMS_SHAPE[0], NMS_SHAPE[2], layout)
    surv = _survivors(cube, stored, bits0)
    ramp = surv[0, slice(*RAMP[0]), slice(*RAMP[1]), slice(*RAMP[2])]
    flat = surv[0, slice(*FLAT[0]), slice(*FLAT[1]), slice(*FLAT[2])]
    assert ramp.sum() == 144 and ramp[-1].all() and flat.all() and flat.sum() == 729
    assert surv[0].sum() > SURVIVOR_QUEUE + 256
    assert mask[0, slice(*FLAT[0]), slice(*FLAT[1]), slice(*FLAT[2])].all()
    kinds = H.face_kind(cube.shape)[mask]
    assert set(range(16)) <= set(kinds.tolist()) if ns >= 3 else set(kinds.tolist()) >= {1, 3, 5, 7, 9, 11, 13, 15}
    row = {tuple(k[1:]): i for i, k in enumerate(cand_key(table))}
    assert sites["beaten_by_last"] not in row and sites["beaten_by_first"] not in row
    first, last = _site_offsets(ns)
    where = {tuple(o): j for j, o in enumerate(H.OFFSETS)}
    for name, o in (("edge_with_last", last), ("edge_with_first", first)):
        r = table[row[sites[name]]]
        j = where[tuple(o)]
        band = int(r["band"]) | (int(r["flags"]) >> 16) << 64
        assert band == 1 << j and r["flags"] & H.CONTESTED
    if ns >= 3:
        assert tuple(last) == (1, 1, 1, 1) and tuple(first) == (-1, -1, -1, -1)
    if ns >= 2:
        r = table[row[sites["band_63_64_79"]]]
        assert int(r["band"]) == 1 << 63 and int(r["flags"]) >> 16 == (1 << 0) | (1 << 15)
    assert 1500 < len(table) < CAP


@pytest.mark.parametrize("layout", [ROWS, QUADS], ids=["rows", "quads"])
@pytest.mark.parametrize("ns", [1, 2, 5])
def test_sparse_kernel_in_two_stages_nominates_exactly_the_reference(gpu, ns, layout):
    """The whole table as a sorted set of rows, every field, and the counter; the rows behind the table untouched."""
    _, _, want, _ = _nms_reference(ns, layout)
    count, table = _nms_run(gpu, ns, layout, CAP)
    print("ns", ns, "layout", layout, "candidates", count, "reference", len(want))
    assert count == len(want)
    _assert_same_rows(_sorted(table[:count]), want)
    assert (table[CAP:].view(np.uint8) == 0xA5).all()


@pytest.mark.parametrize("layout", [ROWS, QUADS], ids=["rows", "quads"])
def test_sparse_kernel_counts_past_a_table_that_is_too_small(gpu, layout):
    """``cap`` a third of the candidates: the counter is the full count, the rows written are distinct members of the
    reference with their fields, nothing behind the table is touched."""
    ns = 2
    _, _, want, _ = _nms_reference(ns, layout)
    cap = len(want) // 3
    count, table = _nms_run(gpu, ns, layout, cap)
    assert count == len(want)
    got = _sorted(table[:cap])
    assert len(np.unique(cand_key(got), axis=0)) == cap
    pos = {tuple(k): i for i, k in enumerate(cand_key(want))}
    idx = [pos.get(tuple(k), -1) for k in cand_key(got)]
    assert min(idx) >= 0
    _assert_same_rows(got, want[idx])
    assert (table[cap:].view(np.uint8) == 0xA5).all()
