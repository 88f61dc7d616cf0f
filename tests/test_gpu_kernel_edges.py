"""GPU tests of the branches only larger or odder inputs take: kernel radii far above the register-resident ones,
the strip loop of the exact re-score, and the table and resampling kernels beyond the sizes of their fixtures.
Every case is a small input with its float64 reference computed here (NumPy / SciPy / ``oracle/``), and each test
asserts that the branch it is about really ran.  Needs a real MI355X (``-m gpu``)."""
import ctypes
import math

import numpy as np
import pytest

from gpu_support import as_dtype, gpu, rescore_strip, stream_ptr  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LOG_TOL = 1e-4


@pytest.fixture(params=["native", "numpy"])
def host_path(request, monkeypatch):
    """Both host formulations of the per-batch decisions (as in test_gpu_parity.py)."""
    from magellanmapper_amd import blob_log as bl
    monkeypatch.setattr(bl, "HOST_PATH", request.param)
    return request.param


DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
DTYPE_IDS = ["u8", "u16", "f32", "f64"]


# ---------------------------------------------------------------- 1. LoG cube at large radii
LARGE_RADII = (26, 31, 43, 64, 100, 180, 255)
# thin along every axis (3, 5 and 9 voxels: R >= 2n for every radius here), long along the others, and one thick block
THIN_ORIGINS = [(3, 10, 0), (20, 0, 150), (0, 100, 17), (5, 200, 240)]
THIN_SHAPES = [(7, 40, 300), (3, 260, 9), (40, 5, 33), (34, 36, 40)]


@pytest.fixture(scope="module")
def thin_volume():
    from magellanmapper_amd import synth
    return synth.make_volume(101, (40, 260, 300), 14, blob_sigma=7.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_log_cube_at_large_radii_on_blocks_thinner_than_the_radius(gpu, thin_volume, dtype):
    """Radii 26..255 (sigma = (R + 0.2) / 4) take the generic passes of mmx_generic.hip on both entries
    (``mmx_log_batch_f32`` falls back to them above MMX_MAX_RADIUS_FAST); one batch holds blocks thinner than half the
    radius along each axis -- SciPy's ``reflect`` extension wraps there several times -- beside a thick one."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    from oracle import blob_log_oracle as blo
    vol = as_dtype(thin_volume, dtype)
    dvol = bl.DeviceVolume(vol)
    subs = [blo.img_as_float(vol[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]])
            for o, s in zip(THIN_ORIGINS, THIN_SHAPES)]
    tol = LOG_TOL * 1e-2
    try:
        for R in LARGE_RADII:
            sigma = (R + 0.2) / 4.0
            space = bl.ScaleSpace.make(sigma, sigma, 1)
            assert space.radii[0] == R
            for a in range(3):          # the branch: at least one block has R >= 2n on every axis
                assert any(R >= 2 * s[a] for s in THIN_SHAPES)
            want = [blo.log_cube(sub, np.array([[sigma] * 3]))[..., 0] for sub in subs]
            for generic in (False, True):
                nat.timing_enable(True)
                nat.timing_read()
                cubes = bl.log_cube_blocks(dvol, 0, THIN_ORIGINS, THIN_SHAPES, space, generic=generic)
                kinds = nat.timing_read()
                nat.timing_enable(False)
                # no register-resident or fused pass ran; the default entry fell back to its three generic passes
                # (the generic entry itself launches them untimed)
                assert all(kinds[k][1] == 0 for k in ("zpass", "ypass", "xpass", "zxpass", "y2pass", "zxpack"))
                assert kinds["generic"][1] == (0 if generic else 3), (R, generic, kinds)
                assert bl.LAST_ZX_PATH == (None if generic else nat.MMX_ZX_SEPARATE)
                for shp, got, ref in zip(THIN_SHAPES, cubes, want):
                    err = np.abs(got[..., 0] - ref).max()
                    assert got.shape[:3] == shp and err < tol, (R, generic, shp, err)
    finally:
        nat.timing_enable(False)


# ---------------------------------------------------------------- 2. exact re-score: the strip loop
def _n_strips(r, strip):
    n = 2 * r + 1
    return -(-n // min(strip, n))


def _ladder(sigmas):
    """Half-kernel tables, radii and norms of a sigma ladder given scale by scale (each as blob_log computes it)."""
    from magellanmapper_amd import blob_log as bl
    sp = [bl.ScaleSpace.make(s, s, 1) for s in sigmas]
    return (np.ascontiguousarray(np.concatenate([s.w0_tab for s in sp])),
            np.ascontiguousarray(np.concatenate([s.w2_tab for s in sp])),
            np.ascontiguousarray(np.concatenate([s.radii for s in sp]).astype(np.int32)),
            np.ascontiguousarray(np.concatenate([s.norms for s in sp])))


def _boundary(shape):
    """Every face, edge and corner voxel of a block, and how many of its coordinates lie on a face."""
    g = np.indices(shape).reshape(3, -1).T
    on = ((g == 0) | (g == np.array(shape) - 1)).sum(axis=1)
    return g[on > 0], on[on > 0]


def _rescore(dvol, origins, shapes, ladder, pts, store_f32, dev):
    from magellanmapper_amd import _native as nat, blob_log as bl
    w0, w2, radii, norms = ladder
    blocks, _ = bl._make_blocks(dvol, 0, origins, shapes)
    d_blocks = bl._to_device_bytes(blocks, dev)
    d_pts = bl._to_device_bytes(pts, dev)
    d_w0, d_w2 = torch.from_numpy(w0).to(dev), torch.from_numpy(w2).to(dev)
    vol = dvol.view(0, False)
    nat.check(nat.lib().mmx_rescore_f64(
        ctypes.byref(vol), d_blocks.data_ptr(), len(blocks), d_pts.data_ptr(), len(pts), None, d_w0.data_ptr(),
        d_w2.data_ptr(), nat.as_int32_ptr(radii), nat.as_double_ptr(norms), len(radii), store_f32, stream_ptr()),
        "mmx_rescore_f64")
    return d_pts.cpu().numpy().view(nat.CAND_DTYPE)["v64"]


RESCORE_ORIGINS = [(0, 0, 0), (5, 3, 20), (12, 20, 1)]
RESCORE_SHAPES = [(9, 12, 11), (5, 9, 4), (7, 13, 6)]
# (sigmas of one call, the radius whose strip count is asserted, expected strips per point radius)
RESCORE_CASES = [((7.3,), {29: 1}), ((7.55,), {30: 2}), ((7.8,), {31: 2}), ((10.8,), {43: 3}),
                 ((63.8,), {255: 103}), ((0.8, 50.05), {3: 1, 200: 58}), ((1.3, 63.8), {5: 3, 255: 103})]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_rescore_strip_loop_bit_exact(gpu, dtype):
    """``mmx_rescore_f64`` stages the x window in LDS strips whose width comes from the batch's LARGEST radius, each
    point running its own 2R + 1 columns through them: one strip (R = 29), two with a last one of one column (R = 30)
    or five (R = 31), three with a remainder of 3 (R = 43), 103 (R = 255), and small-radius points under the strip
    width of a large radius (R = 3 beside R = 200; R = 5 beside R = 255: three strips of 5, 5, 1).  Every face, edge
    and corner voxel (fewer at R >= 200) and random inner points of three small blocks: bit for bit the oracle cube."""
    from magellanmapper_amd import _native as nat, blob_log as bl, synth
    from oracle import blob_log_oracle as blo
    vol = as_dtype(synth.make_volume(5, (24, 40, 36), 10, blob_sigma=2.5), dtype)
    dvol = bl.DeviceVolume(vol)
    store_f32 = 1 if dtype == np.float32 else 0
    rng = np.random.default_rng(17)
    for sigmas, strips in RESCORE_CASES:
        lad = _ladder(sigmas)
        radii = lad[2]
        assert sorted(strips) == sorted(int(r) for r in radii)
        strip = rescore_strip(int(radii.max()))
        for r, n in strips.items():
            assert _n_strips(r, strip) == n, (r, strip)
        rows, want = [], []
        for b, (o, shp) in enumerate(zip(RESCORE_ORIGINS, RESCORE_SHAPES)):
            sub = blo.img_as_float(vol[o[0]:o[0] + shp[0], o[1]:o[1] + shp[1], o[2]:o[2] + shp[2]])
            cube = blo.log_cube(sub, np.array([[s] * 3 for s in sigmas]))
            bnd, on = _boundary(shp)
            for s, r in enumerate(radii):
                if r < 200:
                    pts = bnd
                else:           # (1e8 taps per point: corners, some edge and face voxels)
                    pick = np.concatenate((np.flatnonzero(on == 3),
                                           rng.choice(np.flatnonzero(on < 3), 12, replace=False)))
                    pts = bnd[pick]
                inner = np.stack([rng.integers(0, n, 6) for n in shp], axis=1)
                pts = np.concatenate((pts, inner))
                rows.append(np.column_stack((np.full(len(pts), b), np.full(len(pts), s), pts)))
                want.append(cube[pts[:, 0], pts[:, 1], pts[:, 2], s])
        rows = np.concatenate(rows)
        pts = np.zeros(len(rows), dtype=nat.CAND_DTYPE)
        for k, name in enumerate(("slot", "s", "z", "y", "x")):
            pts[name] = rows[:, k]
        pts["v64"] = np.nan
        got = _rescore(dvol, RESCORE_ORIGINS, RESCORE_SHAPES, lad, pts, store_f32, gpu)
        np.testing.assert_array_equal(got, np.concatenate(want).astype(np.float64), err_msg=str(sigmas))


# ---------------------------------------------------------------- 3. blob_log end to end at large sigma
LARGE_SIGMA_CASES = {"sigma_8_12": ((48, 64, 64), 6, 9.0, (8.0, 12.0, 4)),
                     "sigma_15_25": ((56, 80, 80), 4, 18.0, (15.0, 25.0, 2))}
_LARGE_SIGMA_ORACLE = {}


@pytest.mark.parametrize("case", sorted(LARGE_SIGMA_CASES))
def test_blob_log_at_large_sigma_matches_oracle(gpu, case, host_path):
    """Radii 32..48 (four scales) and 60 / 100 (two) on volumes whose blobs have those sizes: generic passes, the
    re-score's multi-strip loop for every candidate and probe, and the prune -- the same rows in the same order."""
    from magellanmapper_amd import blob_log as bl, synth
    from oracle import blob_log_oracle as blo
    shape, n_blobs, blob_sigma, (lo, hi, ns) = LARGE_SIGMA_CASES[case]
    vol = synth.make_volume(7, shape, n_blobs, blob_sigma=blob_sigma, margin=10)
    space = bl.ScaleSpace.make(lo, hi, ns)
    assert space.radii.min() > 30 and _n_strips(int(space.radii.max()), rescore_strip(int(space.radii.max()))) > 2
    if case not in _LARGE_SIGMA_ORACLE:
        _LARGE_SIGMA_ORACLE[case] = blo.blob_log(vol, lo, hi, ns, 0.05, 0.5)
    want = _LARGE_SIGMA_ORACLE[case]
    got = bl.blob_log(vol, lo, hi, ns, 0.05, 0.5)
    assert len(want) >= 2
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- 4. mmx_overlap_pairs
def _overlap_pairs_ref(allb, offsets, overlap, band, max_sigma):
    """All pairs ``(i, j)``, ``i < j`` of each block whose overlap fraction exceeds ``overlap - band``, and the fractions:
    skimage's ``_blob_overlap`` (oracle/blob_log_oracle.py ``blob_overlap``) restated in float64 NumPy in the operation
    order the kernel states (products where Python calls ``**``)."""
    from scipy import spatial
    root3 = math.sqrt(3.0)
    out_p, out_f = [], []
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi - lo < 2:
            continue
        blk = allb[lo:hi]
        cand = spatial.cKDTree(blk[:, :3]).query_pairs(2 * root3 * max_sigma + 2.0, output_type="ndarray")
        if not len(cand):
            continue
        i, j = cand.min(axis=1), cand.max(axis=1)
        bi, bj = blk[i], blk[j]
        si, sj = bi[:, 3], bj[:, 3]
        with np.errstate(all="ignore"):
            first = si > sj
            ms = np.where(first, si, sj)
            r1 = np.where(first, 1.0, si / sj)
            r2 = np.where(first, sj / si, 1.0)
            den = ms * root3
            d0 = bj[:, 0] / den - bi[:, 0] / den
            d1 = bj[:, 1] / den - bi[:, 1] / den
            d2 = bj[:, 2] / den - bi[:, 2] / den
            d = np.sqrt((d0 * d0 + d1 * d1) + d2 * d2)
            rs = r1 + r2
            tt = rs - d
            vol = np.pi / (12 * d) * (tt * tt) * (d * d + 2 * d * rs - 3 * (r1 * r1 + r2 * r2) + 6 * r1 * r2)
            rm = np.minimum(r1, r2)
            f = np.where(d <= np.abs(r1 - r2), 1.0, vol / (4. / 3 * np.pi * (rm * rm * rm)))
        keep = ~((si == 0) & (sj == 0)) & ~(d > rs) & (f > overlap - band)
        out_p.append(np.stack((i[keep] + lo, j[keep] + lo), axis=1))
        out_f.append(f[keep])
    if not out_p:
        return np.zeros((0, 2), dtype=np.int64), np.zeros(0)
    p, f = np.concatenate(out_p), np.concatenate(out_f)
    order = np.lexsort((p[:, 1], p[:, 0]))
    return p[order], f[order]


def _edge_blobs():
    """Pairs at the exact geometric edges of ``_blob_overlap``, 100 voxels apart from each other."""
    r3 = math.sqrt(3.0)
    rows = []
    y = 0.0
    # spheres that touch (d = r1 + r2, equal sigmas 2): at the distance and a few ulps of d either side
    x0 = 2 * 2 * r3
    for x in (x0, x0 * (1 + 1e-15), x0 * (1 - 1e-15)):
        rows += [(0.0, y, 0.0, 2.0), (0.0, y, x, 2.0)]
        y += 100
    # one sphere inside the other, touching (d = |r1 - r2|: sigmas 3 and 1)
    x0 = (2.0 / 3.0) * 3 * r3
    for x in (x0, x0 * (1 + 1e-15), x0 * (1 - 1e-15)):
        rows += [(0.0, y, 0.0, 3.0), (0.0, y, x, 1.0)]
        y += 100
    rows += [(5.0, y, 5.0, 1.5), (5.0, y, 5.0, 1.5)]               # equal sigmas, coincident: fraction 1
    y += 100
    rows += [(5.0, y, 5.0, 1.5), (6.0, y, 5.0, 1.5)]               # equal sigmas, lens
    y += 100
    rows += [(20.0, y, 20.0, 0.0), (20.0, y, 20.0, 0.0)]           # both sigmas zero: never a pair
    y += 100
    rows += [(20.0, y, 20.0, 0.0), (20.0, y, 21.0, 1.0)]           # one zero sigma: a point inside a sphere
    return np.array(rows, dtype=np.float64)


def _overlap_table():
    rng = np.random.default_rng(8)
    big = np.column_stack((rng.integers(0, 60, (4500, 3)).astype(np.float64),
                           rng.choice([1.0, 1.5, 2.0, 2.5], 4500)))
    small = np.column_stack((rng.integers(0, 12, (40, 3)).astype(np.float64), rng.choice([1.0, 2.5], 40)))
    parts = [small, big, np.zeros((0, 4)), _edge_blobs(), small[:3]]
    offsets = np.zeros(len(parts) + 1, dtype=np.int32)
    np.cumsum([len(p) for p in parts], out=offsets[1:])
    return np.ascontiguousarray(np.concatenate(parts)), offsets


def _overlap_call(allb, offsets, overlap, band, max_sigma, cap, guard, dev):
    from magellanmapper_amd import _native as nat
    d_blobs = torch.from_numpy(allb).to(dev)
    d_off = torch.from_numpy(offsets).to(dev)
    d_pairs = torch.full(((cap + guard) * 2,), -7, dtype=torch.int32, device=dev)
    d_frac = torch.full((cap + guard,), -3.5, dtype=torch.float64, device=dev)
    d_count = torch.zeros(1, dtype=torch.int32, device=dev)
    nat.check(nat.lib().mmx_overlap_pairs(d_blobs.data_ptr(), d_off.data_ptr(), len(offsets) - 1, overlap, band,
                                          max_sigma, d_pairs.data_ptr(), d_frac.data_ptr(), cap, d_count.data_ptr(),
                                          stream_ptr()), "mmx_overlap_pairs")
    n = int(d_count.item()) & 0xFFFFFFFF
    return n, d_pairs.cpu().numpy().reshape(-1, 2).astype(np.int64), d_frac.cpu().numpy()


def test_overlap_pairs_rounds_chunks_edges_and_cap(gpu):
    """``mmx_overlap_pairs`` against the float64 restatement of ``_blob_overlap``: a block of 4500 blobs (three
    rounds of 8 x 256 rows, three LDS chunks of 2048 centres) between small blocks and an empty one in the same call;
    touching spheres (d = r1 + r2) and inner tangency (d = |r1 - r2|) with their one-ulp neighbours, coincident equal
    sigmas, a zero-sigma pair and a zero sigma beside a sphere; limits with and without a band.  Pairs as sets,
    fractions bit for bit.  A table smaller than the pair count: the count is exact, the first ``cap`` entries are
    true pairs, nothing lands past ``cap``."""
    from oracle import blob_log_oracle as blo
    allb, offsets = _overlap_table()
    max_sigma = float(allb[:, 3].max())
    sizes = np.diff(offsets)
    assert sizes.max() > 4096 and -(-sizes.max() // (8 * 256)) > 1 and -(-sizes.max() // 2048) > 2   # rounds, chunks
    guard = 1024
    e0, e1 = int(offsets[3]), int(offsets[4])
    edges = {}
    for overlap, band in ((0.5, 0.0), (0.5, 0.05), (0.0, 0.0), (0.9, 0.3)):
        want_p, want_f = _overlap_pairs_ref(allb, offsets, overlap, band, max_sigma)
        n, pairs, frac = _overlap_call(allb, offsets, overlap, band, max_sigma, len(want_p) + 16, guard, gpu)
        assert n == len(want_p), (overlap, band, n, len(want_p))
        order = np.lexsort((pairs[:n, 1], pairs[:n, 0]))
        np.testing.assert_array_equal(pairs[:n][order], want_p, err_msg=str((overlap, band)))
        np.testing.assert_array_equal(frac[:n][order], want_f, err_msg=str((overlap, band)))
        assert (pairs[n:] == -7).all() and (frac[n:] == -3.5).all()
        edges[(overlap, band)] = {(int(i) - e0, int(j) - e0): f for (i, j), f in zip(want_p, want_f) if e0 <= i < e1}
    # the edges were reached: touching spheres just inside (a sliver of a lens) and just outside (no pair); inner
    # tangency on the containment branch and just past it on the lens one; coincident spheres; zero sigmas
    edge0, edge = edges[(0.0, 0.0)], edges[(0.5, 0.05)]
    assert 0.0 < edge0[(4, 5)] < 1e-20 and (2, 3) not in edge0
    assert edge[(10, 11)] == 1.0 and abs(edge[(8, 9)] - 1.0) < 1e-12
    assert edge[(12, 13)] == 1.0 and edge[(18, 19)] == 1.0 and (16, 17) not in edge0
    # the restatement is skimage's own function up to the rounding of its libm calls
    want_p, want_f = _overlap_pairs_ref(allb, offsets, 0.5, 0.05, max_sigma)
    rng = np.random.default_rng(2)
    for k in rng.choice(len(want_p), 400, replace=False):
        i, j = want_p[k]
        assert abs(want_f[k] - blo.blob_overlap(allb[i], allb[j])) <= 1e-13
    # a table a third of the pair count: exact count, true pairs, the guard untouched
    cap = len(want_p) // 3
    n, pairs, frac = _overlap_call(allb, offsets, 0.5, 0.05, max_sigma, cap, guard, gpu)
    assert n == len(want_p)
    ref = {(int(i), int(j)): f for (i, j), f in zip(want_p, want_f)}
    got = {(int(i), int(j)): f for (i, j), f in zip(pairs[:cap], frac[:cap])}
    assert len(got) == cap and all(ref.get(p) == f for p, f in got.items())
    assert (pairs[cap:] == -7).all() and (frac[cap:] == -3.5).all()


def test_overlap_pairs_table_overflow_is_retried(gpu, monkeypatch):
    """``host_resolve._prune_batch`` (the prune for peaks that are not a native PeakBatch): a block of 64 blobs on a
    4 x 4 x 4 grid has 2016 over-limit pairs, more than the first table (1024 rows) holds -- the call is made again
    with room for all of them, and the pairs it hands on are the reference's; the blobs left are the oracle's."""
    from magellanmapper_amd import _native as nat, blob_log as bl, host_resolve as hr
    from oracle import blob_log_oracle as blo
    L = nat.lib()
    real, real_apply = L.mmx_overlap_pairs, hr._apply_pairs
    caps, seen = [], []

    def counting(*args):
        caps.append(int(args[8]))
        return real(*args)

    def capture(allb, sig, offsets, pairs, frac, overlap, stats, only_blocks=None):
        seen.append((pairs.copy(), frac.copy()))
        return real_apply(allb, sig, offsets, pairs, frac, overlap, stats, only_blocks)

    monkeypatch.setattr(L, "mmx_overlap_pairs", counting)
    monkeypatch.setattr(hr, "_apply_pairs", capture)
    space = bl.ScaleSpace.make(3.0, 3.0, 1)
    grid = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), axis=-1).reshape(-1, 3) + 10
    other = np.array([[40, 40, 40], [41, 40, 40], [60, 60, 60]])
    peaks = [(np.column_stack((grid, np.zeros(64, dtype=np.int64))).astype(np.int32), np.zeros(64)),
             (np.column_stack((other, np.zeros(3, dtype=np.int64))).astype(np.int32), np.zeros(3))]
    stats = bl.BatchStats()
    res = hr._prune_batch(peaks, space, 0.1, gpu, stats)
    allb = np.concatenate([c for c, _ in peaks]).astype(np.float64)
    allb[:, 3] = space.sigmas[0]
    offsets = np.array([0, 64, 67], dtype=np.int32)
    want_p, want_f = _overlap_pairs_ref(allb, offsets, 0.1, hr.OVERLAP_BAND, float(space.sigmas[0]))
    assert len(want_p) == 2016 + 1 and stats.n_overlap_pairs == len(want_p)
    assert caps == [1024, len(want_p) + 64], caps
    (pairs, frac), = seen
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    np.testing.assert_array_equal(pairs[order], want_p)
    np.testing.assert_array_equal(frac[order], want_f)
    for b in range(2):
        np.testing.assert_array_equal(res[b], blo.prune_blobs(allb[offsets[b]:offsets[b + 1]], 0.1))


# ---------------------------------------------------------------- 5. resampling kernels
def _block_table(origins, shapes, strides, pad=None):
    from magellanmapper_amd import _native as nat
    blocks = np.zeros(len(shapes), dtype=nat.BLOCK_DTYPE)
    for i, (o, s) in enumerate(zip(origins, shapes)):
        px = -(-s[2] // nat.MMX_ROW_ALIGN) * nat.MMX_ROW_ALIGN
        blocks[i] = (int(np.dot(o, strides)), s[0], s[1], s[2], i, px, 0 if pad is None else pad[i])
    return blocks


# (in extent, out extent): x up to 383 / 384 (six 64-lane column groups: x tables in registers) and 385 / 700
# (seven and eleven: tables reloaded per row); z up, z down, y down; z only with rows of 200 and of 400
RESIZE_CASES = [((5, 7, 300), (9, 7, 383)), ((5, 7, 300), (3, 7, 384)), ((6, 8, 300), (6, 8, 385)),
                ((4, 8, 900), (4, 5, 700)), ((6, 5, 200), (11, 5, 200)), ((6, 5, 400), (11, 5, 400))]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_resize_wide_rows_bit_exact(gpu, dtype):
    """``mmx_minmax_batch`` + ``mmx_resize_batch_as`` on one batch of the cases above, each against
    ``scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True)`` of the block, clipped to the block's range and cast
    back to its type (truncation for integers) as ``preprocess.Rescaler`` states; bit for bit (and the float32 copy of
    a float64 result is its rounding)."""
    from scipy import ndimage as ndi
    from magellanmapper_amd import _native as nat, blob_log as bl, preprocess
    rng = np.random.default_rng(19)
    vol = as_dtype(rng.integers(0, 65536, (6, 8, 900)).astype(np.uint16), dtype)
    dvol = bl.DeviceVolume(vol)
    src = dvol.view(0, False)
    strides = (src.stride_z, src.stride_y, src.stride_x)
    nb = len(RESIZE_CASES)
    ins = [c[0] for c in RESIZE_CASES]
    outs = [c[1] for c in RESIZE_CASES]
    nxc = [-(-o[2] // 64) for o in outs]
    assert min(nxc) <= 6 < max(nxc) and sum(n > 6 for n in nxc) >= 3          # both x-table branches
    origins = [(0, 0, 0), (1, 1, 600), (0, 0, 100), (1, 0, 0), (0, 3, 700), (0, 2, 450)]
    src_blocks = _block_table(origins, ins, strides)
    mm = np.empty((nb, 2))
    mm[:, 0], mm[:, 1] = np.inf, -np.inf
    d_mm = torch.from_numpy(mm).to(gpu)
    d_src = bl._to_device_bytes(src_blocks, gpu)
    nat.check(nat.lib().mmx_minmax_batch(ctypes.byref(src), d_src.data_ptr(), src_blocks.ctypes.data, nb,
                                         d_mm.data_ptr(), stream_ptr()), "mmx_minmax_batch")
    tabs_i, tabs_w, rb, at = [], [], np.zeros(nb, dtype=nat.RESIZE_DTYPE), 0
    for i, (o, si, so) in enumerate(zip(origins, ins, outs)):
        t3 = []
        for a in range(3):
            ix, w = preprocess.zoom_axis_table(si[a], so[a], "mirror")
            tabs_i.append(ix)
            tabs_w.append(w)
            t3.append(at)
            at += len(ix)
        rb[i] = (src_blocks["src_off"][i], *si, *so, i, *t3)
    d_idx = torch.from_numpy(np.concatenate(tabs_i).reshape(-1)).to(gpu)
    d_wts = torch.from_numpy(np.concatenate(tabs_w).reshape(-1)).to(gpu)
    d_rb = bl._to_device_bytes(rb, gpu)
    sy = -(-max(o[2] for o in outs) // 32) * 32
    sz = sy * max(o[1] for o in outs)
    slot = sz * max(o[0] for o in outs)
    # (uint16 results land in an int16 tensor of the same bytes)
    tdt = {np.uint8: torch.uint8, np.uint16: torch.int16, np.float32: torch.float32, np.float64: torch.float64}[dtype]
    out = torch.zeros(nb * slot, dtype=tdt, device=gpu)
    out32 = torch.zeros(nb * slot, dtype=torch.float32, device=gpu) if dtype == np.float64 else None
    nat.check(nat.lib().mmx_resize_batch_as(ctypes.byref(src), d_rb.data_ptr(), rb.ctypes.data, nb, d_idx.data_ptr(),
                                            d_wts.data_ptr(), d_mm.data_ptr(), slot, sy, sz, int(src.dtype),
                                            out.data_ptr(), None if out32 is None else out32.data_ptr(), stream_ptr()),
              "mmx_resize_batch_as")
    mm_got = d_mm.cpu().numpy()
    res = out.cpu().numpy().view(dtype).reshape(nb, -1)
    res32 = None if out32 is None else out32.cpu().numpy().reshape(nb, -1)
    for i, (o, si, so) in enumerate(zip(origins, ins, outs)):
        sub = vol[o[0]:o[0] + si[0], o[1]:o[1] + si[1], o[2]:o[2] + si[2]]
        np.testing.assert_array_equal(mm_got[i], [float(sub.min()), float(sub.max())])
        img = sub if dtype == np.float32 else sub.astype(np.float64)
        want = ndi.zoom(img, [b / a for a, b in zip(si, so)], order=1, mode="mirror", grid_mode=True)
        assert want.shape == so
        want = np.clip(want, sub.min(), sub.max()).astype(dtype)
        got = res[i, :so[0] * sz].reshape(so[0], -1)[:, :so[1] * sy].reshape(so[0], so[1], sy)[..., :so[2]]
        np.testing.assert_array_equal(got, want, err_msg=str((si, so)))
        if res32 is not None:
            g32 = res32[i, :so[0] * sz].reshape(so[0], -1)[:, :so[1] * sy].reshape(so[0], so[1], sy)[..., :so[2]]
            np.testing.assert_array_equal(g32, want.astype(np.float32))


@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64], ids=["u16", "f32", "f64"])
def test_gauss_axis_short_lines_mirror_and_nearest(gpu, dtype):
    """``mmx_gauss_axis_batch`` along each axis on lines of length 1, 2 and 3 with radii at or above the length
    ('mirror' then wraps with period 2n - 2 several times; n = 1 repeats its one sample), all blocks mirrored, all
    'nearest', and per block (mode 2: ``_pad`` bit 0) in one batch; against ``scipy.ndimage.correlate1d`` bit for bit
    (a float32 image filtered into float32, as SciPy does)."""
    from scipy import ndimage as ndi
    from magellanmapper_amd import _native as nat, blob_log as bl, kernels1d as k1
    rng = np.random.default_rng(23)
    vol = as_dtype(rng.integers(0, 65536, (12, 14, 140)).astype(np.uint16), dtype)
    dvol = bl.DeviceVolume(vol)
    src = dvol.view(0, False)
    strides = (src.stride_z, src.stride_y, src.stride_x)
    lengths, radii = (1, 2, 3, 3), np.array([4, 5, 7, 3], dtype=np.int32)
    others = [(5, 70), (4, 65), (6, 130), (3, 64)]
    pad = [0, 1, 0, 1]
    sigmas = [1.1, 1.3, 1.8, 0.8]
    pitch = int(radii.max()) + 1
    wts = np.zeros((len(radii), pitch))
    for i, (s, r) in enumerate(zip(sigmas, radii)):
        assert k1.kernel_radius(s) == r and r >= lengths[i]
        wts[i, :r + 1] = k1.gaussian_half_kernel(s, 0, int(r))
    d_w = torch.from_numpy(wts.reshape(-1)).to(gpu)
    d_r = torch.from_numpy(radii).to(gpu)
    out_t = torch.float32 if dtype == np.float32 else torch.float64
    for axis in range(3):
        shapes = []
        for n, (p, q) in zip(lengths, others):
            s = [p, q]
            s.insert(axis, n)
            s = tuple(min(v, lim) for v, lim in zip(s, vol.shape))
            shapes.append(s)
        origins = [tuple(int(rng.integers(0, f - v + 1)) for f, v in zip(vol.shape, s)) for s in shapes]
        for nearest in (0, 1, 2):
            blocks = _block_table(origins, shapes, strides, pad)
            d_blocks = bl._to_device_bytes(blocks, gpu)
            sy = -(-max(s[2] for s in shapes) // 32) * 32
            sz = sy * max(s[1] for s in shapes)
            slot = sz * max(s[0] for s in shapes)
            out = torch.zeros(len(shapes) * slot, dtype=out_t, device=gpu)
            nat.check(nat.lib().mmx_gauss_axis_batch(ctypes.byref(src), d_blocks.data_ptr(), blocks.ctypes.data,
                                                     len(shapes), axis, d_w.data_ptr(), d_r.data_ptr(), pitch, nearest,
                                                     slot, sy, sz, out.data_ptr(), stream_ptr()), "mmx_gauss_axis_batch")
            res = out.cpu().numpy().reshape(len(shapes), -1)
            for i, (o, s) in enumerate(zip(origins, shapes)):
                assert s[axis] == lengths[i]
                sub = vol[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]]
                img = sub if dtype == np.float32 else sub.astype(np.float64)
                full = np.concatenate((wts[i, 1:radii[i] + 1][::-1], wts[i, :radii[i] + 1]))
                mode = "nearest" if nearest == 1 or (nearest == 2 and pad[i]) else "mirror"
                want = ndi.correlate1d(img, full, axis=axis, mode=mode)
                got = res[i, :s[0] * sz].reshape(s[0], -1)[:, :s[1] * sy].reshape(s[0], s[1], sy)[..., :s[2]]
                assert want.dtype == got.dtype
                np.testing.assert_array_equal(got, want, err_msg=str((axis, nearest, s, mode)))


def test_minmax_extremes_at_the_last_row_and_column_of_channel_views(gpu):
    """``mmx_minmax_batch`` on the channels of a (z, y, x, c) image (x stride = channels): the block's minimum or
    maximum sits in its last row (last z, last y) and last column only, for row lengths around the kernel's 64 / 128
    column steps and row counts that leave a wave with one row; bit-equal to NumPy."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    rng = np.random.default_rng(29)
    img = rng.integers(1000, 60000, (9, 11, 300, 3)).astype(np.uint16)
    # (disjoint blocks: each one's extreme is its own)
    origins = [(0, 0, 0), (4, 0, 0), (0, 5, 0), (0, 5, 70), (0, 0, 299), (4, 0, 131)]
    shapes = [(4, 5, 130), (5, 11, 129), (4, 6, 65), (4, 6, 128), (9, 11, 1), (5, 11, 168)]
    for c in range(3):
        for b, (o, s) in enumerate(zip(origins, shapes)):
            last = (o[0] + s[0] - 1, o[1] + s[1] - 1, o[2] + s[2] - 1, c)
            img[last] = 65535 - 7 * b - c if (b + c) % 2 else 3 * b + c
    dvol = bl.DeviceVolume(img)
    for c in range(3):
        v = dvol.view(c, False)
        assert v.stride_x == 3
        blocks = _block_table(origins, shapes, (v.stride_z, v.stride_y, v.stride_x))
        mm = np.empty((len(shapes), 2))
        mm[:, 0], mm[:, 1] = np.inf, -np.inf
        d_mm = torch.from_numpy(mm).to(gpu)
        d_blocks = bl._to_device_bytes(blocks, gpu)
        nat.check(nat.lib().mmx_minmax_batch(ctypes.byref(v), d_blocks.data_ptr(), blocks.ctypes.data, len(shapes),
                                             d_mm.data_ptr(), stream_ptr()), "mmx_minmax_batch")
        got = d_mm.cpu().numpy()
        for b, (o, s) in enumerate(zip(origins, shapes)):
            sub = img[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2], c]
            np.testing.assert_array_equal(got[b], [float(sub.min()), float(sub.max())], err_msg=str((c, b)))
            assert sub[-1, -1, -1] in (sub.min(), sub.max())


# ---------------------------------------------------------------- 6. cdist and close pairs
def test_cdist_row_limit_and_chunked_rows(gpu, monkeypatch):
    """``mmx_cdist_f64`` takes 65535 rows and refuses 65536 (``MMX_ERR_UNSUPPORTED``); ``verifier._cdist`` cuts
    70 000 rows into launches of 32768 and the seams change nothing: bit-equal to ``scipy.spatial.distance.cdist``
    for points of 3 and of 11 coordinates (tied and zero distances included)."""
    from scipy.spatial import distance
    from magellanmapper_amd import _native as nat, verifier
    L = nat.lib()
    rng = np.random.default_rng(31)
    a = rng.random((65536, 3)) * 300
    b = rng.random((5, 3)) * 300
    d_a, d_b = torch.from_numpy(a).to(gpu), torch.from_numpy(b).to(gpu)
    d_out = torch.full((65536 * 5,), -1.0, dtype=torch.float64, device=gpu)
    nat.check(L.mmx_cdist_f64(d_a.data_ptr(), 65535, d_b.data_ptr(), 5, 3, d_out.data_ptr(), stream_ptr()), "mmx_cdist_f64")
    got = d_out.cpu().numpy().reshape(-1, 5)
    np.testing.assert_array_equal(got[:65535], distance.cdist(a[:65535], b))
    assert (got[65535] == -1.0).all()
    assert L.mmx_cdist_f64(d_a.data_ptr(), 65536, d_b.data_ptr(), 5, 3, d_out.data_ptr(), stream_ptr()) == 5
    torch.cuda.synchronize()
    real = L.mmx_cdist_f64
    rows = []

    def counting(*args):
        rows.append(int(args[1]))
        return real(*args)

    monkeypatch.setattr(L, "mmx_cdist_f64", counting)
    for dim in (3, 11):
        a = np.round(rng.random((70000, dim)) * 200, 1)
        b = np.round(rng.random((9, dim)) * 200, 1)
        a[32767:32770] = b[2]                          # zero distances on both sides of the first seam
        a[65535:65537] = b[:2]
        rows.clear()
        got = verifier._cdist(a, b)
        assert rows == [32768, 32768, 70000 - 65536]
        np.testing.assert_array_equal(got, distance.cdist(a, b), err_msg=str(dim))


def _close_ref(master, check, tol):
    last = np.full(len(master), -1, dtype=np.int32)
    hit = np.zeros(len(check), dtype=np.uint8)
    for m, row in enumerate(master):
        match = np.flatnonzero((np.abs(check - row) <= tol).all(axis=1))
        if len(match):
            last[m] = match[-1]
            hit[match] = 1
    return last, hit


def _close_call(master, check, tol, dev):
    from magellanmapper_amd import _native as nat
    d_m = torch.from_numpy(np.ascontiguousarray(master, dtype=np.int32)).to(dev)
    d_c = torch.from_numpy(np.ascontiguousarray(check if len(check) else np.zeros((1, 3)), dtype=np.int32)).to(dev)
    d_last = torch.full((max(1, len(master)),), -5, dtype=torch.int32, device=dev)
    d_hit = torch.full((max(1, len(check)),), 9, dtype=torch.uint8, device=dev)
    t = np.ascontiguousarray(tol, dtype=np.int32)
    nat.check(nat.lib().mmx_close_pairs(d_m.data_ptr(), len(master), d_c.data_ptr(), len(check), nat.as_int32_ptr(t),
                                        d_last.data_ptr(), d_hit.data_ptr(), stream_ptr()), "mmx_close_pairs")
    return d_last.cpu().numpy()[:len(master)], d_hit.cpu().numpy()


def test_close_pairs_last_match_across_check_tiles(gpu):
    """``mmx_close_pairs`` against a brute-force loop: 845 check rows (three full tiles of 256 and a ragged one), a
    master row matching rows in the first, second and last tile -- the last one wins, as NumPy's fancy assignment
    gives --, master counts that are not multiples of 256, zero tolerances, and an empty check table."""
    rng = np.random.default_rng(37)
    check = rng.integers(0, 40, (845, 3)).astype(np.int32)
    master = rng.integers(0, 40, (300, 3)).astype(np.int32)
    master[0] = (100, 100, 100)
    for r, d in ((5, (0, 0, 0)), (300, (1, -1, 2)), (600, (0, 2, 0)), (840, (-2, 0, 1))):
        check[r] = master[0] + np.array(d, dtype=np.int32)
    check[844], check[255] = (300, 300, 300), (200, 200, 200)      # rows no other row is near
    master[299] = check[844]
    master[150] = check[255]
    for tol in ((2, 1, 2), (2, 2, 2), (0, 0, 0), (3, 0, 5)):
        tol = np.array(tol, dtype=np.int32)
        last, hit = _close_call(master, check, tol, gpu)
        want_last, want_hit = _close_ref(master, check, tol)
        np.testing.assert_array_equal(last, want_last, err_msg=str(tol))
        np.testing.assert_array_equal(hit, want_hit, err_msg=str(tol))
        if tol.min() > 0:
            assert want_last[0] == 840 and len(set(np.flatnonzero((np.abs(check - master[0]) <= tol).all(1)) // 256)) >= 3
        if not tol.any():
            assert want_last[299] == 844 and want_last[150] == 255
    last, hit = _close_call(master[:77], np.zeros((0, 3), dtype=np.int32), np.array([2, 2, 2]), gpu)
    np.testing.assert_array_equal(last, np.full(77, -1))
