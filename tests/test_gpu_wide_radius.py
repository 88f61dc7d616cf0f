"""GPU tests of the wide passes (``csrc/mmx_wide.hip``, ``MMX_ZX_WIDE``): kernel radii 25 .. 64 on blocks whose every
extent is at least the radius -- the cube at the edges of that geometry, the fall-back one voxel short of it, the passes
by name at small radii, the row entries of the Y pass, the one-round ladder rule of ``mmx_log_scales_f32`` and the tables
of ``blob_log`` / ``detect_blobs_blocks`` at a fine resolution.  Float64 references come from ``oracle/`` and are computed
once per input.  Needs a real MI355X (``-m gpu``)."""
import numpy as np
import pytest

from gpu_support import as_dtype, gpu, ladder_run, timed_cubes  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LOG_TOL = 1e-4
#: the bound the large-radius test of test_gpu_kernel_edges.py holds the generic float32 passes to
CUBE_TOL = LOG_TOL * 1e-2


DTYPES = [np.uint8, np.uint16, np.float32, np.float64]
DTYPE_IDS = ["u8", "u16", "f32", "f64"]
WIDE_RADII = (25, 31, 48, 64)


def _odd(n):
    """The next odd number: no multiple of 16 or 64."""
    return n | 1


def _edge_blocks(R, short_axis=None):
    """The batch at the edges of the wide geometry: one block exactly R thick along each axis (the other extents odd),
    one with rows wider than 512, one at a non-zero origin.  ``short_axis``: the first block is one voxel short of R
    along that axis instead."""
    shapes = [(R, _odd(R + 6), _odd(R + 10)), (_odd(R + 4), R, _odd(R + 8)), (_odd(R + 2), _odd(R + 6), R),
              (R + 2, R + 2, 530), (_odd(R + 2), _odd(R + 4), _odd(R + 6))]
    origins = [(0, 0, 0), (1, 2, 3), (2, 0, 5), (0, 1, 7), (3, 5, 9)]
    if short_axis is not None:
        s = list(shapes[short_axis])
        s[short_axis] = R - 1
        shapes[short_axis] = tuple(s)
    return origins, shapes


@pytest.fixture(scope="module")
def edge_volume():
    from magellanmapper_amd import synth
    return synth.make_volume(303, (80, 84, 540), 30, blob_sigma=7.0)


_REFERENCE = {}


def _reference(vol, kind, R, origins, shapes, tag=""):
    """float64 cubes of the blocks at sigma = (R + 0.2) / 4, once per (input, radius): uint16 and float64 voxels are the
    same float64 image (v / 65535), so they share theirs."""
    from oracle import blob_log_oracle as blo
    key = (kind, R, tag)
    if key not in _REFERENCE:
        sigma = (R + 0.2) / 4.0
        _REFERENCE[key] = [blo.log_cube(blo.img_as_float(vol[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]]),
                                        np.array([[sigma] * 3]))[..., 0] for o, s in zip(origins, shapes)]
    return _REFERENCE[key]


def _kind_of(dtype):
    return "u16" if dtype in (np.uint16, np.float64) else np.dtype(dtype).name


# ---------------------------------------------------------------- 1. the cube at the edges of the geometry
@pytest.mark.parametrize("R", WIDE_RADII)
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_cube_at_the_edges_of_the_wide_geometry(gpu, edge_volume, dtype, R):
    """Radii 25 .. 64 under MMX_ZX_AUTO on blocks exactly R thick along one axis, on rows wider than 512 and at a
    non-zero origin: three wide passes, no generic one, the cube within the generic float32 passes' bound of the float64
    oracle and within the float32 paths' agreement of the generic passes."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    vol = as_dtype(edge_volume, dtype)
    origins, shapes = _edge_blocks(R)
    for a in range(3):
        assert shapes[a][a] == R and all(s[i] % 2 == 1 for i, s in enumerate([shapes[a]] * 3) if i != a)
    assert shapes[3][2] > 512 and any(origins[4])
    dvol = bl.DeviceVolume(vol)
    sigma = (R + 0.2) / 4.0
    space = bl.ScaleSpace.make(sigma, sigma, 1)
    assert space.radii[0] == R
    want = _reference(vol, _kind_of(dtype), R, origins, shapes)
    got, kinds = timed_cubes(dvol, origins, shapes, space)
    assert kinds["widepass"][1] == 3 and kinds["generic"][1] == 0, kinds
    assert all(kinds[k][1] == 0 for k in ("zpass", "ypass", "xpass", "zxpass", "y2pass", "zxpack"))
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_WIDE
    gen = bl.log_cube_blocks(dvol, 0, origins, shapes, space, generic=True)
    for shp, g, ref, ge in zip(shapes, got, want, gen):
        err = np.abs(g[..., 0] - ref).max()
        dev = np.abs(g[..., 0] - ge[..., 0]).max()
        print("R %d %s block %s: |wide - oracle| %.3g, |wide - generic| %.3g" % (R, np.dtype(dtype).name, shp, err, dev))
        assert g.shape[:3] == shp and err < CUBE_TOL, (R, shp, err)
        assert dev < 2e-6 * max(1.0, np.abs(ref).max()), (R, shp, dev)


# ---------------------------------------------------------------- 2. one voxel short
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_voxel_short_of_the_radius_takes_the_generic_passes(gpu, edge_volume, axis):
    """The same batch with one block of extent R - 1 along one axis: the whole call is the three generic passes."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    R = 31
    origins, shapes = _edge_blocks(R, short_axis=axis)
    assert min(min(s) for s in shapes) == R - 1
    dvol = bl.DeviceVolume(edge_volume)
    sigma = (R + 0.2) / 4.0
    space = bl.ScaleSpace.make(sigma, sigma, 1)
    want = _reference(edge_volume, "u16", R, origins, shapes, tag="short%d" % axis)
    got, kinds = timed_cubes(dvol, origins, shapes, space)
    assert kinds["generic"][1] == 3 and kinds["widepass"][1] == 0, kinds
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_SEPARATE
    for shp, g, ref in zip(shapes, got, want):
        err = np.abs(g[..., 0] - ref).max()
        assert g.shape[:3] == shp and err < CUBE_TOL, (shp, err)


# ---------------------------------------------------------------- 3. by name at small radii
@pytest.mark.parametrize("shape", [(20, 26, 40), (24, 26, 40)], ids=["20x26x40", "24x26x40"])
@pytest.mark.parametrize("R", [1, 8, 24])
def test_wide_passes_by_name_at_small_radii(gpu, monkeypatch, R, shape):
    """MMX_ZX_WIDE by name takes any radius from 1 that the block's extents cover, and agrees with the separate passes
    as the float32 paths agree with each other.  The 20-voxel block is thinner than radius 24: the call then goes on to
    the paths it would take without the name (the second block is there for radius 24 to run the wide passes)."""
    from magellanmapper_amd import _native as nat, blob_log as bl, synth
    vol = synth.make_volume(77, (26, 30, 44), 5, blob_sigma=3.0)
    origins, shapes = [(1, 2, 3)], [shape]
    dvol = bl.DeviceVolume(vol)
    sigma = (R + 0.2) / 4.0
    space = bl.ScaleSpace.make(sigma, sigma, 1)
    assert space.radii[0] == R
    monkeypatch.setattr(bl, "ZX_MODE", nat.MMX_ZX_WIDE)
    wide, kinds = timed_cubes(dvol, origins, shapes, space)
    path = bl.LAST_ZX_PATH
    monkeypatch.setattr(bl, "ZX_MODE", nat.MMX_ZX_SEPARATE)
    sep = bl.log_cube_blocks(dvol, 0, origins, shapes, space)
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_SEPARATE
    if min(shape) >= R:
        assert path == nat.MMX_ZX_WIDE and kinds["widepass"][1] == 3, (path, kinds)
    else:
        assert path != nat.MMX_ZX_WIDE and kinds["widepass"][1] == 0, (path, kinds)
    dev = np.abs(wide[0] - sep[0]).max()
    assert dev < 2e-6 * max(1.0, np.abs(sep[0]).max()), dev


# ---------------------------------------------------------------- 4. entries
ENTRY_SHAPE, ENTRY_R = (34, 40, 70), 31


def _entry_case():
    """The block, its float64 cube and a threshold that leaves 64-voxel segments of both kinds."""
    from magellanmapper_amd import synth
    from oracle import blob_log_oracle as blo
    if "entries" not in _REFERENCE:
        vol = synth.make_volume(11, ENTRY_SHAPE, 3, blob_sigma=7.0)
        sigma = (ENTRY_R + 0.2) / 4.0
        cube = blo.log_cube(blo.img_as_float(vol), np.array([[sigma] * 3]))[..., 0]
        _REFERENCE["entries"] = (vol, cube, float(0.5 * (cube.max() + np.median(cube))))
    return _REFERENCE["entries"]


def test_entry_case_has_segments_of_both_kinds():
    """(CPU) the threshold of the entries test splits the oracle cube's 64-voxel segments into both kinds."""
    _, cube, lo = _entry_case()
    nz, ny, nx = cube.shape
    px = -(-nx // 32) * 32
    flat = np.full((ny, nz, px), -np.inf)
    flat[:, :, :nx] = np.moveaxis(cube, 1, 0)
    flat = flat.reshape(ny, nz * px)
    pad = -flat.shape[1] % 64
    seg = np.pad(flat, ((0, 0), (0, pad)), constant_values=-np.inf).reshape(ny, -1, 64)
    above = (seg > lo).any(axis=2)
    assert above.any() and (~above).any()
    assert above.sum() > 20 and (~above).sum() > 20


def test_row_entries_and_unwritten_segments_of_the_wide_y_pass(gpu):
    """``mmx_log_batch_f32`` in wide mode with entries on a NaN-filled ``d_log``: the layout is MMX_MASK_ROWS, word 1 is
    ``cube > nms_lo`` (voxels within the float32 bound of the threshold aside), every local maximum of the oracle above
    the threshold has its word-0 bit, written segments hold the values and the others still hold NaN."""
    from scipy import ndimage
    from magellanmapper_amd import _native as nat
    from magellanmapper_amd.rawbatch import RawBatch
    vol, cube, lo = _entry_case()
    nz, ny, nx = ENTRY_SHAPE
    sigma = (ENTRY_R + 0.2) / 4.0
    eps = 2e-5
    b = RawBatch(vol, [(0, 0, 0)], [ENTRY_SHAPE], (sigma, sigma, 1), lo, eps, 0)
    assert b.space.radii[0] == ENTRY_R
    px, slot, ws = int(b.blocks["px"][0]), b.slot, b.ws
    off = (b.log_base - ws.data_ptr()) // 4
    d_log = ws[off:off + slot]
    d_log.fill_(float("nan"))
    mask_base = b.entries_base
    n_entries = slot >> 5
    path, written = b.log_batch(0, nat.MMX_ZX_WIDE, lo, eps, entries=True)
    torch.cuda.synchronize()
    assert written == nat.MMX_MASK_ROWS and path == nat.MMX_ZX_WIDE
    off = (mask_base - ws.data_ptr()) // 4
    words = ws[off:off + n_entries * 4].cpu().numpy().view(np.uint64).reshape(-1, 2)
    log = d_log.cpu().numpy()[:nz * ny * px].reshape(nz, ny, px)
    ncol = nz * px
    nwords = (ncol + 63) >> 6
    assert ny * nwords <= n_entries
    bits = ((words[:ny * nwords, :, None] >> np.arange(64, dtype=np.uint64)[None, None, :]) & np.uint64(1)).astype(bool)
    # [y][word][which][bit] -> [which][y][c] -> [which][z][y][x]
    by_col = np.moveaxis(bits.reshape(ny, nwords, 2, 64), 2, 0).reshape(2, ny, nwords * 64)[:, :, :ncol]
    grid = np.moveaxis(by_col.reshape(2, ny, nz, px), 1, 2)
    cand, above = grid[0], grid[1]
    assert not above[:, :, nx:].any() and not cand[:, :, nx:].any()          # (pitch columns carry no bits)
    cand, above = cand[:, :, :nx], above[:, :, :nx]
    want_above = cube > lo
    sure = np.abs(cube - lo) > CUBE_TOL
    assert sure.mean() > 0.99
    np.testing.assert_array_equal(above[sure], want_above[sure])
    assert not (cand & ~above).any()
    peaks = (cube == ndimage.maximum_filter(cube, size=3, mode="constant", cval=-np.inf)) & (cube > lo + CUBE_TOL)
    assert peaks.sum() >= 1
    assert cand[peaks].all()
    # the segments: 64 columns of a row; with a bit -> values, without -> untouched
    seg_on = by_col[1].reshape(ny, nwords, 64).any(axis=2)                  # [y][word]
    assert seg_on.any() and (~seg_on).any()
    col_on = np.repeat(seg_on, 64, axis=1)[:, :ncol]                         # [y][c]
    vox_on = np.moveaxis(col_on.reshape(ny, nz, px), 0, 1)                   # [z][y][px]
    assert np.isnan(log[~vox_on]).all()
    inside = vox_on[:, :, :nx]
    err = np.abs(log[:, :, :nx][inside] - cube[inside]).max()
    print("written segments: %d of %d, |wide - oracle| %.3g" % (seg_on.sum(), seg_on.size, err))
    assert err < CUBE_TOL


# ---------------------------------------------------------------- 5. the ladder rule
@pytest.fixture(scope="module")
def ladder_volume():
    from magellanmapper_amd import synth
    return synth.make_volume(19, (40, 48, 540), 24, blob_sigma=6.3)


@pytest.mark.parametrize("width", [64, 530])
def test_a_ladder_with_wide_radii_is_one_round_with_row_entries(gpu, ladder_volume, width):
    """Radii {24, 25, 26} on a uint16 block of 40 x 48 x 64: laid out before the first launch -- one round, row entries,
    the last scale wide -- and the re-scored candidates are those nominated from the full cube of the same kernels.
    On rows 530 wide the radius-24 scale goes wide too."""
    from magellanmapper_amd import _native as nat
    from magellanmapper_amd.rawbatch import timed
    origin, shape = (0, 0, 5), (40, 48, width)
    info, cands, space = ladder_run(ladder_volume, origin, shape, 6.05, 6.55, 3)
    assert [int(r) for r in space.radii] == [24, 25, 26]
    assert (info.n_pass_rounds, info.mask_layout, info.zx_path) == (1, nat.MMX_MASK_ROWS, nat.MMX_ZX_WIDE)
    modes = [nat.MMX_ZX_PACKED if width <= 320 else nat.MMX_ZX_WIDE, nat.MMX_ZX_WIDE, nat.MMX_ZX_WIDE]
    _, dense, _ = ladder_run(ladder_volume, origin, shape, 6.05, 6.55, 3, by_name=modes)
    assert len(dense) > 0 and len(cands) == len(dense)
    for f in ("slot", "s", "z", "y", "x", "v", "v64"):
        np.testing.assert_array_equal(cands[f], dense[f], err_msg=f)
    # the kinds that ran: three wide passes per wide scale, the packed Z+X and Y kernels for the other
    _, kinds = timed(lambda: ladder_run(ladder_volume, origin, shape, 6.05, 6.55, 3))
    n_wide = modes.count(nat.MMX_ZX_WIDE)
    # (mmx_log_scales_f32 and mmx_detect_batch each ran the ladder once)
    assert kinds["widepass"][1] == 2 * 3 * n_wide and kinds["generic"][1] == 0, kinds
    assert kinds["zxpass"][1] == kinds["y2pass"][1] == 2 * (3 - n_wide) and kinds["zxpack"][1] == 0, kinds


def test_a_ladder_without_wide_radii_runs_what_it_ran(gpu, ladder_volume):
    """Radii {20, 24} only: the report is the one of the register-resident paths -- 16-bit tiles, quads, one round."""
    from magellanmapper_amd import _native as nat
    info, cands, space = ladder_run(ladder_volume, (0, 0, 5), (40, 48, 64), 5.0, 6.0, 2)
    assert [int(r) for r in space.radii] == [20, 24]
    assert (info.n_pass_rounds, info.mask_layout, info.zx_path) == (1, nat.MMX_MASK_QUADS, nat.MMX_ZX_TILED_Q16)
    assert len(cands) > 0


# ---------------------------------------------------------------- 6. tables
def test_blob_log_at_wide_radii_matches_the_oracle_row_for_row(gpu):
    """sigma 5.5 .. 7.5 in five steps (radii 22 .. 30) on a volume every extent of which covers them."""
    from magellanmapper_amd import _native as nat, blob_log as bl, synth
    from oracle import blob_log_oracle as blo
    vol = synth.make_volume(23, (48, 56, 60), 6, blob_sigma=7)
    want = blo.blob_log(vol, 5.5, 7.5, 5, 0.05, 0.5)
    got = bl.blob_log(vol, 5.5, 7.5, 5, 0.05, 0.5)
    assert len(want) > 0
    np.testing.assert_array_equal(got, want)
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_WIDE
    assert (bl.LAST_PASS_ROUNDS, bl.LAST_MASK_LAYOUT) == (1, nat.MMX_MASK_ROWS)


def test_stack_detection_at_fine_resolution_matches_the_oracle(gpu):
    """A stack at 0.65 um / px with the stock factors 3 .. 5 in four scales (sigma 4.6 .. 7.7 px, radii 18 .. 31) and
    segment_size 40: blocks of 62 + 8 px, every one at least 31 voxels thick; the final table equals the oracle's, and
    every batch took one round with row entries."""
    from magellanmapper_amd import _native as nat, blob_log as bl, config, stack_detect, synth
    from oracle import magmap_oracle as mmo
    vol = synth.make_volume(29, (40, 96, 100), 12, blob_sigma=6.0)
    saved = (config.resolutions, config.filename)
    try:
        config.resolutions = np.array([[0.65] * 3])
        config.filename = "fine"
        config.setup_roi_profiles(None)
        config.roi_profile.update(dict(min_sigma_factor=3, max_sigma_factor=5, num_sigma=4, segment_size=40,
                                       denoise_size=None))
        prof = dict(config.roi_profile)
        blocks = mmo.setup_blocks(prof, vol.shape, config.resolutions)
        shapes = [mmo._slice_shape(s, vol.shape) for s in blocks["sub_roi_slices"].ravel()]
        assert len(shapes) == 4 and min(min(s) for s in shapes) >= 31 and max(max(s) for s in shapes) == 70
        _, _, blobs = stack_detect.detect_blobs_blocks("fine", stack_detect.Image5d(vol[None]), None, None, None,
                                                       False, False, True, False)
        want, _ = mmo.detect_blobs_blocks(vol, None, [prof], config.resolutions)
    finally:
        config.resolutions, config.filename = saved
        config.setup_roi_profiles(None)
    got = blobs.blobs

    def canon(t):
        return t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]
    assert want is not None and len(want) > 0 and got is not None
    assert got.shape == want.shape
    np.testing.assert_array_equal(canon(got), canon(want))
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_WIDE
    assert (bl.LAST_PASS_ROUNDS, bl.LAST_MASK_LAYOUT) == (1, nat.MMX_MASK_ROWS)
