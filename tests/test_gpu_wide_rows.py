"""GPU tests of the tiled matrix-core path on rows wider than 512 voxels (one panel of its voxel copy): the cube of every
geometry class and voxel type against the float64 oracle at widths around the panel seams, the resolved peaks against
the separate passes and the oracle, the rules that did not move, and a stack whose blocks are 565 and 540 voxels wide.
The volumes, and the proof that the oracle has peaks on both sides of every seam, are in tests/test_wide_rows_host.py.
Needs a real MI355X (``-m gpu``).

The slot of a batch.  The tiled path keeps its tiles, tables and voxel copy in the four intermediate arrays of the
workspace (4 x slot_elems floats per block), and z tiles are 16 planes deep: a block of 20 planes pays for 32.  With the
slot ``blob_log`` gives a block -- nz ny px, nothing to spare when px is the row itself -- the 20-plane blocks below do
not fit (513 wide, uint16: 4 337 664 bytes of plan against 4 177 920) and the library routes them to the separate
passes, as it must.  ``slot_elems`` is the caller's to choose, so where the ABI is driven directly (the cube test) a
batch gets the larger of that slot and the one its plan needs (``_tiled_slot``: the arithmetic of
``mmx_zx6_plan_make``), which is what puts these widths on the tiled kernels at all; through ``blob_log_blocks`` the path
of each case is the one that arithmetic predicts (the 513 voxels wide block of 26 planes is there for the tiled path to
meet an odd number of column tiles through ``blob_log_blocks`` as well)."""
import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401
from test_wide_rows_host import (CASES, OVERLAP, SIGMAS, STACK_BLOCKS, STACK_SEGMENT, STACK_SIGMAS, THRESHOLD, block_image,
                                 oracle_peaks, stack_volume, volume)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LOG_TOL = 1e-4
F32_TILE_TOL = LOG_TOL * 1e-2           # float32 tiles against the float64 oracle (test_gpu_parity.py, every radius)
FAMILIES = ("zpass", "ypass", "xpass", "generic", "zxpass", "y2pass", "zxpack", "widepass")
#: one radius per compiled geometry class of the Z+X kernel (<= 8, <= 16, <= 24) and, at 12 and 16, the form with two
#: column tiles per wave on an odd (513 -> 33) and an even (530 -> 34) number of column tiles
RADII = (8, 12, 16, 17, 24)
KINDS = ("u8", "u16", "f32")


def _voxels(vol16, kind):
    if kind == "u16":
        return vol16
    if kind == "u8":
        return (vol16 >> 8).astype(np.uint8)
    return (vol16 / 65535.0).astype(np.float32)


def _radii_of(shape):
    """Radius 24 only where the fused path takes it: nz >= 25, ny >= 28."""
    return [r for r in RADII if r < 24 or (shape[0] >= 25 and shape[1] >= 28)]


def _plan_bytes(shapes, pieces):
    """What the tiled path needs of a batch's four intermediate arrays (``mmx_zx6_plan_make``): float32 tiles of P and
    of Q, the Toeplitz tables, the voxel copy (``pieces``: 2 for float voxels)."""
    ntx, ntz = [-(-s[2] // 16) for s in shapes], [-(-s[0] // 16) for s in shapes]
    tile = max(tx * tz * s[1] * 256 for s, tx, tz in zip(shapes, ntx, ntz))
    pack = max(s[1] * tz * -(-s[2] // 8) * 128 * pieces for s, tz in zip(shapes, ntz))
    ncw, ncz = len({s[2] for s in shapes}), len({s[0] for s in shapes})
    tab = (ncw * max(ntx) * 2 * 2 + ncz * max(ntz) * 3 * 2) * 2 * 64 * 16
    n = len(shapes)
    return -(-(2 * n * tile * 4 + tab) // 256) * 256 + n * pack * 2


def _blob_log_slot(shapes):
    return max(s[0] * s[1] * (-(-s[2] // 32) * 32) for s in shapes)


def _plan_fits(shapes, pieces):
    return _plan_bytes(shapes, pieces) <= 16 * len(shapes) * _blob_log_slot(shapes)


def _tiled_slot(shapes, pieces):
    need = -(-_plan_bytes(shapes, pieces) // (16 * len(shapes)))
    return max(_blob_log_slot(shapes), -(-need // 32) * 32)


_REFERENCE = {}


def _reference(name, i, kind, R):
    """The float64 cube of block ``i`` of a case at sigma = (R + 0.2) / 4, once per voxel type: of the very voxels the
    GPU gets (float32 voxels as they are, in float64 arithmetic)."""
    from oracle import blob_log_oracle as blo
    key = (name, i, kind, R)
    if key not in _REFERENCE:
        sigma = (R + 0.2) / 4.0
        img = blo.img_as_float(_voxels(block_image(name, i), kind)).astype(np.float64)
        _REFERENCE[key] = blo.log_cube(img, np.array([[sigma] * 3]))[..., 0]
    return _REFERENCE[key]


class _Batch:
    """One batch of a case on the device, driven through the ABI with a slot of this test's choosing."""

    def __init__(self, bl, name, kind):
        from magellanmapper_amd.rawbatch import RawBatch
        self.bl = bl
        shapes = [s for _, s in CASES[name][2]]
        self.raw = RawBatch(_voxels(volume(name), kind), [o for o, _ in CASES[name][2]], shapes, self.space(RADII[0]), 0.0,
                            0.0, 0, slot=_tiled_slot(shapes, 2 if kind == "f32" else 1),
                            value_range=1.0 if kind == "f32" else None, exact=0, expand=0)
        assert self.raw.blocks_slot == _blob_log_slot(shapes)
        self.shapes = shapes

    def space(self, R):
        sigma = (R + 0.2) / 4.0
        space = self.bl.ScaleSpace.make(sigma, sigma, 1)
        assert space.radii[0] == R
        return space

    def ladder_of_one(self, R, thr, eps):
        """``mmx_log_scales_f32`` of the one scale under MMX_ZX_AUTO (entries wanted) on a NaN-filled workspace: the
        report, the kernel families, the LoG arrays and, per block, which voxels the entries say were written."""
        from magellanmapper_amd import _native as nat
        from magellanmapper_amd.rawbatch import families, timed
        b = self.raw
        b.set_scales(self.space(R))
        a = b.args(thr=thr, eps=eps, d_cands=None, d_count=None)     # (no table, no counters: this entry has no tail)
        b.ws.fill_(float("nan"))
        info, kinds = timed(lambda: b.log_scales(a))
        torch.cuda.synchronize()
        logs = b.cubes(b.log_arrays()[0])
        written = b.quads_written() if info.mask_layout == nat.MMX_MASK_QUADS else None
        return info, families(kinds, FAMILIES), logs, written, b.space

    def by_name(self, R, mode):
        """``mmx_log_batch_f32`` in ``mode`` without entries: the whole cube."""
        b = self.raw
        b.set_scales(self.space(R))
        b.ws.fill_(float("nan"))
        path = b.log_batch(0, mode)
        torch.cuda.synchronize()
        return path, b.cubes(b.log_arrays()[0])


# ---------------------------------------------------------------- 1. the cube
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_cube_on_rows_wider_than_one_panel(gpu, name, kind):
    """Every radius class on every width around the panel seams, per voxel type.  Under MMX_ZX_AUTO with entries: the
    16-bit tiles, quad entries, one round, the voxel copy + Z+X + Y families and no other; the values within the
    library's own analytic bound of the oracle wherever the entries say they were written, NaN (untouched) elsewhere,
    and nothing above the threshold left unwritten.  MMX_ZX_TILED by name: the whole cube within the float32 tiles'
    tolerance."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    b = _Batch(bl, name, kind)
    eps = bl.EPS_REL_Q16
    both_kinds = False              # at the detection threshold, some radius leaves written and unwritten segments
    for R in _radii_of(min(b.shapes)):
        path, full = b.by_name(R, nat.MMX_ZX_TILED)
        assert path == nat.MMX_ZX_TILED
        # the detection threshold (entries and values around the blobs only), then one below every value: the whole cube
        for thr in (THRESHOLD, -1.0):
            info, fams, logs, written, space = b.ladder_of_one(R, thr, eps)
            print("%s %s R %d thr %g: path %d layout %d rounds %d families %s" % (
                name, kind, R, thr, info.zx_path, info.mask_layout, info.n_pass_rounds, fams))
            assert (info.zx_path, info.mask_layout, info.n_pass_rounds) == (nat.MMX_ZX_TILED_Q16, nat.MMX_MASK_QUADS, 1)
            assert fams == dict(zxpack=1, zxpass=1, y2pass=1)
            bound = space.q16_bound()                              # (value range 1 for all three voxel types)
            assert info.q16_bound == bound and bound > 0
            for i, (shp, log, on, f32) in enumerate(zip(b.shapes, logs, written, full)):
                want = _reference(name, i, kind, R)
                nx = shp[2]
                got = log[:, :, :nx]
                assert np.isnan(log[:, :, nx:]).all()              # (pitch columns are nobody's)
                np.testing.assert_array_equal(~np.isnan(got), on)
                if thr < 0:
                    assert on.all()
                elif i == 0:
                    both_kinds = both_kinds or (on.any() and not on.all())
                err = np.abs(got[on] - want[on]).max() if on.any() else 0.0
                # what was left out lies below the threshold of the entries, thr - eps, up to the bound
                missed = want[~on].max() if (~on).any() else -np.inf
                err32 = np.abs(f32[:, :, :nx] - want).max()
                print("  block %s: %d of %d voxels written, |q16 - oracle| %.3g (bound %.3g), |f32 tiles - oracle| %.3g"
                      % (shp, on.sum(), on.size, err, bound, err32))
                assert err < bound, (name, kind, R, shp, err, bound)
                assert missed <= thr - eps + bound, (name, kind, R, shp, missed)
                assert err32 < F32_TILE_TOL, (name, kind, R, shp, err32)
    assert both_kinds


# ---------------------------------------------------------------- 2. the peaks
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_peaks_equal_those_of_the_separate_passes(gpu, monkeypatch, name, kind):
    """``blob_log_blocks`` on the two-scale ladder: coordinates, scale index and float64 values of the resolved peaks
    equal those of the same call on the separate passes -- and, for uint16 voxels, those of the oracle.  The path is
    the tiled one wherever the batch's plan fits the slot ``blob_log`` gives it."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    dvol = bl.DeviceVolume(_voxels(volume(name), kind))
    origins, shapes = [o for o, _ in CASES[name][2]], [s for _, s in CASES[name][2]]
    res, peaks = bl.blob_log_blocks(dvol, 0, origins, shapes, *SIGMAS, THRESHOLD, OVERLAP, return_peaks=True)
    path = bl.LAST_ZX_PATH
    fits = _plan_fits(shapes, 2 if kind == "f32" else 1)
    print(name, kind, "path", path, "plan fits", fits)
    assert path == (nat.MMX_ZX_TILED_Q16 if fits else nat.MMX_ZX_SEPARATE)
    assert fits or min(shapes)[0] == 20                            # (only the 20-plane blocks do not: the module's docstring)
    monkeypatch.setattr(bl, "ZX_MODE", nat.MMX_ZX_SEPARATE)
    res_s, peaks_s = bl.blob_log_blocks(dvol, 0, origins, shapes, *SIGMAS, THRESHOLD, OVERLAP, return_peaks=True)
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_SEPARATE
    assert len(peaks[0][0]) > 6
    for i in range(len(shapes)):
        np.testing.assert_array_equal(peaks[i][0], peaks_s[i][0])
        np.testing.assert_array_equal(peaks[i][1], peaks_s[i][1])
        np.testing.assert_array_equal(res[i], res_s[i])
        if kind == "u16":
            want_res, want_peaks, want_values = oracle_peaks(name, i)
            np.testing.assert_array_equal(peaks[i][0], want_peaks)
            np.testing.assert_array_equal(peaks[i][1], want_values)
            np.testing.assert_array_equal(res[i], want_res)


def test_blob_log_of_a_wide_image_equals_the_oracle(gpu):
    """``blob_log`` of the 1040 voxels wide volume as one image: the oracle's rows, row for row, from the tiled path."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    want, _, _ = oracle_peaks("1040", 0)
    got = bl.blob_log(volume("1040"), *SIGMAS, THRESHOLD, OVERLAP)
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_TILED_Q16
    assert len(want) > 12
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------- 3. the rules that did not move
def test_rules_beside_the_row_width_are_unchanged(gpu):
    """Float voxels with no stated range still take the separate passes at 530 wide (no tiled path without a range,
    and the packed kernel stops at 320 floats); a uint16 block of 40 x 20 x 530 at radius 18 still does, because the
    fused path needs R + 4 = 22 rows.  Both against the oracle at the float32 passes' tolerance."""
    from magellanmapper_amd import _native as nat, blob_log as bl, synth
    from oracle import blob_log_oracle as blo
    vol = _voxels(volume("530"), "f32")
    space = bl.ScaleSpace.make(2.05, 2.05, 1)
    assert space.radii[0] == 8
    got = bl.log_cube_blocks(bl.DeviceVolume(vol), 0, [(0, 0, 0)], [vol.shape], space, value_range=0.0)[0][..., 0]
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_SEPARATE
    assert np.abs(got - _reference("530", 0, "f32", 8)).max() < F32_TILE_TOL
    thin = synth.make_volume(105, (40, 20, 530), 12, blob_sigma=4.0)
    space = bl.ScaleSpace.make(4.55, 4.55, 1)
    assert space.radii[0] == 18
    assert _plan_fits([thin.shape], 1)                             # (not for want of room)
    got = bl.log_cube_blocks(bl.DeviceVolume(thin), 0, [(0, 0, 0)], [thin.shape], space)[0][..., 0]
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_SEPARATE
    want = blo.log_cube(blo.img_as_float(thin), np.array([[4.55] * 3]))[..., 0]
    assert np.abs(got - want).max() < F32_TILE_TOL


# ---------------------------------------------------------------- 4. a stack of wide blocks
@pytest.mark.parametrize("denoise", [None, 25], ids=["raw", "denoise25"])
def test_stack_with_blocks_wider_than_512_equals_the_oracle(gpu, denoise):
    """A 40 x 60 x 1100 uint16 stack at 1 um / px with ``segment_size`` 560: two blocks, 565 and 540 voxels wide, with
    blobs on both sides of the panel seam of either (test_wide_rows_host.py), on the 16-bit tiles -- raw (the uint16
    copy) and preprocessed (ranged float voxels, the float copy) -- and the final table equal to the oracle's."""
    from magellanmapper_amd import _native as nat, blob_log as bl, config, stack_detect
    from oracle import magmap_oracle as mmo
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(num_sigma=STACK_SIGMAS[2], denoise_size=denoise, segment_size=STACK_SEGMENT,
                                   min_sigma_factor=STACK_SIGMAS[0], max_sigma_factor=STACK_SIGMAS[1]))
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "wide_rows"
    vol = stack_volume()
    try:
        layout = mmo.setup_blocks(dict(config.roi_profile), vol.shape, config.resolutions)
        widths = [s[2].stop - s[2].start for s in np.asarray(layout["sub_roi_slices"]).ravel()]
        assert widths == [shape[2] for _, shape in STACK_BLOCKS] == [565, 540]
        img5d = stack_detect.Image5d(vol[None])
        _, _, blobs = stack_detect.detect_blobs_blocks("wide_rows", img5d, None, None, None, False, False, True, False)
        assert bl.LAST_ZX_PATH == nat.MMX_ZX_TILED_Q16, bl.LAST_ZX_PATH
        want, _ = mmo.detect_blobs_blocks(vol, None, [dict(config.roi_profile)], config.resolutions)
        got = blobs.blobs
        assert want is not None and got is not None and got.shape == want.shape and len(want) > 10
        for seam in (512, 560 + 512):                              # (the oracle's table has blobs at either seam)
            assert (np.abs(want[:, 2] - seam) <= 8).sum() >= 6, seam
        key = lambda t: t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]      # noqa: E731
        np.testing.assert_array_equal(key(got), key(want))
    finally:
        config.setup_roi_profiles(None)
