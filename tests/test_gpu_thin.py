"""GPU tests of ``MMX_ZX_THIN`` (``csrc/mmx_thin.hip``: the folded-reflection passes for blocks shorter than the
kernel) and of the batch plan that gives a ragged stack's thin remainders batches of their own: the cubes by name against
the generic passes and the float64 oracle, the mode by name on thick blocks, the golden image of 5 planes through
``blob_log``, and a ragged stack end to end -- the tables of the split plan against the oracle and against the unsplit
plan, raw, streamed, preprocessed, with two co-localised channels and pruned ahead.  Needs a real MI355X (``-m gpu``)."""
import numpy as np
import pytest

from conftest import load_golden
from gpu_support import as_dtype, gpu, timed_cubes  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LOG_TOL = 1e-4
#: float32 passes against the float64 oracle, voxels in [0, 1]: test_gpu_parity.py (radii <= 24), and the bound
#: test_gpu_wide_radius.py holds the float32 passes to above radius 24
F32_TOL, CUBE_TOL = 5e-6, LOG_TOL * 1e-2
FAMILIES = ("zpass", "ypass", "xpass", "generic", "zxpass", "y2pass", "zxpack", "widepass", "thinpass")
DTYPES = [np.uint8, np.uint16, np.float32]


def _thin_blocks(R):
    """The blocks of the cube test, ONE batch: 1, 2 and 3 planes, each axis at R - 1, R and R + 3, a block thin along
    all three axes, rows of 100 and 300 voxels; at non-zero origins of a 44 x 44 x 310 volume."""
    shapes = [(1, 40, 64), (2, 33, 65), (3, 26, 40), (R - 1, 30, 33), (30, R, 31), (30, 31, R + 3), (5, 6, 7), (40, 9, 100),
              (27, 11, 300)]
    origins = [(3, 1, 5), (0, 2, 7), (1, 0, 3), (2, 3, 1), (5, 7, 9), (1, 2, 3), (4, 5, 6), (3, 30, 11), (7, 9, 10)]
    return origins, shapes


_VOLUMES, _REFERENCE = {}, {}


def _volume(name):
    from magellanmapper_amd import synth
    if name not in _VOLUMES:
        if name == "thin":
            _VOLUMES[name] = synth.make_volume(2058, (44, 44, 310), 60, blob_sigma=2.5)
        else:
            # blobs AT the faces and corners of the blocks cut from it: (30, 40, 44) at (1, 2, 3), (66, 70, 40) at (2, 1, 4)
            rng = np.random.default_rng(31)
            centres = rng.uniform((0, 0, 0), (70, 74, 50), (30, 3))
            centres[:8] = [(1, 2, 3), (30, 41, 46), (1, 20, 25), (15, 2, 46), (2, 1, 4), (67, 70, 43), (40, 1, 20), (67, 35, 4)]
            _VOLUMES[name] = synth.make_volume(64, (70, 74, 50), centres=centres, blob_sigma=6.0)
    return _VOLUMES[name]


def _reference(name, dtype, R, origins, shapes):
    """float64 cubes of the blocks at sigma = (R + 0.2) / 4, once per input and radius."""
    from oracle import blob_log_oracle as blo
    key = (name, np.dtype(dtype).name, R)
    if key not in _REFERENCE:
        vol = as_dtype(_volume(name), dtype)
        sigma = (R + 0.2) / 4.0
        _REFERENCE[key] = [blo.log_cube(blo.img_as_float(vol[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]]),
                                        np.array([[sigma] * 3]))[..., 0] for o, s in zip(origins, shapes)]
    return _REFERENCE[key]


def _families(kinds):
    from magellanmapper_amd.rawbatch import families
    return families(kinds, FAMILIES)


def _ring_passes(shapes, R):
    """Passes of a batch that a register-ring kernel takes (csrc/mmx_route.h): z and y from radius + 4 voxels, x from
    radius voxels, radii up to 24."""
    if R > 24:
        return 0
    mins = [min(s[a] for s in shapes) for a in range(3)]
    return int(mins[0] >= R + 4) + int(mins[1] >= R + 4) + int(mins[2] >= R)


def _check_cubes(bl, nat, monkeypatch, name, dtype, R, origins, shapes, tol):
    vol = as_dtype(_volume(name), dtype)
    dvol = bl.DeviceVolume(vol)
    sigma = (R + 0.2) / 4.0
    space = bl.ScaleSpace.make(sigma, sigma, 1)
    assert space.radii[0] == R
    want = _reference(name, dtype, R, origins, shapes)
    monkeypatch.setattr(bl, "ZX_MODE", nat.MMX_ZX_THIN)
    got, kinds = timed_cubes(dvol, origins, shapes, space)
    fams = _families(kinds)
    print("R %d %s families %s" % (R, np.dtype(dtype).name, fams))
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_THIN
    rings = _ring_passes(shapes, R)
    assert fams.get("thinpass", 0) == 3 - rings and "generic" not in fams, fams
    assert sum(fams.get(k, 0) for k in ("zpass", "ypass", "xpass")) == rings
    assert set(fams) <= {"zpass", "ypass", "xpass", "thinpass"}
    again = bl.log_cube_blocks(dvol, 0, origins, shapes, space)
    gen = bl.log_cube_blocks(dvol, 0, origins, shapes, space, generic=True)
    for shp, g, a, ref, ge in zip(shapes, got, again, want, gen):
        err = np.abs(g[..., 0] - ref).max()
        dev = np.abs(g[..., 0] - ge[..., 0]).max()
        print("R %d %s block %s: |thin - oracle| %.3g, |thin - generic| %.3g" % (R, np.dtype(dtype).name, shp, err, dev))
        assert g.shape[:3] == tuple(shp) and np.isfinite(g).all()
        assert dev < 2e-6 * max(1.0, np.abs(ref).max()), (R, shp, dev)
        assert err < tol, (R, shp, err)
        np.testing.assert_array_equal(g, a)                  # two runs: the same bits


# ---------------------------------------------------------------- 1. the cubes by name
@pytest.mark.parametrize("R", [8, 24])
@pytest.mark.parametrize("dtype", DTYPES, ids=["u8", "u16", "f32"])
def test_thin_cubes_by_name(gpu, monkeypatch, dtype, R):
    """Nine thin blocks in one batch under ``MMX_ZX_THIN``: every pass folded (the batch's smallest extents are 1, 6
    and 7), within the float32 paths' agreement of the generic passes and their bound of the float64 oracle."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    origins, shapes = _thin_blocks(R)
    assert _ring_passes(shapes, R) == 0
    _check_cubes(bl, nat, monkeypatch, "thin", dtype, R, origins, shapes, F32_TOL)


@pytest.mark.parametrize("R,origin,shape", [(31, (1, 2, 3), (30, 40, 44)), (64, (2, 1, 4), (66, 70, 40))], ids=["R31", "R64"])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_thin_cubes_at_wide_radii(gpu, monkeypatch, dtype, R, origin, shape):
    """Radii above 24, where no ring kernel runs: a block shorter than the radius along z (R 31), and one whose y extent
    (70) is beyond what the passes fold -- that pass runs the tap loop -- with blobs at its faces."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    assert min(shape) < R + 4 and (R != 64 or shape[1] > nat.MMX_FOLD_MAX_N >= shape[0])
    _check_cubes(bl, nat, monkeypatch, "faces", dtype, R, [origin], [shape], CUBE_TOL)


def test_a_ring_kernel_keeps_its_pass(gpu, monkeypatch):
    """One block of 30 x 30 x 10 at radius 12: Z and Y on the register-ring kernels, X folded."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    origins, shapes = [(2, 3, 5)], [(30, 30, 10)]
    assert _ring_passes(shapes, 12) == 2
    _check_cubes(bl, nat, monkeypatch, "thin", np.uint16, 12, origins, shapes, F32_TOL)


# ---------------------------------------------------------------- 2. by name on thick blocks
def test_thin_by_name_on_thick_blocks_is_auto(gpu, monkeypatch):
    """``MMX_ZX_THIN`` on a batch with no thin block: the path and the kernel families of ``MMX_ZX_AUTO``."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    dvol = bl.DeviceVolume(_stack_volume())
    space = bl.ScaleSpace.make(2.05, 2.05, 1)
    assert space.radii[0] == 8
    origins, shapes = [(1, 2, 3)], [(48, 40, 64)]
    seen = {}
    for mode in (nat.MMX_ZX_AUTO, nat.MMX_ZX_THIN):
        monkeypatch.setattr(bl, "ZX_MODE", mode)
        cubes, kinds = timed_cubes(dvol, origins, shapes, space)
        seen[mode] = (bl.LAST_ZX_PATH, _families(kinds), cubes[0])
    print(seen[nat.MMX_ZX_THIN][:2])
    assert seen[nat.MMX_ZX_THIN][0] == seen[nat.MMX_ZX_AUTO][0] != nat.MMX_ZX_THIN
    assert seen[nat.MMX_ZX_THIN][1] == seen[nat.MMX_ZX_AUTO][1] and "thinpass" not in seen[nat.MMX_ZX_THIN][1]
    np.testing.assert_array_equal(seen[nat.MMX_ZX_THIN][2], seen[nat.MMX_ZX_AUTO][2])


# ---------------------------------------------------------------- 3. the golden image
@pytest.mark.parametrize("mode", ["MMX_ZX_THIN", "MMX_ZX_AUTO"])
def test_blob_log_of_a_thin_image_gives_the_golden_rows(gpu, monkeypatch, mode):
    """``tests/golden/bloblog_u16_thin.npz`` (scikit-image's rows for a uint16 image of 5 planes, radii 12, 14 and 16):
    ``blob_log`` with the mode by name, and under ``MMX_ZX_AUTO`` -- where the one batch of the call asks for the mode
    itself --, gives the stored rows from the folded Z pass."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    g = load_golden("bloblog_u16_thin.npz")
    monkeypatch.setattr(bl, "ZX_MODE", getattr(nat, mode))
    got = bl.blob_log(g["volume"], float(g["min_sigma"]), float(g["max_sigma"]), int(g["num_sigma"]),
                      float(g["threshold"]), float(g["overlap"]))
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_THIN and bl.LAST_MASK_LAYOUT == 0
    assert g["volume"].shape[0] == 5 and len(g["pruned"]) >= 6
    np.testing.assert_array_equal(got, g["pruned"])


# ---------------------------------------------------------------- 4. a ragged stack end to end
STACK_SHAPE = (70, 90, 133)
#: blocks of 48 x 40 x 64 voxels (+ the overlap of 4, 4, 5) with remainders of 22, 10 and 5: segment_size 64 at these
#: resolutions; two scales, radii 8 and 12 -- a block is thin below 16 voxels, so the remainders in y and x are
RESOLUTIONS = np.array([[4.0 / 3.0, 1.6, 1.0]])
PROFILE = dict(num_sigma=2, segment_size=64, min_sigma_factor=2.05, max_sigma_factor=3.05)
#: three regular blocks (52 x 44 x 69 voxels in rows of 96 floats, 25 bytes per voxel) fit, four do not
BUDGET = int(3.5 * 52 * 44 * 96 * 25)


def _stack_volume(channels=1):
    from magellanmapper_amd import synth
    key = ("stack", channels)
    if key not in _VOLUMES:
        vol = synth.make_volume(133, STACK_SHAPE, 90, blob_sigma=2.4, margin=1)
        if channels == 2:
            other = synth.make_volume(134, STACK_SHAPE, 60, blob_sigma=2.4, margin=1)
            vol = np.stack((vol, np.maximum(other, (vol.astype(np.int32) * 7 // 10).astype(vol.dtype))), axis=-1)
        _VOLUMES[key] = vol
    return _VOLUMES[key]


@pytest.fixture
def ragged(monkeypatch):
    """The profile of the ragged stack, a budget of three regular blocks per batch, and a spy on the batches enqueued:
    ``(block shapes, mode asked for, path reported)`` per batch."""
    from magellanmapper_amd import blob_log as bl, config, volume
    config.setup_roi_profiles(None)
    monkeypatch.setattr(bl, "BUDGET_BYTES", BUDGET)
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(config, "resolutions", RESOLUTIONS)
    monkeypatch.setattr(config, "filename", "ragged")
    monkeypatch.setattr(config, "near_max", [-1.0, -1.0])
    seen = []
    enqueue = bl._enqueue_detect

    def spy(dvol, lane, origins, shapes, *a, **k):
        out = enqueue(dvol, lane, origins, shapes, *a, **k)
        seen.append(([tuple(s) for s in shapes], k.get("zx_mode"), bl.LAST_ZX_PATH))
        return out
    monkeypatch.setattr(bl, "_enqueue_detect", spy)

    def setup(denoise=None, channels=1):
        config.setup_roi_profiles(None if channels == 1 else ["default"] * channels)
        config.roi_profile.update(dict(PROFILE, denoise_size=denoise))
        for p in config.roi_profiles:
            p.update(config.roi_profile)
        del seen[:]
    yield setup, seen
    config.setup_roi_profiles(None)


def _grid():
    from magellanmapper_amd import config, stack_detect
    b = stack_detect.setup_blocks(config.roi_profile, STACK_SHAPE)
    origins, shapes = [], []
    for coord in np.ndindex(*b.sub_roi_slices.shape):
        ext = [s.indices(n)[:2] for s, n in zip(b.sub_roi_slices[coord], STACK_SHAPE)]
        origins.append(tuple(int(e[0]) for e in ext))
        shapes.append(tuple(int(e[1] - e[0]) for e in ext))
    return b, origins, shapes


def _check_batches(nat, seen, split):
    """With the split: at least three regular batches on the tiled path, then the thin ones, each asking for and
    reporting ``MMX_ZX_THIN``.  Without: some batches mix thin and regular blocks; they ask for nothing and leave the tiled
    path for the separate passes (a batch the z-major order happens to fill with thin blocks alone still asks for the mode)."""
    thin = [min(min(s) for s in shapes) < 16 for shapes, _, _ in seen]
    if split:
        n_reg = thin.index(True)
        assert n_reg >= 3 and all(thin[n_reg:])
        for shapes, mode, path in seen[:n_reg]:
            assert min(min(s) for s in shapes) >= 16 and mode is None and path == nat.MMX_ZX_TILED_Q16, (shapes, mode, path)
        for shapes, mode, path in seen[n_reg:]:
            assert all(min(s) < 16 for s in shapes) and mode == path == nat.MMX_ZX_THIN, (shapes, mode, path)
    else:
        mixed = [(mode, path) for shapes, mode, path in seen if min(min(s) for s in shapes) < 16 <= max(min(s) for s in shapes)]
        assert mixed and all(mode is None and path == nat.MMX_ZX_SEPARATE for mode, path in mixed), seen


def test_ragged_stack_block_tables(gpu, monkeypatch, ragged):
    """``detect_blobs_blocks_device`` on the 18 blocks of the ragged stack: every block's table equals the oracle's and
    the unsplit plan's; the regular batches run the tiled kernels and no generic pass runs anywhere."""
    from magellanmapper_amd import _native as nat, blob_log as bl, config, detector
    from oracle import magmap_oracle as mmo
    setup, seen = ragged
    setup()
    monkeypatch.setattr(bl, "THIN_SPLIT_MIN_VOXELS", 0)
    vol = _stack_volume()
    _, origins, shapes = _grid()
    assert sorted(set(shapes)) == sorted({(a, b, c) for a in (52, 22) for b in (44, 10) for c in (69, 5)}) and len(shapes) == 18
    nat.timing_enable(True)
    try:
        nat.timing_read()
        got = detector.detect_blobs_blocks_device(bl.DeviceVolume(vol), None, origins, shapes)
        fams = _families(nat.timing_read())
    finally:
        nat.timing_enable(False)
    print("families", fams, "batches", [(len(s), m, p) for s, m, p in seen])
    _check_batches(nat, seen, True)
    assert "generic" not in fams and fams.get("thinpass", 0) > 0 and fams.get("zxpass", 0) > 0
    del seen[:]
    monkeypatch.setattr(bl, "THIN_SPLIT_MIN_VOXELS", 1 << 62)
    unsplit = detector.detect_blobs_blocks_device(bl.DeviceVolume(vol), None, origins, shapes)
    _check_batches(nat, seen, False)
    profs = [dict(config.roi_profile)]
    n_rows = 0
    for o, s, g, u in zip(origins, shapes, got, unsplit):
        want = mmo.detect_blobs(vol[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]], None, profs, config.resolutions)
        assert (g is None) == (want is None) == (u is None), (o, s)
        if want is not None:
            np.testing.assert_array_equal(g, want)
            np.testing.assert_array_equal(g, u)
            n_rows += len(want)
    assert n_rows > 60 and any(g is not None and min(s) < 16 for g, s in zip(got, shapes))


def _stack_run(stack_detect, vol, channels, coloc):
    img = vol[None]
    img5d = stack_detect.Image5d(img)
    _, _, blobs = stack_detect.detect_blobs_blocks("ragged", img5d, None, None, None if channels == 1 else list(range(channels)),
                                                   False, False, True, coloc)
    return blobs


CONFIGS = {
    # name: (channels, denoise_size, coloc, PRUNE_AHEAD, streamed device volume)
    "raw": (1, None, False, "", False),
    "streamed": (1, None, False, "", True),
    "denoise": (1, 25, False, "", False),
    "coloc-2ch": (2, None, True, "", False),
    "prune-ahead": (1, None, False, "1", False),
}


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_ragged_stack_tables(gpu, monkeypatch, ragged, name):
    """``stack_detect.detect_blobs_blocks`` on the ragged stack: the final table (and the co-localisation flags) of the
    split plan equals that of the unsplit plan row for row, and the oracle's; the thin batches come last and report
    ``MMX_ZX_THIN``.  Raw, from a streamed upload, preprocessed, two co-localised channels, pruned ahead."""
    from magellanmapper_amd import _native as nat, blob_log as bl, config, detector, stack_detect
    from oracle import magmap_oracle as mmo
    channels, denoise, coloc, ahead, streamed = CONFIGS[name]
    setup, seen = ragged
    setup(denoise, channels)
    monkeypatch.setattr(stack_detect, "PRUNE_AHEAD", ahead)
    vol = _stack_volume(channels)

    def run():
        if streamed:
            _, origins, shapes = _grid()
            return detector.detect_blobs_blocks_device(bl.DeviceVolume(vol, streamed=True), None, origins, shapes)
        return _stack_run(stack_detect, vol, channels, coloc)

    monkeypatch.setattr(bl, "THIN_SPLIT_MIN_VOXELS", 0)
    got = run()
    split_seen = list(seen)
    print("batches", [(len(s), m, p) for s, m, p in split_seen])
    thin = [min(min(s) for s in shapes) < 16 for shapes, _, _ in split_seen]
    n_reg = thin.index(True)
    assert n_reg >= 3 * channels and all(thin[n_reg:])
    assert all(mode is None and path != nat.MMX_ZX_THIN for _, mode, path in split_seen[:n_reg])
    assert all(mode == path == nat.MMX_ZX_THIN for _, mode, path in split_seen[n_reg:])
    if denoise is None:
        assert all(path == nat.MMX_ZX_TILED_Q16 for _, _, path in split_seen[:n_reg])
    del seen[:]
    monkeypatch.setattr(bl, "THIN_SPLIT_MIN_VOXELS", 1 << 62)
    unsplit = run()
    mixed = [mode for shapes, mode, _ in seen if min(min(s) for s in shapes) < 16 <= max(min(s) for s in shapes)]
    assert mixed and all(mode is None for mode in mixed)         # (batches of thin and regular blocks: today's plan)
    if streamed:
        assert len(got) == len(unsplit) == 18 and sum(len(t) for t in got if t is not None) > 60
        for g, u in zip(got, unsplit):
            assert (g is None) == (u is None)
            if g is not None:
                np.testing.assert_array_equal(g, u)
        return
    assert got.blobs is not None and len(got.blobs) > 60
    np.testing.assert_array_equal(got.blobs, unsplit.blobs)
    profs = [dict(config.roi_profile)] * channels
    if coloc:
        np.testing.assert_array_equal(got.colocalizations, unsplit.colocalizations)
        want, stages = mmo.detect_blobs_blocks(vol, list(range(channels)), profs, config.resolutions, near_max=[-1.0] * channels,
                                               coloc=True)
        np.testing.assert_array_equal(got.blobs, want)
        np.testing.assert_array_equal(got.colocalizations, stages["colocs"])
    else:
        want, _ = mmo.detect_blobs_blocks(vol, None, profs, config.resolutions)
        key = lambda t: t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]      # noqa: E731
        np.testing.assert_array_equal(key(got.blobs), key(want))
