"""int16 images on the device: the native voxel type ``MMX_I16`` from the C ABI to ``detect_blobs_stack`` against the
oracle on the int16 array itself (the cases and their "this can fail" checks: ``test_int16_host.py``).

Nominated float32 cubes stay within the bound the library states -- for the value span 2 of a signed image --, every
float64 value, every preprocessed voxel, every bound and every table is compared bit for bit / row for row.
"""
import ctypes

import numpy as np
import pytest

import test_int16_host as cases
from conftest import lexsorted, load_golden
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

#: float32 paths on images in [0, 1] are held to 1e-6 by the existing parity tests (``LOG_TOL * 1e-2``); a signed image
#: spans 2, and the tiled path carries it as [0, 2] less a constant: twice that
F32_TOL = 2e-6
EPS = 2.5e-4            # the product's band for raw integer volumes (blob_log.EPS_REL_Q16)


@pytest.fixture
def env(monkeypatch):
    """The preprocessing tests' environment (test_gpu_preproc.py): both sides on the fixtures' sigma-8 weights."""
    from magellanmapper_amd import config, preprocess
    from oracle import preprocess_oracle as ppo
    g = load_golden("preproc.npz")
    monkeypatch.setattr(preprocess, "RGB_GUESS", True)
    monkeypatch.setattr(preprocess, "GAUSS_WEIGHTS_OVERRIDE", np.ascontiguousarray(g["gauss8_weights"][32:]))
    monkeypatch.setattr(ppo, "GAUSS_WEIGHTS", g["gauss8_weights"])
    yield
    config.setup_roi_profiles(None)
    config.near_max = [-1.0]
    config.resolutions = None


# ------------------------------------------------------------------------------------------------------------ 1. ABI
def _space(sigmas):
    from magellanmapper_amd import blob_log as bl
    space = bl.ScaleSpace.make(float(sigmas[0]), float(sigmas[-1]), len(sigmas))
    np.testing.assert_array_equal(space.sigmas, np.asarray(sigmas, dtype=np.float64))
    return space


def _q16_bound(space):
    """The bound of the 16-bit tiles for this ladder in value units of a SIGNED image: span 2."""
    from magellanmapper_amd import _native as nat
    L = nat.lib()
    return 2.0 * max(L.mmx_tiled_q16_error_bound(nat.as_double_ptr(space.w0[s]), nat.as_double_ptr(space.w2[s]),
                                                 int(space.radii[s]), float(space.norms[s]))
                     for s in range(len(space.sigmas)))


def _cubes(monkeypatch, dvol, name, mode, flags=0, generic=False):
    """``mmx_log_batch_f32`` (or the generic entry) per scale: the float32 cubes of the case's blocks, the path run."""
    from magellanmapper_amd import blob_log as bl
    _, origins, shapes, sigmas = cases.log_case(name)
    monkeypatch.setattr(bl, "ZX_MODE", int(mode))
    monkeypatch.setattr(bl, "ZX_FLAGS", int(flags))
    got = bl.log_cube_blocks(dvol, 0, origins, shapes, _space(sigmas), generic=generic)
    return got, bl.LAST_ZX_PATH


def _u16_path(monkeypatch, name, mode, flags=0):
    """The path the same call takes for a uint16 volume of the same geometry: int16 must route alike."""
    from magellanmapper_amd import blob_log as bl
    vol = cases.log_case(name)[0]
    return _cubes(monkeypatch, bl.DeviceVolume((vol.view(np.uint16) ^ np.uint16(0x8000))), name, mode, flags)[1]


LOG_RUNS = [
    # case, zx_mode, flags, the path it must report (None: whatever uint16 reports), 16-bit tiles
    ("tiled", "MMX_ZX_TILED_Q16", 0, 7, True),
    ("tiled", "MMX_ZX_TILED_Q16", "MMX_ZX_Y_VALU", 7, True),
    ("tiled", "MMX_ZX_TILED", 0, 6, False),
    ("tiled", "MMX_ZX_PACKED", 0, 2, False),
    ("tiled", "MMX_ZX_SEPARATE", 0, 0, False),
    ("tiled", "MMX_ZX_AUTO", 0, None, False),
    ("ragged", "MMX_ZX_TILED_Q16", 0, 7, True),
    ("ragged", "MMX_ZX_TILED", 0, 6, False),
    ("two_kstep", "MMX_ZX_TILED_Q16", 0, 7, True),
    ("two_kstep", "MMX_ZX_TILED_Q16", "MMX_ZX_EDGE_GLOBAL", 7, True),
    ("two_kstep", "MMX_ZX_TILED", 0, 6, False),
    ("wide", "MMX_ZX_AUTO", 0, 8, False),
    ("wide", "MMX_ZX_WIDE", 0, 8, False),
    ("thin", "MMX_ZX_THIN", 0, 9, False),
    ("wide_rows", "MMX_ZX_TILED_Q16", 0, None, True),          # (20 rows, 20 planes: the separate passes, as for uint16)
    ("wide_rows", "MMX_ZX_AUTO", 0, None, False),
    ("wide_rows_tiled", "MMX_ZX_TILED_Q16", 0, 7, True),        # the panelled voxel copy
    ("wide_rows_tiled", "MMX_ZX_TILED", 0, 6, False),
]


@pytest.mark.parametrize("name,mode,flags,path,q16", LOG_RUNS,
                         ids=["%s-%s%s" % (r[0], r[1][7:].lower(), "-" + r[2][7:].lower() if r[2] else "") for r in LOG_RUNS])
def test_log_batch_of_an_int16_volume(gpu, monkeypatch, name, mode, flags, path, q16):
    """``mmx_log_batch_f32`` with an ``MMX_I16`` volume, one case per kernel family and a two-scale ladder each: the
    family that ran (``h_zx_path``) and the float32 cube against the oracle's -- within the stated bound x span 2 on
    16-bit tiles, within float32 rounding elsewhere.  A load biased by 32768 that forgot a scale's constant would be off
    by 1.6e-3 and more."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    vol, origins, shapes, sigmas = cases.log_case(name)
    dvol = bl.DeviceVolume(vol)
    assert dvol.view(0, True).dtype == nat.MMX_I16 and dvol.tensor.element_size() == 2
    mode_v = getattr(nat, mode)
    flags_v = getattr(nat, flags) if flags else 0
    got, ran = _cubes(monkeypatch, dvol, name, mode_v, flags_v)
    want_path = path if path is not None else _u16_path(monkeypatch, name, mode_v, flags_v)
    assert ran == want_path, (ran, want_path)
    on_q16 = ran == nat.MMX_ZX_TILED_Q16
    assert on_q16 == q16 or path is None
    space = _space(sigmas)
    tol = _q16_bound(space) if on_q16 else F32_TOL
    if on_q16:
        assert 5e-5 < tol < 1.1e-4
    for g, w in zip(got, cases.log_cubes(name)):
        err = np.abs(g.astype(np.float64) - w).max(axis=(0, 1, 2))
        print(name, mode, flags, "path", ran, "max |f32 - f64| per scale", err, "tol", tol)
        assert (err < tol).all(), (err, tol)


def test_generic_entry_of_an_int16_volume(gpu, monkeypatch):
    from magellanmapper_amd import _native as nat, blob_log as bl
    for name in ("tiled", "thin"):
        vol = cases.log_case(name)[0]
        got, _ = _cubes(monkeypatch, bl.DeviceVolume(vol), name, nat.MMX_ZX_AUTO, generic=True)
        for g, w in zip(got, cases.log_cubes(name)):
            assert np.abs(g.astype(np.float64) - w).max() < F32_TOL


def test_edge_tables_in_lds_and_in_global_memory_give_the_same_bits(gpu, monkeypatch):
    """Radius 18 / 20 on 16-bit tiles: the LDS edge form of the z march stays available for int16 and equals the
    global-table form (``MMX_ZX_EDGE_GLOBAL``) bit for bit -- and both equal what the same kernels give for the uint16
    volume ``x ^ 0x8000`` once that volume's own constant is accounted for by the oracle (checked above); here: bits."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    vol = cases.log_case("two_kstep")[0]
    dvol = bl.DeviceVolume(vol)
    lds, p0 = _cubes(monkeypatch, dvol, "two_kstep", nat.MMX_ZX_TILED_Q16)
    glb, p1 = _cubes(monkeypatch, dvol, "two_kstep", nat.MMX_ZX_TILED_Q16, nat.MMX_ZX_EDGE_GLOBAL)
    assert p0 == p1 == nat.MMX_ZX_TILED_Q16
    for a, b in zip(lds, glb):
        np.testing.assert_array_equal(a, b)


def _detect(vol, origins, shapes, sigmas, thr, zx_mode, zx_flags=0, eps=EPS):
    """``mmx_detect_batch`` from raw pointers (as tests/test_gpu_parity.py drives it): ``(info, candidate rows)``."""
    from magellanmapper_amd.rawbatch import RawBatch
    cap = 60000
    b = RawBatch(vol, origins, shapes, _space(sigmas), thr, eps, cap, zx_mode=zx_mode, zx_flags=zx_flags, host_entries=cap,
                 event=True)
    info = b.detect()
    b.event.synchronize()
    torch.cuda.synchronize()
    n_all, n_cands = b.counts(host=True)
    assert 0 < n_cands <= n_all <= cap
    return info, b.table(host=True)[:n_all].copy(), n_cands, _q16_bound(b.space)


DETECT_RUNS = [("tiled", "MMX_ZX_AUTO", 7), ("tiled", "MMX_ZX_TILED", 6), ("tiled", "MMX_ZX_PACKED", 2),
               ("tiled", "MMX_ZX_SEPARATE", 0), ("ragged", "MMX_ZX_AUTO", 7), ("two_kstep", "MMX_ZX_AUTO", 7),
               ("wide", "MMX_ZX_AUTO", 8), ("thin", "MMX_ZX_THIN", 9), ("wide_rows", "MMX_ZX_AUTO", None),
               ("wide_rows_tiled", "MMX_ZX_AUTO", 7)]


@pytest.mark.parametrize("name,mode,path", DETECT_RUNS, ids=["%s-%s" % (r[0], r[1][7:].lower()) for r in DETECT_RUNS])
def test_detect_batch_of_an_int16_volume(gpu, monkeypatch, name, mode, path):
    """``mmx_detect_batch`` with ``MMX_I16`` volumes (nomination and exact re-score read the same int16 voxels): the
    family (``mmx_detect_info``), the bound of the 16-bit tiles stated for span 2, every peak of the real rule on the
    oracle's float64 cube nominated, and EVERY ``v64`` the batch wrote equal to that cube bit for bit."""
    from magellanmapper_amd import _native as nat
    from oracle import blob_log_oracle as blo
    vol, origins, shapes, sigmas = cases.log_case(name)
    thr = cases.THRESHOLD
    info, cands, n_cands, bound = _detect(vol, origins, shapes, sigmas, thr, getattr(nat, mode))
    if path is None:
        u16 = vol.view(np.uint16) ^ np.uint16(0x8000)
        path = _detect(u16, origins, shapes, sigmas, thr, getattr(nat, mode))[0].zx_path
    assert info.zx_path == path, (info.zx_path, path)
    if info.zx_path == nat.MMX_ZX_TILED_Q16:
        assert info.q16_bound == bound and 4.0 * info.q16_bound <= EPS
    else:
        assert info.q16_bound == 0.0
    n_peaks = 0
    for b, cube in enumerate(cases.log_cubes(name)):
        want = blo.peak_coords(cube, blo.peak_mask(cube, thr))
        mine = cands[cands["slot"] == b]
        scored = mine[~np.isnan(mine["v64"]) & (mine["s"] >= 0) & (mine["s"] < cube.shape[3])]
        assert len(scored) >= len(want)
        np.testing.assert_array_equal(scored["v64"], cube[scored["z"], scored["y"], scored["x"], scored["s"]])
        have = set(zip(mine["z"].tolist(), mine["y"].tolist(), mine["x"].tolist(), mine["s"].tolist()))
        for z, y, x, s_ in want:
            assert (int(z), int(y), int(x), int(s_)) in have
        n_peaks += len(want)
    assert n_peaks >= 3


def test_float32_tiles_when_the_band_does_not_cover_the_doubled_bound(gpu):
    """``MMX_ZX_AUTO``: the band of unsigned volumes' kernels covers 4 x the bound of span 1 but, just below 2.4e-4, not
    of span 2 -- int16 then keeps float32 tiles where uint16 takes 16-bit ones."""
    from magellanmapper_amd import _native as nat
    vol, origins, shapes, sigmas = cases.log_case("tiled")
    info, _, _, bound = _detect(vol, origins, shapes, sigmas, cases.THRESHOLD, nat.MMX_ZX_AUTO, eps=1.5e-4)
    assert 4.0 * bound > 1.5e-4 >= 2.0 * bound           # (`bound` is for span 2: 4 x bound / 2 <= eps < 4 x bound)
    assert info.zx_path == nat.MMX_ZX_TILED and info.q16_bound == 0.0
    u16 = vol.view(np.uint16) ^ np.uint16(0x8000)
    info, _, _, _ = _detect(u16, origins, shapes, sigmas, cases.THRESHOLD, nat.MMX_ZX_AUTO, eps=1.5e-4)
    assert info.zx_path == nat.MMX_ZX_TILED_Q16


# ------------------------------------------------------------------------------------------------------ 2. blob_log
@pytest.mark.parametrize("name", ["tiled", "two_kstep", "thin"])
def test_blob_log_of_an_int16_image(gpu, name):
    from magellanmapper_amd import _native as nat, blob_log as bl
    from oracle import blob_log_oracle as blo
    vol, _, _, sigmas = cases.log_case(name)
    want = blo.blob_log(vol, sigmas[0], sigmas[-1], len(sigmas), cases.THRESHOLD, cases.OVERLAP)
    got = bl.blob_log(vol, sigmas[0], sigmas[-1], len(sigmas), cases.THRESHOLD, cases.OVERLAP)
    assert len(want) > 3
    np.testing.assert_array_equal(lexsorted(got), lexsorted(want))
    if name != "thin":
        assert bl.LAST_ZX_PATH == nat.MMX_ZX_TILED_Q16      # the default route of a raw int16 image: 16-bit tiles
    # a device tensor and a read-only array are held as int16 too
    t = torch.from_numpy(vol.copy()).to(gpu)
    dv = bl.DeviceVolume(t)
    assert dv.np_dtype == np.int16 and dv.tensor.dtype == torch.int16 and dv.value_range(0) == (-1.0, 1.0)


# ------------------------------------------------------------------------------------------------- 3. preprocessing
@pytest.mark.parametrize("dms", cases.DMS_LIST)
def test_preprocessed_int16_block_matches_oracle(gpu, env, monkeypatch, dms):
    """Raw int16 values through the contrast stretch (``near_max`` in raw units), the unsharp mask and the erosion:
    ``MMX_PP_SINGLE``, ``MMX_PP_PIPELINED`` and the generic entry against ``preprocess_block``, every float64 voxel.
    The block holds an all-negative tile, a constant tile (identity: raw values passed on) and a two-valued tile whose
    ``clip_vmin`` percentile wraps in int16."""
    from magellanmapper_amd import _native as nat, preprocess
    from oracle import preprocess_oracle as ppo
    roi = cases.preproc_block()
    profs = cases.stack_profiles(n=1)
    want = ppo.preprocess_block(roi, dms, profs, [cases.NEAR_MAX])
    assert want.dtype == np.float64
    runs = [("generic", None, True), ("one output per lane", None, "big")]
    fits_lds = max(dms) <= 32
    if fits_lds:
        runs = [("single", nat.MMX_PP_SINGLE, False), ("pipelined", nat.MMX_PP_PIPELINED, False)] + runs
    for label, mode, force in runs:
        monkeypatch.setattr(preprocess, "KERNEL_MODE", nat.MMX_PP_AUTO if mode is None else mode)
        monkeypatch.setattr(preprocess, "FORCE_GENERIC", force)
        got, infos = preprocess.preprocess_roi(roi, dms, near_max=[cases.NEAR_MAX], return_info=True)
        np.testing.assert_array_equal(got, want, err_msg=label)
        info = np.concatenate([i[1] for i in infos])
        if tuple(dms) == (25, 25, 25):
            assert (info["flags"] & nat.MMX_PP_IDENTITY).sum() >= 1
            assert (info["vmin"] < -30000).any()                      # the wrapped percentile, below both values


# -------------------------------------------------------------------------------------------------------- 4. bounds
def test_intensity_bounds_of_an_int16_image(gpu):
    from magellanmapper_amd import importer
    img = cases.bounds_image()
    lows = [np.percentile(p, 0.5) for p in img]
    highs = [np.percentile(p, 99.5) for p in img]
    assert lows[3] > 30000                                            # the wrap plane's low bound (wrapped difference)
    near_min, near_max = importer.measure_near_bounds(img)
    assert near_min == [min(lows)] and near_max == [max(highs)]
    lo, hi = importer.calc_intensity_bounds(img)
    want = np.percentile(img, (0.5, 99.5))
    assert lo == [want[0]] and hi == [want[1]]
    # the wrap plane alone as the whole image, and a two-channel image
    lo, hi = importer.calc_intensity_bounds(img[3:4])
    assert (lo[0], hi[0]) == (lows[3], highs[3])
    two = np.stack((img, img[::-1]), axis=-1)
    near_min, near_max = importer.measure_near_bounds(two)
    assert near_min == [min(lows)] * 2 and near_max == [max(highs)] * 2


# --------------------------------------------------------------------------------------------------------- 5. stack
def _stack(monkeypatch, tmp_path, roi, over=None, res=(1.0, 1.0, 1.0), coloc=False, unmix=None, near_max=cases.NEAR_MAX,
           image=None):
    """``stack_detect.detect_blobs_blocks`` and the oracle on the same int16 stack: ``(blobs, want, stages)``."""
    from magellanmapper_amd import config, stack_detect
    from oracle import magmap_oracle as mmo
    monkeypatch.chdir(tmp_path)
    profs = cases.stack_profiles(over)
    config.resolutions = np.array([list(res)])
    config.filename = "i16"
    monkeypatch.setattr(config, "near_max", [near_max] * roi.shape[3])
    for p in config.roi_profiles:
        p.spectral_unmixing = unmix
    if unmix is not None:
        profs = [dict(p, spectral_unmixing=unmix) for p in profs]
    try:
        _, _, blobs = stack_detect.detect_blobs_blocks("i16", stack_detect.Image5d(roi[None] if image is None else image),
                                                       None, None, None, False, False, True, coloc)
        want, st = mmo.detect_blobs_blocks(roi, None, profs, config.resolutions, near_max=[near_max] * roi.shape[3],
                                           coloc=coloc)
    finally:
        for p in config.roi_profiles:
            p.spectral_unmixing = None
    return blobs, want, st


@pytest.mark.parametrize("coloc", [False, True])
def test_stack_of_int16_voxels_matches_oracle(gpu, env, monkeypatch, tmp_path, coloc):
    """2 x 2 x 2 blocks of a (40, 70, 70, 2) int16 stack, stock preprocessing, ``near_max`` in raw units; the device
    copy holds 2 bytes per voxel."""
    from magellanmapper_amd import blob_log as bl
    roi = cases.stack_image()
    made = []
    init = bl.DeviceVolume.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append((tuple(self.tensor.shape), self.tensor.dtype, self.tensor.element_size()))
    monkeypatch.setattr(bl.DeviceVolume, "__init__", spy)
    blobs, want, st = _stack(monkeypatch, tmp_path, roi, coloc=coloc)
    assert np.asarray(st["blocks"]["sub_roi_slices"]).shape == (2, 2, 2)
    assert want is not None and len(want) > 40 and set(np.unique(want[:, 6])) == {0.0, 1.0}
    np.testing.assert_array_equal(blobs.blobs, want)
    whole = [m for m in made if m[0] == roi.shape]
    assert whole and all(m[1] == torch.int16 and m[2] == 2 for m in whole)
    if coloc:
        np.testing.assert_array_equal(blobs.colocalizations, st["colocs"])
        assert st["colocs"][:, 1].any()


def test_stack_with_spectral_unmixing_by_a_float_factor(gpu, env, monkeypatch, tmp_path):
    roi = cases.stack_image()
    for over in ({}, {"denoise_size": None}):           # preprocessed float64 blocks / raw int16 voxels, in float64
        blobs, want, _ = _stack(monkeypatch, tmp_path, roi, over=over, unmix={0: {1: 0.4}})
        assert want is not None and len(want) > 20
        np.testing.assert_array_equal(blobs.blobs, want)


def test_integer_unmixing_factor_is_still_refused(gpu, env, monkeypatch, tmp_path):
    roi = cases.stack_image()
    with pytest.raises(NotImplementedError, match="int16"):
        _stack(monkeypatch, tmp_path, roi, over={"denoise_size": None}, unmix={0: {1: 1}})


@pytest.mark.parametrize("denoise", [25, None])
def test_stack_with_isotropic_rescale(gpu, env, monkeypatch, tmp_path, denoise):
    """``isotropic = (0.9, 1, 1)`` at resolutions (2, 1, 1): after the stock preprocessing (float64 blocks), and on the
    raw voxels, where the resized block is clipped to the raw range and cast back to int16 by truncation."""
    roi = cases.stack_image()
    blobs, want, _ = _stack(monkeypatch, tmp_path, roi, over={"isotropic": (0.9, 1, 1), "denoise_size": denoise},
                            res=(2.0, 1.0, 1.0))
    assert want is not None and len(want) > 20
    np.testing.assert_array_equal(blobs.blobs, want)


def test_isotropic_int16_block_is_truncated_like_the_reference(gpu):
    from magellanmapper_amd import preprocess
    from oracle import isotropic_oracle as iso
    vol = cases.make_volume((20, 30, 30), 61, n_blobs=4)
    want = iso.make_isotropic(vol, 0.9, (2.0, 1.0, 1.0))
    got = preprocess.make_isotropic(vol, 0.9, (2.0, 1.0, 1.0))
    assert got.dtype == np.int16
    np.testing.assert_array_equal(got, want)


def test_memory_mapped_int16_stack_in_two_chunks(gpu, env, monkeypatch, tmp_path):
    """A read-only memory map with ``MAX_RESIDENT_BYTES`` small enough for two chunks: the same table, every device
    copy 2 bytes per voxel."""
    from magellanmapper_amd import blob_log as bl, stack_detect, volume
    roi = cases.stack_image()
    np.save(tmp_path / "i16_image5d.npy", roi[None])
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    made = []
    init = bl.DeviceVolume.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append((self.z_off, tuple(self.tensor.shape), self.tensor.dtype))
    monkeypatch.setattr(bl.DeviceVolume, "__init__", spy)
    plane = int(np.prod(roi.shape[1:])) * 2
    # (the image is LARGER than the limit, and half the limit holds less than the two block layers together)
    monkeypatch.setattr(stack_detect, "MAX_RESIDENT_BYTES", 30 * plane)
    mapped = np.load(tmp_path / "i16_image5d.npy", mmap_mode="r")
    assert isinstance(mapped, np.memmap) and not mapped.flags.writeable
    blobs, want, _ = _stack(monkeypatch, tmp_path, roi, image=mapped)
    np.testing.assert_array_equal(blobs.blobs, want)
    # whole layers of blocks, or runs of block rows of a layer: boxes of the map, x and the channels whole
    chunks = [m for m in made if len(m[1]) == 4 and m[1][2:] == roi.shape[2:]]
    assert len(chunks) >= 2 and all(int(np.prod(m[1])) < roi.size for m in chunks)
    assert all(m[2] == torch.int16 for m in chunks)


# ---------------------------------------------------------------------------------- 6. patches and co-localisation
def test_patches_of_an_int16_image(gpu):
    """``mmx_extract_patches`` on signed voxels against the host statement of the formula: negative maxima (an
    all-negative patch: quotients >= 1), an all-zero patch (0 / 0: NaN), the two extreme values."""
    from magellanmapper_amd import blob_log as bl, classifier
    vol = cases.make_volume((12, 40, 44), 71, n_blobs=6, face_blobs=False)
    vol[2, 0:20, 0:20] = 0                                  # an all-zero patch around (2, 10, 10)
    vol[5, 20:40, 24:44] = np.random.default_rng(3).integers(-32768, -100, (20, 20)).astype(np.int16)   # all negative
    rng = np.random.default_rng(9)
    zyx = np.stack([rng.integers(0, 12, 40), rng.integers(8, 32, 40), rng.integers(8, 36, 40)], axis=1)
    zyx[0], zyx[1] = (2, 10, 10), (5, 30, 34)
    table = np.concatenate([zyx.astype(np.float64), np.ones((40, 1))], axis=1)
    for size in (16, 5, 2):
        want = classifier.extract_patches(vol, table, size)
        got = classifier.extract_patches(bl.DeviceVolume(vol), table, size).cpu().numpy()
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, want)
        assert np.isnan(want[0]).all() and (want[1] >= 1.0).all()
        ref, f32 = classifier._patches_device(bl.DeviceVolume(vol), 0, zyx, size, ref=True, f32=True)
        np.testing.assert_array_equal(f32.cpu().numpy(), want[..., 0].astype(np.float32))


def test_coloc_means_of_an_int16_image(gpu):
    """``mmx_coloc_means`` on an interleaved int16 image: ``np.mean`` of the owned voxels, taken in float64."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    from oracle import coloc_oracle
    from scipy import ndimage as ndi
    roi = cases.stack_image()[:20, :24, :28]
    rng = np.random.default_rng(8)
    n = 60
    pts = np.stack([rng.integers(0, s, n) for s in roi.shape[:3]], axis=1)
    pts[:6] = [[0, 0, 0], [19, 23, 27], [0, 1, 1], [5, 5, 5], [5, 6, 6], [5, 5, 5]]
    chl = rng.integers(0, 2, n)
    chl[3:6] = 0
    dvol = bl.DeviceVolume(np.ascontiguousarray(roi))
    blocks, _ = bl._make_blocks(dvol, 0, [(0, 0, 0)], [roi.shape[:3]])
    d_blocks = bl._to_device_bytes(blocks, gpu)
    rows = np.zeros((n, 5), np.int32)
    rows[:, 1:4] = pts
    rows[:, 4] = chl
    d_rows = torch.from_numpy(rows.reshape(-1)).to(gpu)
    d_off = torch.tensor([0, n], dtype=torch.int32, device=gpu)
    d_mean = torch.empty(n, dtype=torch.float64, device=gpu)
    d_cnt = torch.empty(n, dtype=torch.int32, device=gpu)
    n_neg = 0
    for c in range(2):
        vol = dvol.view(c, False)
        assert vol.dtype == nat.MMX_I16
        nat.check(nat.lib().mmx_coloc_means(ctypes.byref(vol), d_blocks.data_ptr(), 1, d_rows.data_ptr(),
                                            d_off.data_ptr(), n, d_mean.data_ptr(), d_cnt.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "coloc")
        got, cnt = d_mean.cpu().numpy(), d_cnt.cpu().numpy()
        for bc in range(2):
            sel = np.where(chl == bc)[0]
            mask = -np.ones(roi.shape[:3], dtype=int)
            mask[pts[sel, 0], pts[sel, 1], pts[sel, 2]] = sel
            mask = ndi.grey_dilation(mask, footprint=coloc_oracle.ball(2))
            for b in sel:
                vox = roi[mask == b, c]
                assert cnt[b] == vox.size
                if vox.size:
                    assert got[b] == np.mean(vox), (b, c)
                    n_neg += got[b] < 0
                else:
                    assert np.isnan(got[b])
    assert n_neg > 10
