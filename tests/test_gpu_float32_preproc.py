"""GPU tests of the preprocessing of FLOAT32 images under NumPy 2's casting rules (``preprocess.FLOAT32_RULES =
"numpy2"``), bit for bit.  Stretched tiles, blocks and intensity bounds against fixtures the CPU oracle made under the
reference's own NumPy (2.2.6); identity tiles, whose float32 arithmetic does not depend on the NumPy release, against
the REAL reference's ``plot_3d.saturate_roi`` / ``plot_3d.denoise_roi`` (``tests/golden/make_golden_f32.py``)."""
import ast

import numpy as np
import pytest

from conftest import load_golden
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TILES = load_golden("preproc_f32.npz")
IDENT = load_golden("preproc_f32_identity.npz")
NUMPY2 = int(np.__version__.split(".")[0]) >= 2


def _set_profiles(over):
    from magellanmapper_amd import config
    config.setup_roi_profiles(["default"])
    config.roi_profiles[0].update(over)
    return dict(config.roi_profiles[0])


@pytest.fixture
def rules(monkeypatch):
    """The switch on, and the weights the fixtures were made with (``np.exp`` is not bit-stable across releases)."""
    from magellanmapper_amd import config, preprocess

    def use(fixture):
        monkeypatch.setattr(preprocess, "FLOAT32_RULES", "numpy2")
        monkeypatch.setattr(preprocess, "RGB_GUESS", False)
        monkeypatch.setattr(preprocess, "GAUSS_WEIGHTS_OVERRIDE", np.ascontiguousarray(fixture["gauss8_weights"][32:]))
    yield use
    config.setup_roi_profiles(None)
    config.near_max = [-1.0]


@pytest.mark.parametrize("case", [str(n) for n in TILES["names"]])
def test_stretched_tile_is_float64_and_matches_the_oracle(gpu, rules, monkeypatch, case):
    """Non-identity tiles: the order statistics from the four-level select on the floats' keys, ``b - a`` of the lerp in
    float32, every voxel widened and then the float64 stages.  The shapes take every kernel form: 25^3 the LDS form
    with 640 lanes, (13, 16, 16), (14, 25, 9) and (2, 1, 5) the LDS form with 256, (32, 40, 36) the scratch-line form,
    (3, 4, 70) the one-output-per-lane kernel; every tile with sides up to 64 is then sent through the scratch-line
    form as well (``FORCE_GENERIC``) and gives the same bits.  Values that share their top key byte, that spread over distinct top bytes with negatives, heavy ties, -0.0, far pairs, near_max."""
    from magellanmapper_amd import _native as nat, preprocess
    rules(TILES)
    roi = TILES[case + "_roi"]
    assert roi.dtype == np.float32
    lds = nat.lib().mmx_preprocess_fast_lds(*roi.shape) != 0
    assert lds == (case not in ("far_big", "long")) and (max(roi.shape) > 64) == (case == "long")
    prof = _set_profiles(ast.literal_eval(str(TILES[case + "_over"])))
    near_max = list(TILES[case + "_near_max"])
    got, infos = preprocess.preprocess_roi(roi, roi.shape[:3], near_max=near_max, return_info=True)
    (subs, info), = infos
    print(case, "vmin", info["vmin"][0], float(TILES[case + "_vmin"]), "vmax", info["vmax"][0], float(TILES[case + "_vmax"]))
    assert got.dtype == np.float64
    assert info["vmin"][0] == TILES[case + "_vmin"] and info["vmax"][0] == TILES[case + "_vmax"]
    if NUMPY2:
        vmin, vmax = np.percentile(roi, (prof["clip_vmin"], prof["clip_vmax"]))
        assert info["vmin"][0] == vmin and info["vmax"][0] == max(vmax, near_max[0] * prof["max_thresh_factor"])
    np.testing.assert_array_equal(got, TILES[case + "_den"])
    if lds:
        monkeypatch.setattr(preprocess, "FORCE_GENERIC", True)
        again, infos2 = preprocess.preprocess_roi(roi, roi.shape[:3], near_max=near_max, return_info=True)
        np.testing.assert_array_equal(again, got)
        assert infos2[0][1]["vmin"][0] == info["vmin"][0] and infos2[0][1]["flags"][0] == info["flags"][0]


def test_far_pair_fixture_differs_from_the_float64_lerp(gpu, rules):
    """What makes float32 its own case: on the far-pair tile the percentile of the widened voxels is another number, so
    a float64 copy of the image (the way round before) does not give the reference's result."""
    from magellanmapper_amd import preprocess
    rules(TILES)
    roi = TILES["far25_roi"]
    _set_profiles(ast.literal_eval(str(TILES["far25_over"])))
    _, infos = preprocess.preprocess_roi(roi.astype(np.float64), roi.shape, near_max=[-1.0], return_info=True)
    assert infos[0][1]["vmax"][0] != TILES["far25_vmax"]


@pytest.mark.parametrize("case", [str(n) for n in IDENT["names"]])
def test_identity_tile_stays_float32_and_matches_the_reference(gpu, rules, monkeypatch, case):
    """``vmin == vmax``: the float32 view goes through denoise_roi in float32 -- clip against the float32 casts of the
    bounds, the blur's double accumulator stored as float32 after every axis pass, a float32 unsharp mask, erosion."""
    from magellanmapper_amd import _native as nat, preprocess
    rules(IDENT)
    roi = IDENT[case + "_roi"]
    _set_profiles(ast.literal_eval(str(IDENT[case + "_over"])))
    got, infos = preprocess.preprocess_roi(roi, roi.shape[:3], near_max=[-1.0], return_info=True)
    flags = int(infos[0][1]["flags"][0])
    assert got.dtype == np.float32
    assert flags & nat.MMX_PP_IDENTITY
    assert bool(flags & nat.MMX_PP_ERODED) == bool(IDENT[case + "_eroded"])
    np.testing.assert_array_equal(got, IDENT[case + "_den"])
    monkeypatch.setattr(preprocess, "FORCE_GENERIC", True)             # the scratch-line form instead of the LDS form
    again = preprocess.preprocess_roi(roi, roi.shape[:3], near_max=[-1.0])
    assert again.dtype == np.float32
    np.testing.assert_array_equal(again, got)


@pytest.mark.parametrize("which,dtype", [("first", np.float32), ("last", np.float64)])
def test_first_tile_decides_the_dtype_of_a_block(gpu, rules, monkeypatch, which, dtype):
    """A (40, 45, 52) block in tiles of (25, 20, 30): an identity FIRST tile makes the reference's merged block float32
    and every float64 piece is rounded into it; an identity tile elsewhere widens into a float64 block.  Every kernel
    form gives the same bits: the LDS form (``KERNEL_MODE`` single / pipelined / auto: one kernel for float32 voxels,
    whose tiles here fill it with 640 lanes and, the ragged ones, 256), the scratch-line form (``FORCE_GENERIC`` True;
    "big" reaches it too for tiles with sides up to 64, as for the integer types).  The one-output-per-lane kernel
    takes tiles with a side above 64: the (3, 4, 70) tile of the test above."""
    from magellanmapper_amd import _native as nat, preprocess
    g = load_golden("preproc_f32_block_%s.npz" % which)
    rules(g)
    _set_profiles({})
    roi, want = g["roi"], g["den"]
    assert want.dtype == dtype
    got = preprocess.preprocess_roi(roi, (25, 20, 30), near_max=[-1.0])
    assert got.dtype == dtype
    np.testing.assert_array_equal(got, want)
    # both blocks in ONE run: the flags are per block, and the float32 copy is the float64 copy rounded
    other = load_golden("preproc_f32_block_%s.npz" % ("last" if which == "first" else "first"))["roi"]
    dvol = preprocess_volume(np.concatenate([roi, other], axis=0))
    pre = preprocess.Preprocessor((25, 20, 30), [-1.0], block_dtypes=True)
    shapes = [roi.shape, other.shape]
    pre.run(dvol, 0, [(0, 0, 0), (roi.shape[0], 0, 0)], shapes)
    assert pre.block_flags.cpu().tolist() == ([1, 0] if which == "first" else [0, 1])
    np.testing.assert_array_equal(pre.fetch(shapes)[0], want.astype(np.float64))
    for force, mode in ((False, nat.MMX_PP_SINGLE), (False, nat.MMX_PP_PIPELINED), (True, nat.MMX_PP_AUTO),
                        ("big", nat.MMX_PP_AUTO)):
        monkeypatch.setattr(preprocess, "FORCE_GENERIC", force)
        monkeypatch.setattr(preprocess, "KERNEL_MODE", mode)
        again = preprocess.preprocess_roi(roi, (25, 20, 30), near_max=[-1.0])
        assert again.dtype == dtype
        np.testing.assert_array_equal(again, want)
    monkeypatch.setattr(preprocess, "FORCE_GENERIC", False)
    monkeypatch.setattr(preprocess, "KERNEL_MODE", nat.MMX_PP_AUTO)
    # a retained channel other than the one run does not stand in the way
    assert pre.retain(dvol, [(0, 0, 0)], [roi.shape], [1]) and not pre.retains(0)
    try:
        pre.run(dvol, 0, [(0, 0, 0)], [roi.shape])
        np.testing.assert_array_equal(pre.block_flags.cpu().tolist(), [1 if which == "first" else 0])
    finally:
        preprocess.release_retained()


def preprocess_volume(arr):
    from magellanmapper_amd import blob_log as bl
    return bl.DeviceVolume(arr)


def test_static_refusals_with_the_switch_on(gpu, rules, monkeypatch):
    """What is not built for float32 images says so before any launch, whatever the data: total-variation denoising,
    several channels in one call, and every caller that takes one dtype per batch (unmixing keeps "not float32")."""
    from magellanmapper_amd import blob_log as bl, preprocess
    rules(TILES)
    roi = np.zeros((6, 8, 10), np.float32)
    _set_profiles({"tot_var_denoise": 0.1})
    with pytest.raises(NotImplementedError, match="tot_var_denoise"):
        preprocess.preprocess_roi(roi, (6, 8, 10))
    _set_profiles({})
    with pytest.raises(NotImplementedError, match="channel"):
        preprocess.preprocess_roi(np.zeros((6, 8, 10, 2), np.float32), (6, 8, 10), near_max=[-1.0, -1.0])
    dvol = bl.DeviceVolume(roi)
    with pytest.raises(NotImplementedError, match="not float32"):
        preprocess.Preprocessor((6, 8, 10), [-1.0]).run(dvol, 0, [(0, 0, 0)], [roi.shape])
    mc = bl.DeviceVolume(np.zeros((6, 8, 10, 2), np.float32))
    un = preprocess.Unmixer([(1, 0.5)], denoise_max_shape=(6, 8, 10), near_max=[-1.0, -1.0])
    with pytest.raises(NotImplementedError, match="not float32"):
        un.run(mc, 0, [(0, 0, 0)], [roi.shape])
    pre = preprocess.Preprocessor((6, 8, 10), [-1.0], block_dtypes=True)
    assert pre.retain(dvol, [(0, 0, 0)], [roi.shape], [0])
    try:
        with pytest.raises(NotImplementedError, match="retain"):
            pre.run(dvol, 0, [(0, 0, 0)], [roi.shape])
    finally:
        preprocess.release_retained()
    monkeypatch.setattr(preprocess, "FLOAT32_RULES", "numpy1")
    with pytest.raises(ValueError, match="FLOAT32_RULES"):
        preprocess.preprocess_roi(roi, (6, 8, 10))
    monkeypatch.setattr(preprocess, "FLOAT32_RULES", None)
    with pytest.raises(NotImplementedError):
        preprocess.preprocess_roi(roi, (6, 8, 10))


class _NoLaunch:
    """Stands in for the device volume of a detection that must be refused before it touches the device: every
    attribute beyond the dtype, the rank and the channel count is an error."""

    def __init__(self, shape):
        self.np_dtype = np.dtype(np.float32)
        self.shape = shape
        self.multichannel = len(shape) > 3
        self.n_channels = shape[3] if len(shape) > 3 else 1

        class _T:
            ndim = len(shape)
        self.tensor = _T()


@pytest.mark.parametrize("combo,match", [
    ("coloc", r"co-localisation \(coloc=True\) of a float32 image"),
    ("isotropic", "isotropic rescale of a float32 image"),
    ("unmixing", "not float32"),
    ("tv", "tot_var_denoise of a float32 image"),
    ("parts", "detected in parts .* of a float32 image"),
    ("channels", "several channels in one detection of a float32 image"),
    ("host_path", "host path 'numpy'"),
])
def test_detection_combinations_are_refused_by_name_before_any_launch(gpu, rules, monkeypatch, combo, match):
    """Each combination the detection of a float32 image with preprocessing does not take raises ``NotImplementedError``
    with a message naming it, from the arguments and profiles alone: the volume handed in has no device tensor, so a
    refusal that came after any set-up or launch would be an ``AttributeError`` instead."""
    from magellanmapper_amd import blob_log as bl, config, detector
    rules(TILES)
    config.setup_roi_profiles(None)
    shape = (30, 32, 34, 2) if combo in ("coloc", "unmixing", "channels") else (30, 32, 34)
    if combo == "isotropic":
        config.roi_profile["isotropic"] = (1, 1, 1)
    if combo == "tv":
        config.roi_profile["tot_var_denoise"] = 0.1
    if combo == "unmixing":
        config.roi_profile.spectral_unmixing = {0: {1: 0.5}}
    if combo == "parts":
        monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", 1000, raising=True)
    if combo == "host_path":
        monkeypatch.setattr(bl, "HOST_PATH", "numpy")
    channel = None if len(shape) == 3 else ([0, 1] if combo == "channels" else [0])
    with pytest.raises(NotImplementedError, match=match):
        detector.detect_blobs_blocks_device(_NoLaunch(shape), channel, [(0, 0, 0)], [shape[:3]],
                                            denoise_max_shape=(25, 25, 25), coloc=combo == "coloc")


def test_one_batch_of_a_float32_and_a_float64_block_through_blob_log(gpu, rules):
    """Two blocks in ONE batch -- the first merged as float32 (identity first tile), the second as float64 -- through
    ``blob_log_blocks``: the exact re-score keeps float32 intermediates for the first and float64 ones for the second
    (``mmx_detect_args.d_block_f32``).  Ordered raw peaks and their values equal the oracle's on the oracle-made
    preprocessed blocks, each in its own dtype; so do the pruned blobs."""
    from magellanmapper_amd import blob_log as bl, preprocess
    from oracle import blob_log_oracle as blo
    first, last = (load_golden("preproc_f32_block_%s.npz" % w) for w in ("first", "last"))
    rules(first)
    _set_profiles({})
    assert first["den"].dtype == np.float32 and last["den"].dtype == np.float64
    dvol = bl.DeviceVolume(np.concatenate([first["roi"], last["roi"]], axis=0))
    shapes = [first["roi"].shape, last["roi"].shape]
    origins = [(0, 0, 0), (shapes[0][0], 0, 0)]
    ladder = (2.0, 3.0, 3, 0.05, 0.5)
    pre = preprocess.Preprocessor((25, 20, 30), [-1.0], block_dtypes=True)
    stats = bl.BatchStats()
    res, peaks = bl.blob_log_blocks(dvol, 0, origins, shapes, *ladder, stats=stats, return_peaks=True, pre=pre)
    assert stats.n_blocks == 2 and pre.block_flags.cpu().tolist() == [1, 0]
    n_peaks = 0
    for i, g in enumerate((first, last)):
        want, st = blo.blob_log(g["den"], *ladder, return_stages=True)
        assert st["peak_values"].dtype == g["den"].dtype
        print("block", i, g["den"].dtype, "peaks", len(peaks[i][0]), "oracle", len(st["peaks"].reshape(-1, 4)))
        np.testing.assert_array_equal(peaks[i][0], st["peaks"].reshape(-1, 4))
        np.testing.assert_array_equal(peaks[i][1], st["peak_values"].astype(np.float64))
        np.testing.assert_array_equal(res[i], want)
        n_peaks += len(peaks[i][0])
    assert n_peaks > 10


def test_float32_stack_with_preprocessing_matches_the_oracle(gpu, rules, monkeypatch, tmp_path):
    """The 48 x 70 x 66 float32 stack with a zeroed 25^3 corner through ``detect_blobs_blocks`` (segment_size 40,
    num_sigma 3, denoise_size 25: 2 x 2 x 2 blocks, the first of them float32): the table equals the fixture's, row for
    row.  With the switch off the same call still raises."""
    from magellanmapper_amd import config, preprocess, stack_detect
    g = load_golden("f32_stack_denoise.npz")
    rules(g)
    monkeypatch.chdir(tmp_path)
    vol, want = g["roi"], g["blobs"]
    assert vol.dtype == np.float32 and vol.shape == (48, 70, 66) and len(want) > 10

    def detect():
        config.setup_roi_profiles(None)
        config.roi_profile.update(ast.literal_eval(str(g["over"])))
        config.resolutions = g["resolutions"]
        return stack_detect.detect_blobs_blocks("f32", stack_detect.Image5d(vol[None]), None, None, None, False, False,
                                                True, False)[2].blobs
    got = detect()
    print("rows", None if got is None else got.shape, "fixture", want.shape)
    assert got is not None and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    monkeypatch.setattr(preprocess, "FLOAT32_RULES", None)
    with pytest.raises(NotImplementedError, match="float32"):
        detect()


def test_intensity_bounds_of_a_float32_image(gpu, rules, monkeypatch):
    """Per-plane and whole-image percentiles of a float32 image, a far-pair plane included: the device's exact order
    statistics, ``b - a`` in float32 on the host."""
    from magellanmapper_amd import importer
    rules(TILES)
    img, planes, whole = TILES["bounds_img"], TILES["bounds_planes"], TILES["bounds_whole"]
    near_min, near_max = importer.measure_near_bounds(img)
    assert near_min == [planes[:, 0].min()] and near_max == [planes[:, 1].max()]
    lows, highs = importer.calc_intensity_bounds(img[None])
    assert (lows[0], highs[0]) == (whole[0], whole[1])
    if NUMPY2:
        want = np.array([np.percentile(p, (0.5, 99.5)) for p in img])
        np.testing.assert_array_equal(want, planes)
        np.testing.assert_array_equal(np.percentile(img, (0.5, 99.5)), whole)
    # the far-pair plane decides the high bound, and the float64 lerp of the same order statistics is another number
    s = np.sort(img[2].reshape(-1)).astype(np.float64)
    from magellanmapper_amd.preprocess import quantile_ranks
    prev, nxt, g = quantile_ranks(s.size, 99.5)
    wide = s[prev] + (s[nxt] - s[prev]) * g if g < 0.5 else s[nxt] - (s[nxt] - s[prev]) * (1 - g)
    assert near_max[0] == planes[2, 1] and planes[2, 1] != wide
    monkeypatch.setattr("magellanmapper_amd.preprocess.FLOAT32_RULES", None)
    with pytest.raises(NotImplementedError):
        importer.measure_near_bounds(img)
