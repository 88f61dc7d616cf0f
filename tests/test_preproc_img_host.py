"""Whole-image preprocessing without a device: the NumPy restatement against the fixture made from the real
scikit-image, the product's host tables and its native clip / map function against the restatement, every refusal
that follows from the arguments, the task names, and ``save_np_image``'s two files."""
import os

import numpy as np
import pytest

import preproc_img_support as sup
from conftest import load_golden
from magellanmapper_amd import _native as nat
from magellanmapper_amd import config, device_image, equalize, importer, preprocess, transformer


@pytest.fixture(scope="module")
def fx():
    return load_golden("preproc_img.npz")


@pytest.fixture(scope="module")
def restated(fx):
    """Every stored case through the restatement, once: ``name -> (input, args, parts, result)``."""
    out = {}
    for name in sup.EQ_CASES:
        img, ks, cl, nb, _, _ = sup.load_case(fx, name)
        parts = {}
        out[name] = (img, (ks, cl, nb), parts, sup.equalize_adapthist(img, ks, cl, nb, parts))
    return out


@pytest.mark.parametrize("name", list(sup.EQ_CASES))
def test_restatement_equals_fixture(fx, restated, name):
    _, _, _, _, clahe, want = sup.load_case(fx, name)
    _, _, parts, got = restated[name]
    assert np.array_equal(parts["clahe"], clahe)
    assert got.dtype == np.float64 and np.array_equal(got, want)


@pytest.mark.parametrize("dtype", sup.DTYPES)
@pytest.mark.parametrize("nbins", [64, 256, 16384])
def test_level_and_bin_table(dtype, nbins):
    """The table by key against NumPy's own expressions applied to an image that holds every value of the type (the
    8- and 16-bit types) or a spread of floats, between two interior extremes."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        vals = np.linspace(-0.3, 0.9, 20001).astype(dtype)
    else:
        info = np.iinfo(dtype)
        vals = np.arange(info.min, info.max + 1, dtype=np.int64)
        vals = vals[(vals >= info.min + (info.max - info.min) // 16) & (vals <= info.max - 5)].astype(dtype)
    u = sup.img_as_uint(vals)
    want = sup.levels_of_uint(u, int(u.min()), int(u.max()))
    levels, bins = equalize.level_bin_table(dtype, vals.min(), vals.max(), nbins)
    key = equalize.key_of_values(vals)
    assert key.min() >= 0 and key.max() < 65536
    assert np.array_equal(levels[key], want)
    assert np.array_equal(bins[key], want // (1 + 16384 // nbins)) and bins.max() < nbins


def test_output_table():
    lv = np.arange(100, 9000, 7, dtype=np.uint16)
    assert np.array_equal(equalize.output_table(100, int(lv.max()))[lv], sup.output_of_levels(lv, 100, int(lv.max())))
    const = np.full(5, 512, dtype=np.uint16)
    assert np.array_equal(equalize.output_table(512, 512)[const], sup.output_of_levels(const, 512, 512))
    assert equalize.output_table(512, 512)[512] == 512 / 65535


@pytest.mark.parametrize("name", list(sup.EQ_CASES))
def test_host_tables_and_native_maps(restated, name):
    """plan + level_bin_table + mmx_host_eq_maps + axis_tables, walked in NumPy as the kernels walk them, give the
    restatement's histograms' maps and its uint16 image."""
    img, (ks, cl, nb), parts, _ = restated[name]
    k, nt, clim = equalize.plan(img.shape, ks, cl, nb)
    assert list(k) == sup.resolve_kernel(img.shape, ks) and nt == parts["ns_hist"]
    assert clim == sup.clip_limit_count(cl, k)
    _, bins = equalize.level_bin_table(img.dtype, img.min(), img.max(), nb)
    hist = np.ascontiguousarray(parts["hist"], dtype=np.uint32)
    n_tiles = hist.shape[0]
    maps = np.empty((n_tiles, nb), dtype=np.uint16)
    entered = np.zeros(n_tiles, dtype=np.uint8)
    nat.check(nat.lib().mmx_host_eq_maps(hist.ctypes.data, n_tiles, nb, clim, int(np.prod(k)), maps.ctypes.data,
                                         entered.ctypes.data), "mmx_host_eq_maps")
    assert np.array_equal(maps, parts["maps"])
    assert np.array_equal(entered.astype(bool), parts["entered"])
    tiles, coef = equalize.axis_tables(img.shape, k, nt)
    got = sup.emulate_apply(bins[equalize.key_of_values(img)].astype(np.int64), maps, tiles, coef, nt, nb)
    assert np.array_equal(got, parts["clahe"])


def test_native_maps_with_no_bin_under_the_limit():
    """Every bin at the limit with excess left: the reference's loop runs one round that changes nothing and ends."""
    hist = np.full((1, 8), 9, dtype=np.uint32)
    maps = np.empty((1, 8), dtype=np.uint16)
    nat.check(nat.lib().mmx_host_eq_maps(hist.ctypes.data, 1, 8, 5, 72, maps.ctypes.data, None), "mmx_host_eq_maps")
    want = sup.map_histogram(sup.clip_histogram(hist[0], 5)[0], 0, 16383, 72)
    assert np.array_equal(maps[0], want)


# ------------------------------------------------------------------------------------------------------- refusals
def _no_device(monkeypatch):
    """Any touch of the device fails the test: the refusals below come from the arguments alone."""
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(device_image, "open_image", boom)
    monkeypatch.setattr(device_image, "free_bytes", boom)


def test_refusals_from_the_arguments(monkeypatch, tmp_path):
    _no_device(monkeypatch)
    img = np.zeros((16, 16, 16), dtype=np.uint16)
    with pytest.raises(NotImplementedError, match="nbins"):
        preprocess.equalize_adapthist(img, nbins=16385)
    with pytest.raises(NotImplementedError, match="nbins"):
        preprocess.remap_intensity(img, nbins=20000, clip_limit=0.01)
    huge = np.lib.stride_tricks.as_strided(img, shape=(2048, 2048, 2048), strides=(0, 0, 0), writeable=False)
    with pytest.raises(NotImplementedError, match="tile"):
        preprocess.equalize_adapthist(huge, kernel_size=(1024, 1024, 2048))
    with pytest.raises(ZeroDivisionError) as exc:
        preprocess.equalize_adapthist(np.zeros((7, 16, 16), dtype=np.uint16))
    with pytest.raises(ZeroDivisionError) as ref:
        7 % 0                                    # (_clahe's `s % k` with the default kernel 7 // 8)
    assert str(exc.value) == str(ref.value)
    for task in ("denoise", "ROTATE", ["saturate", "rotate"]):
        with pytest.raises(NotImplementedError, match="stays in the reference"):
            transformer.preprocess_img(img[None], task, None, str(tmp_path / "out"))
    assert not os.listdir(tmp_path)
    f32 = np.zeros((16, 16, 16), dtype=np.float32)
    monkeypatch.setattr(preprocess, "FLOAT32_RULES", None)
    with pytest.raises(NotImplementedError, match="FLOAT32_RULES"):
        preprocess.saturate_roi(f32)
    with pytest.raises(NotImplementedError):
        preprocess.saturate_roi(np.zeros((16, 16, 16), dtype=np.int32))
    # a float32 result's intensity bounds need the switch as well: refused before the tasks run and a file is made
    with pytest.raises(NotImplementedError, match="FLOAT32_RULES"):
        transformer.preprocess_img(np.zeros((1, 16, 16, 16, 2), dtype=np.float32), "remap", None, str(tmp_path / "f"))
    assert not os.listdir(tmp_path)


def test_image_that_does_not_fit_is_refused(monkeypatch):
    monkeypatch.setattr(device_image, "free_bytes", lambda: 1 << 20)
    img = np.zeros((64, 128, 128), dtype=np.uint16)
    with pytest.raises(NotImplementedError, match="does not fit"):
        preprocess.equalize_adapthist(img)
    with pytest.raises(NotImplementedError, match="does not fit"):
        preprocess.saturate_roi(img)


def test_float32_saturate_passes_the_switch(monkeypatch):
    """Under the NumPy 2 rules a float32 image is taken: the next stop is the device."""
    monkeypatch.setattr(preprocess, "FLOAT32_RULES", "numpy2")

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(device_image, "open_image", reached)
    with pytest.raises(Reached):
        preprocess.saturate_roi(np.zeros((16, 16, 16), dtype=np.float32))


def test_preprocess_keys():
    keys = config.PreProcessKeys
    assert [k.name for k in keys] == ["SATURATE", "DENOISE", "REMAP", "ROTATE"]
    assert transformer._get_enum("saturate", keys) is keys.SATURATE
    assert transformer._get_enum("Remap", keys) is keys.REMAP
    assert transformer._get_enum("sharpen", keys) is None
    assert transformer._get_enum(None, keys) is None and transformer._get_enum(3, keys) is None
    assert transformer.preprocess_img(np.zeros((1, 8, 8, 8)), None, None, "unused") is None


def test_get_if_within_and_channels():
    assert equalize._get_if_within((4, 6, 8), 0) == 4 and equalize._get_if_within((4, 6, 8), 3) is None
    assert equalize._get_if_within(0.5, 2) == 0.5 and equalize._get_if_within(np.array([1, 2]), 1) == 2
    assert equalize._setup_channels((4, 5, 6), [1]) == (False, [0])
    assert equalize._setup_channels((4, 5, 6, 2), None) == (True, range(2))
    assert equalize._setup_channels((4, 5, 6, 2), [1]) == (True, [1])


def test_save_np_image_writes_both_files(monkeypatch, tmp_path):
    img = np.arange(2 * 3 * 4 * 5, dtype=np.float64).reshape(1, 2, 3, 4, 5)[..., 0]
    monkeypatch.setattr(importer, "calc_intensity_bounds", lambda im: ([float(np.percentile(im, 0.5))],
                                                                       [float(np.percentile(im, 99.5))]))
    monkeypatch.setattr(config, "resolutions", np.array([[2.0, 1.0, 1.0]]))
    path = str(tmp_path / "sample.czi")
    importer.save_np_image(importer.roi_to_image5d(img[0]), path)
    assert sorted(os.listdir(tmp_path)) == ["sample_image5d.npy", "sample_meta.yml"]
    assert np.array_equal(np.load(tmp_path / "sample_image5d.npy"), img)
    md, ver = importer.load_metadata(str(tmp_path / "sample_meta.yml"))
    assert ver == importer.IMAGE5D_NP_VER and md["names"] == ["sample.czi"] and md["sizes"] == [[1, 2, 3, 4]]
    assert md["near_min"] == [float(np.percentile(img, 0.5))] and md["near_max"] == [float(np.percentile(img, 99.5))]
    assert md["resolutions"] == [[2.0, 1.0, 1.0]]
