"""Whole-image preprocessing on the device against the fixture made from the real scikit-image / reference: every
comparison is ``np.array_equal``, no tolerance."""
import os

import numpy as np
import pytest

import preproc_img_support as sup
from conftest import load_golden
from gpu_support import gpu  # noqa: F401
from magellanmapper_amd import config, device_image, equalize, importer, preprocess, transformer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_golden("preproc_img.npz")


@pytest.fixture(scope="module")
def restated(fx):
    """The restatement's tile histograms and clipped maps of every stored case, computed once."""
    out = {}
    for name in sup.EQ_CASES:
        img, ks, cl, nb, _, _ = sup.load_case(fx, name)
        parts = {}
        sup.equalize_adapthist(img, ks, cl, nb, parts)
        out[name] = parts
    return out


@pytest.fixture()
def profile(fx):
    """The profile settings and near maxima the fixture was made under."""
    saved = (config.roi_profile, config.roi_profiles, config.near_max, config.resolutions)
    config.setup_roi_profiles(None)
    s = fx["settings"]
    config.roi_profile.update(dict(clip_vmin=float(s[0]), clip_vmax=float(s[1]), max_thresh_factor=float(s[2]),
                                   adapt_hist_lim=float(s[3])))
    config.near_max = [float(v) for v in fx["near_max"]]
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    yield config.roi_profile
    config.roi_profile, config.roi_profiles, config.near_max, config.resolutions = saved


@pytest.mark.parametrize("name", list(sup.EQ_CASES))
def test_equalize_cases(gpu, fx, restated, name):
    img, ks, cl, nb, clahe, want = sup.load_case(fx, name)
    parts = {}
    got = preprocess.equalize_adapthist(img, kernel_size=ks, clip_limit=cl, nbins=nb, parts=parts)
    assert np.array_equal(parts["hist"], restated[name]["hist"])
    assert np.array_equal(parts["maps"], restated[name]["maps"])
    assert np.array_equal(parts["entered"], restated[name]["entered"])
    assert np.array_equal(parts["clahe"], clahe)
    assert got.dtype == np.float64 and got.shape == img.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["nodiv", "float32"])
def test_slabs_resident_volume_and_out(gpu, fx, name, monkeypatch, tmp_path):
    """A result that leaves in several z-slabs, into a memory map, from a resident volume: the same bytes."""
    from magellanmapper_amd.volume import DeviceVolume
    img, ks, cl, nb, _, want = sup.load_case(fx, name)
    monkeypatch.setattr(device_image, "SLAB_BYTES", 3 * img.shape[1] * img.shape[2] * 8)
    out = np.lib.format.open_memmap(str(tmp_path / "out.npy"), mode="w+", dtype=np.float64, shape=img.shape)
    dv = DeviceVolume(img)
    got = preprocess.equalize_adapthist(dv, kernel_size=ks, clip_limit=cl, nbins=nb, out=out)
    assert got is out and out.tobytes() == want.tobytes()
    assert preprocess.equalize_adapthist(img, kernel_size=ks, clip_limit=cl, nbins=nb).tobytes() == want.tobytes()


def test_float_image_outside_the_unit_range(gpu):
    img = np.linspace(0, 1.5, 16 * 16 * 16).reshape(16, 16, 16)
    with pytest.raises(ValueError, match="between -1 and 1"):
        preprocess.equalize_adapthist(img)


def test_remap_two_channels(gpu, fx, profile):
    from magellanmapper_amd.volume import DeviceVolume
    two = fx["two_in"]
    cases = {"all": dict(channel=None), "c1": dict(channel=[1]),
             "seq": dict(channel=None, kernel_size=(4, 6, 8), nbins=[64, 128], clip_limit=0.02)}
    for k, kw in cases.items():
        got = preprocess.remap_intensity(two, **dict(kw))
        assert got.dtype == two.dtype and np.array_equal(got, fx["remap2_%s" % k]), k
    got = preprocess.remap_intensity(DeviceVolume(two), channel=[1])
    assert got.tobytes() == fx["remap2_c1"].tobytes()
    # a single channel: the float64 result, the clip limit from the profile
    one = np.ascontiguousarray(two[..., 0])
    want = sup.equalize_adapthist(one, None, float(fx["settings"][3]), 256)
    assert np.array_equal(preprocess.remap_intensity(one), want)
    # the sequence-valued kernel on channel 0 means 4, on channel 1 it means 6: the float64 channels behind the cast
    for c, (ks, nb) in enumerate(((4, 64), (6, 128))):
        want = sup.equalize_adapthist(np.ascontiguousarray(two[..., c]), ks, 0.02, nb)
        assert np.array_equal(fx["remap2_seq"][..., c], want.astype(two.dtype))


def np_saturate(roi, channel, near_max):
    """``plot_3d.saturate_roi``, evaluated here in NumPy."""
    multichannel = roi.ndim > 3
    channels = (range(roi.shape[3]) if channel is None else channel) if multichannel else [0]
    out = None
    for chl in channels:
        s = config.get_roi_profile(chl)
        show = roi[..., chl] if multichannel else roi
        vmin, vmax = np.percentile(show, (s["clip_vmin"], s["clip_vmax"]))
        if vmin == vmax:
            sat = show
        else:
            vmax = max(vmax, near_max[chl] * s["max_thresh_factor"])
            # (float32 under the NumPy 2 rules: the float64 bounds make the clip float64)
            src = show.astype(np.float64) if show.dtype == np.float32 else show
            sat = (np.clip(src, vmin, vmax) - vmin) / (vmax - vmin)
        if multichannel:
            if out is None:
                out = np.zeros(roi.shape, dtype=sat.dtype)
            out[..., chl] = sat
        else:
            out = sat
    return out


@pytest.mark.parametrize("dtype", sup.DTYPES)
def test_saturate_roi(gpu, fx, profile, dtype, monkeypatch):
    monkeypatch.setattr(preprocess, "FLOAT32_RULES", "numpy2")
    img = sup.as_dtype(fx["in_u16_16_24_33"], dtype)
    near_max = [float(img.max()) * 2.0] if dtype == "uint8" else [0.0]      # (a ceiling that binds, and one that does not)
    monkeypatch.setattr(config, "near_max", near_max)
    got = preprocess.saturate_roi(img)
    want = np_saturate(img, None, near_max)
    assert got.dtype == want.dtype == np.float64 and np.array_equal(got, want)
    assert 0 < np.count_nonzero(got == 0) < got.size and np.count_nonzero((got > 0) & (got < 1)) > 0
    # explicit percentiles and factor
    got = preprocess.saturate_roi(img, clip_vmin=10, clip_vmax=90, max_thresh_factor=0.0)
    vmin, vmax = np.percentile(img, (10, 90))
    src = img.astype(np.float64) if img.dtype == np.float32 else img
    assert np.array_equal(got, (np.clip(src, vmin, vmax) - vmin) / (vmax - vmin))


def test_saturate_two_channels_and_quirks(gpu, fx, profile, monkeypatch):
    from magellanmapper_amd.volume import DeviceVolume
    two = fx["two_in"]
    for k, chl in (("all", None), ("c1", [1])):
        got = preprocess.saturate_roi(two, channel=chl)
        assert got.dtype == np.float64 and np.array_equal(got, np_saturate(two, chl, config.near_max))
        for c in range(2):
            want = fx["sat2_%s_vals%d" % (k, c)][np.searchsorted(fx["sat2_%s_uniq%d" % (k, c)], two[..., c])]
            assert np.array_equal(got[..., c], want)
    assert not preprocess.saturate_roi(two, channel=[1])[..., 0].any()
    assert preprocess.saturate_roi(DeviceVolume(two)).tobytes() == np_saturate(two, None, config.near_max).tobytes()
    # equal percentiles: the channel comes back unchanged, in its own dtype -- which a multichannel result then keeps
    const = np.full((8, 9, 10), 7, dtype=np.uint16)
    got = preprocess.saturate_roi(const)
    assert got.dtype == np.uint16 and np.array_equal(got, const)
    mixed = np.stack([const, np.ascontiguousarray(two[:8, :9, :10, 1])], axis=-1)
    want = np_saturate(mixed, None, config.near_max)
    got = preprocess.saturate_roi(mixed)
    assert got.dtype == want.dtype == np.uint16 and np.array_equal(got, want)


def test_preprocess_img_end_to_end(gpu, fx, profile, tmp_path):
    src = fx["in_u16_16_24_33"]
    want = sup.unpack_float(fx["chain_clahe"], fx["chain_uniq"], fx["chain_vals"])
    path = str(tmp_path / "stack.czi")
    res = transformer.preprocess_img(src[None], ["saturate", "remap"], None, path)
    assert sorted(os.listdir(tmp_path)) == ["stack_image5d.npy", "stack_meta.yml"]
    assert res.shape == (1,) + src.shape and res.dtype == np.float64 and np.array_equal(res[0], want)
    on_disk = np.load(str(tmp_path / "stack_image5d.npy"))
    assert on_disk.tobytes() == want[None].tobytes()
    md, _ = importer.load_metadata(str(tmp_path / "stack_meta.yml"))
    lows, highs = importer.calc_intensity_bounds(on_disk)
    assert md["near_min"] == [float(v) for v in lows] and md["near_max"] == [float(v) for v in highs]
    assert np.array_equal(md["near_min"], fx["chain_lows"]) and np.array_equal(md["near_max"], fx["chain_highs"])
    assert md["sizes"] == [list(res.shape)] and md["names"] == ["stack.czi"]
    # one task by name, two channels, one of them; an unknown name is skipped
    two = fx["two_in"]
    res = transformer.preprocess_img(two[None], ["sharpen", "remap"], [1], str(tmp_path / "two"))
    assert res.dtype == two.dtype and np.array_equal(res[0], fx["remap2_c1"])
    res = transformer.preprocess_img(two[None], "saturate", None, str(tmp_path / "sat"))
    assert np.array_equal(res[0], np_saturate(two, None, config.near_max))
