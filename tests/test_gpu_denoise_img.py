"""Whole-image denoise on the device (``equalize.denoise_roi``, the ``denoise`` task of ``transformer.preprocess_img``)
against the real reference's results (``tests/golden/denoise_img.npz``) and the CPU oracle, bit for bit."""
import os

import numpy as np
import pytest

import denoise_img_support as sup
from conftest import load_golden
from gpu_support import gpu  # noqa: F401
from magellanmapper_amd import config, device_image, equalize, importer, preprocess, transformer
from oracle import preprocess_oracle as ppo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def fx():
    return load_golden("denoise_img.npz")


@pytest.fixture()
def profiles(fx, monkeypatch):
    """scikit-image 0.18.3's RGB guess and the half kernel of the fixture's run; ``profiles(over)`` sets one default
    profile per entry of ``over`` and returns them as dicts for the oracle."""
    saved = (config.roi_profile, config.roi_profiles, config.near_max, config.resolutions)
    monkeypatch.setattr(preprocess, "RGB_GUESS", True)
    monkeypatch.setattr(preprocess, "GAUSS_WEIGHTS_OVERRIDE", np.ascontiguousarray(fx["gauss8_weights"][32:]))
    monkeypatch.setattr(ppo, "GAUSS_WEIGHTS", fx["gauss8_weights"])
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    yield lambda over: sup.set_profiles(config, config.setup_roi_profiles, over)
    config.roi_profile, config.roi_profiles, config.near_max, config.resolutions = saved


def _same(got, want):
    assert isinstance(got, np.ndarray) and got.dtype == want.dtype == np.float64 and got.shape == want.shape
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("name", list(sup.CASES))
def test_fixture_cases(gpu, fx, profiles, name):
    """Every stored case against what the real ``plot_3d.denoise_roi`` returned."""
    make, over, channel = sup.CASES[name]
    img = make()
    assert sup.sha(img) == str(fx[name + "_sha"])
    profiles(over)
    _same(preprocess.denoise_roi(img, channel), fx[name + "_out"])


# The shapes where the kernels can go wrong.  The march kernels (z and y passes) take 8 outputs per step, cut a thin
# image's marched axis into segments of at least 64 and put 256 columns into a workgroup; the x pass takes 512 outputs
# and a 32-voxel halo each side per wave.  (70, 140, 530) is no multiple of 8, 64, 256 or 512 on any axis and has a seam
# on every axis: z in two segments (40 + 30), y in three (48 + 48 + 44), x in two row segments (512 + 18).
SHAPES = [(1, 1, 1), (5, 33, 66), (34, 7, 3), (2, 130, 67), (70, 45, 131), (70, 140, 530)]
DTYPES = ["uint8", "uint16", "int16", "float64"]


def _input(shape, dtype):
    seed = 1000 + sum(shape)
    return sup.f64_image(seed, shape) if dtype == "float64" else sup.int_image(seed, shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_against_the_oracle(gpu, profiles, shape, dtype, monkeypatch):
    img = _input(shape, dtype)
    profs = profiles([{}])
    for rgb in ((True, False) if shape[2] == 3 else (True,)):
        monkeypatch.setattr(preprocess, "RGB_GUESS", rgb)
        # (the oracle guesses RGB as scikit-image 0.18 does; without the guess an (M, N, 3) image is blurred along x too)
        want = ppo.denoise_roi(img, profs) if rgb else _oracle_no_guess(img, profs[0])
        _same(preprocess.denoise_roi(img), want)


def _oracle_no_guess(img, prof):
    """``ppo.denoise_roi`` with all three axes blurred (scikit-image >= 0.19), from the oracle's own pieces."""
    from scipy import ndimage as ndi
    mean = np.mean(img)
    den = np.clip(img, prof["clip_min"], prof["clip_max"])
    blur = np.empty_like(den)
    src = den
    for axis in range(3):
        ndi.correlate1d(src, ppo.GAUSS_WEIGHTS[::-1], axis, blur, "nearest", 0.0, 0)
        src = blur
    den = den + (den - prof["unsharp_strength"] * blur)
    if mean > prof["erosion_threshold"]:
        out = np.empty_like(den)
        ndi.grey_erosion(den, footprint=ppo.OCTAHEDRON1, output=out)
        den = out
    return den


@pytest.mark.parametrize("over", [dict(unsharp_strength=0), dict(erosion_threshold=0),
                                  dict(unsharp_strength=0, erosion_threshold=0), dict(erosion_threshold=5.0)],
                         ids=["nounsharp", "noero", "clip_only", "thr_above"])
@pytest.mark.parametrize("dtype", ["uint16", "float64"])
def test_steps_switched_off(gpu, profiles, over, dtype):
    img = _input((5, 33, 66), dtype)
    profs = profiles([over])
    _same(preprocess.denoise_roi(img), ppo.denoise_roi(img, profs))


def test_gate_at_its_edge(gpu, profiles):
    """``erosion_threshold`` equal to NumPy's mean: not eroded; one ulp below: eroded."""
    img = sup.f64_image(21, sup.SHAPE)
    mean = float(np.mean(img))
    results = []
    for thr in (mean, float(np.nextafter(mean, 0))):
        profs = profiles([dict(erosion_threshold=thr)])
        want = ppo.denoise_roi(img, profs)
        stats = {}
        _same(equalize.denoise_roi(img, _stats=stats), want)
        results.append((want, stats["verdicts"]))
    assert not np.array_equal(results[0][0], results[1][0])
    assert results[0][1] == ["keep"] and results[1][1] == ["erode"]
    # two channels: each channel's view is strided, and NumPy's mean of it is what decides
    two = sup.f64_image(22, sup.SHAPE2)
    means = [float(np.mean(two[..., c])) for c in range(2)]
    wants = []
    for pick in (lambda m: m, lambda m: float(np.nextafter(m, 0))):
        profs = profiles([dict(erosion_threshold=pick(m)) for m in means])
        want = ppo.denoise_roi(two, profs)
        stats = {}
        _same(equalize.denoise_roi(two, _stats=stats), want)
        wants.append((want, stats["verdicts"]))
    assert not np.array_equal(wants[0][0][..., 0], wants[1][0][..., 0])
    assert not np.array_equal(wants[0][0][..., 1], wants[1][0][..., 1])
    assert wants[0][1] == ["keep", "keep"] and wants[1][1] == ["erode", "erode"]
    # the same from a resident volume: the host view is the C-contiguous download
    from magellanmapper_amd.volume import DeviceVolume
    _same(equalize.denoise_roi(DeviceVolume(two)), wants[1][0])


@pytest.mark.parametrize("over", [dict(), dict(erosion_threshold=0)], ids=["eroded", "noero"])
def test_slabs_memmap_resident_volume_and_keep(gpu, profiles, over, monkeypatch, tmp_path):
    from magellanmapper_amd.volume import DeviceVolume
    img = sup.f64_image(31, (10, 37, 70))
    want = ppo.denoise_roi(img, profiles([over]))
    monkeypatch.setattr(device_image, "SLAB_BYTES", 3 * img.shape[1] * img.shape[2] * 8)
    assert device_image.slab_step(img.shape, 8) == (3, 4)
    out = np.lib.format.open_memmap(str(tmp_path / "out.npy"), mode="w+", dtype=np.float64, shape=img.shape)
    got = preprocess.denoise_roi(img, _out=out)
    assert got is out and out.tobytes() == want.tobytes()
    _same(preprocess.denoise_roi(DeviceVolume(img)), want)
    kept = preprocess.denoise_roi(img, _keep=True)
    assert isinstance(kept, torch.Tensor) and kept.is_cuda and kept.dtype == torch.float64
    assert tuple(kept.shape) == img.shape and kept.cpu().numpy().tobytes() == want.tobytes()
    # the factory form of _out, as preprocess_img passes it
    made = []
    got = preprocess.denoise_roi(img, _out=lambda shape, dtype: made.append((shape, dtype)) or np.empty(shape, dtype))
    assert made == [(img.shape, np.dtype(np.float64))] and got.tobytes() == want.tobytes()


def test_two_channels(gpu, fx, profiles, monkeypatch):
    """Channels not named stay zero, the result is float64 whatever the voxel type, every channel has its profile."""
    from magellanmapper_amd.volume import DeviceVolume
    two = sup.f64_image(4, sup.SHAPE2)
    profs = profiles([{}, sup.CHANNEL1])
    monkeypatch.setattr(device_image, "SLAB_BYTES", 4 * two.shape[1] * two.shape[2] * 8)
    for channel, key in ((None, "two_all_out"), ([1], "two_c1_out")):
        got = preprocess.denoise_roi(DeviceVolume(two), channel)
        _same(got, fx[key])
        kept = preprocess.denoise_roi(two, channel, _keep=True)
        assert kept.dtype == torch.float64 and kept.cpu().numpy().tobytes() == fx[key].tobytes()
    assert not fx["two_c1_out"][..., 0].any()
    # per-channel profiles do what they say: channel 1 under channel 0's settings differs
    alone = ppo.denoise_roi(np.ascontiguousarray(two[..., 1]), profs[:1])
    assert not np.array_equal(alone, fx["two_all_out"][..., 1])
    ints = np.stack([sup.int_image(8, sup.SHAPE2[:3], np.uint16), sup.int_image(9, sup.SHAPE2[:3], np.uint16)], axis=-1)
    _same(preprocess.denoise_roi(ints, [1]), ppo.denoise_roi(ints, profs, [1]))


def test_preprocess_img_end_to_end(gpu, fx, profiles, tmp_path):
    profiles([{}])
    config.near_max = [float(v) for v in fx["chain_near_max"]]
    src = sup.chain_image()
    assert sup.sha(src) == str(fx["chain_sha"])
    want = fx["chain_out"]
    res = transformer.preprocess_img(src[None], ["saturate", "denoise"], None, str(tmp_path / "stack.czi"))
    assert sorted(os.listdir(tmp_path)) == ["stack_image5d.npy", "stack_meta.yml"]
    assert res.shape == want.shape and res.dtype == np.float64 and np.asarray(res).tobytes() == want.tobytes()
    on_disk = np.load(str(tmp_path / "stack_image5d.npy"))
    assert on_disk.tobytes() == want.tobytes()
    md, _ = importer.load_metadata(str(tmp_path / "stack_meta.yml"))
    assert np.array_equal(md["near_min"], fx["chain_lows"]) and np.array_equal(md["near_max"], fx["chain_highs"])
    assert md["sizes"] == [list(res.shape)] and md["names"] == ["stack.czi"]
    # three tasks: what the three functions give one after the other through the host (clip_max 0.5 keeps the unsharp
    # mask below 1: equalize_adapthist refuses a float image beyond it, as scikit-image does)
    profiles([dict(clip_max=0.5)])
    config.near_max = [float(v) for v in fx["chain_near_max"]]
    res = transformer.preprocess_img(src[None], ["saturate", "denoise", "remap"], None, str(tmp_path / "three"))
    step = preprocess.remap_intensity(preprocess.denoise_roi(preprocess.saturate_roi(src)))
    assert res.dtype == np.float64 and np.asarray(res[0]).tobytes() == step.tobytes()
    assert not np.array_equal(step, want[0])
    # a float64 image with the task alone
    profiles([{}])
    f64 = sup.f64_image(41, (6, 20, 40))
    res = transformer.preprocess_img(f64[None], "denoise", None, str(tmp_path / "f64"))
    _same(np.asarray(res[0]), ppo.denoise_roi(f64, [dict(config.roi_profile)]))
