"""GPU tests of the intensity bounds: the radix select (``mmx_order_stats``) through the C ABI and through
``DeviceVolume.order_stats`` against ``np.sort``, and ``importer.calc_intensity_bounds`` / ``measure_near_bounds``
against the fixture of the real reference and ``np.percentile`` of the running NumPy.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden
from test_bounds_host import BOUNDS, NAMES, fixture_volume
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PCTS = [tuple(float(v) for v in p) for p in BOUNDS["pcts"]]


@pytest.fixture
def clean_config():
    from magellanmapper_amd import config
    yield config
    config.setup_roi_profiles(None)
    config.near_max = [-1.0]
    config.near_min = [0.0]


def _channel(vol, c):
    return vol[..., c] if vol.ndim == 4 else vol


def _want(vol, c, groups, ranks):
    """np.sort(group.ravel())[rank] for every group (NaNs last, as np.sort puts them)."""
    ch = _channel(vol, c)
    ranks = np.broadcast_to(np.asarray(ranks, dtype=np.int64), (len(groups), 4))
    out = np.empty((len(groups), 4))
    for g, (z0, z1) in enumerate(groups):
        out[g] = np.sort(ch[z0:z1].ravel())[ranks[g]].astype(np.float64)
    return out


def _abi(vol, c, groups, ranks, dev):
    """The same through the bare C ABI (no DeviceVolume): ``(status, stats, nan flags)``."""
    from magellanmapper_amd import _native as nat
    L = nat.lib()
    t = torch.from_numpy(np.ascontiguousarray(vol)).to(dev)
    n_chl = vol.shape[3] if vol.ndim == 4 else 1
    code = {np.dtype(np.uint8): nat.MMX_U8, np.dtype(np.uint16): nat.MMX_U16, np.dtype(np.float32): nat.MMX_F32,
            np.dtype(np.float64): nat.MMX_F64}[vol.dtype]
    nz, ny, nx = vol.shape[:3]
    v = nat.Volume(t.data_ptr() + c * vol.dtype.itemsize, code, 0, ny * nx * n_chl, nx * n_chl, n_chl)
    table = np.zeros(len(groups), dtype=nat.RANK_GROUP_DTYPE)
    table["z0"] = [g[0] for g in groups]
    table["z1"] = [g[1] for g in groups]
    table["rank"] = np.broadcast_to(np.asarray(ranks, dtype=np.int64), (len(groups), 4))
    d_groups = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
    d_stats = torch.full((len(groups), 4), -7.0, dtype=torch.float64, device=dev)
    d_nan = torch.full((len(groups),), -7, dtype=torch.int32, device=dev)
    wb = int(L.mmx_order_stats_workspace(len(groups)))
    d_work = torch.empty(wb, dtype=torch.uint8, device=dev)
    rc = L.mmx_order_stats(v, nz, ny, nx, d_groups.data_ptr(), table.ctypes.data, len(groups), d_stats.data_ptr(),
                           d_nan.data_ptr(), d_work.data_ptr(), wb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, d_stats.cpu().numpy(), d_nan.cpu().numpy()


def _rank_sets(groups, plane, seed):
    """Per group: the ranks of (0.5, 99.5), seeded ranks, 0 and n - 1, four equal ranks -- as (name, (G, 4))."""
    from magellanmapper_amd import importer
    rng = np.random.default_rng(seed)
    n = np.array([(z1 - z0) * plane for z0, z1 in groups], dtype=np.int64)
    sets = {"pct": np.array([importer._bounds_ranks(int(k), 0.5, 99.5)[0] for k in n]),
            "seeded": np.array([rng.integers(0, k, 4) for k in n]),
            "ends": np.stack([np.zeros_like(n), n - 1, n - 1, np.zeros_like(n)], axis=1),
            "equal": np.repeat(np.array([rng.integers(0, k) for k in n])[:, None], 4, axis=1)}
    return sets.items()


def _group_tables(nz):
    mixed = [(0, 1), (min(1, nz - 1), min(4, nz)), (0, nz), (nz - 1, nz)]
    return {"planes": [(z, z + 1) for z in range(nz)], "whole": [(0, nz)], "mixed": mixed}.items()


def _check_volume(vol, dev, seed=0):
    from magellanmapper_amd.volume import DeviceVolume
    n_chl = vol.shape[3] if vol.ndim == 4 else 1
    dv = DeviceVolume(vol)
    plane = vol.shape[1] * vol.shape[2]
    for c in range(n_chl):
        for gname, groups in _group_tables(vol.shape[0]):
            for rname, ranks in _rank_sets(groups, plane, seed):
                want = _want(vol, c, groups, ranks)
                got, has_nan = dv.order_stats(c, ranks, groups)
                np.testing.assert_array_equal(got, want, err_msg=f"python {gname} {rname} channel {c}")
                assert not has_nan.any()
                rc, got_abi, nan_abi = _abi(vol, c, groups, ranks, dev)
                assert rc == 0
                np.testing.assert_array_equal(got_abi, want, err_msg=f"abi {gname} {rname} channel {c}")
                assert not nan_abi.any()


@pytest.mark.parametrize("name", NAMES)
def test_order_stats_fixture_volumes(gpu, name):
    """Per-plane groups, one whole-volume group and a mixed table (ranges of 1, 3 and all planes in one call)."""
    _check_volume(fixture_volume(name), gpu)


def test_order_stats_float32(gpu):
    """The fourth voxel type (its order statistics do not depend on the NumPy release; its percentiles would)."""
    _check_volume(fixture_volume("f64").astype(np.float32), gpu, seed=1)
    rng = np.random.default_rng(2)
    vol = rng.normal(0, 1, (5, 21, 34)).astype(np.float32)
    vol[0, 0, :4] = [-0.0, 0.0, np.inf, -np.inf]
    _check_volume(vol, gpu, seed=3)


@pytest.mark.parametrize("dtype", ["uint8", "uint16", "float32", "float64"])
def test_order_stats_edge_planes(gpu, dtype):
    """A constant plane; a plane of two values whose boundary sits exactly on a rank; a 37 x 53 plane (no multiple
    of the load width); a one-voxel plane."""
    from magellanmapper_amd.volume import DeviceVolume
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(7)
    const = np.full((3, 37, 53), 77, dtype=dtype)
    got, _ = DeviceVolume(const).order_stats(0, [0, 5, 1000, 37 * 53 - 1])
    np.testing.assert_array_equal(got, np.full((3, 4), 77.0))
    # two values: ranks [0, b) hold `lo`, [b, n) hold `hi`; ranks b - 1 and b straddle the boundary
    n = 37 * 53
    for b in (1, 980, n - 1):
        plane = np.full(n, 200, dtype=dtype)
        plane[:b] = 100
        rng.shuffle(plane)
        vol = plane.reshape(1, 37, 53)
        ranks = [b - 1, b, 0, n - 1]
        got, _ = DeviceVolume(vol).order_stats(0, ranks)
        np.testing.assert_array_equal(got, _want(vol, 0, [(0, 1)], ranks))
        np.testing.assert_array_equal(got[0], [100.0, 200.0, 100.0, 200.0])
    if dtype.kind == "u":
        odd = rng.integers(0, np.iinfo(dtype).max + 1, (4, 37, 53)).astype(dtype)
    else:
        odd = (rng.normal(0, 1, (4, 37, 53)) * 1e3).astype(dtype)
    _check_volume(odd, gpu, seed=8)
    one = odd[:3, :1, :1].copy()
    got, _ = DeviceVolume(one).order_stats(0, [0, 0, 0, 0])
    np.testing.assert_array_equal(got, np.repeat(one.reshape(3, 1).astype(np.float64), 4, axis=1))
    rc, got, _ = _abi(one, 0, [(0, 3)], [0, 1, 2, 2], gpu)
    assert rc == 0
    np.testing.assert_array_equal(got[0], np.sort(one.ravel())[[0, 1, 2, 2]].astype(np.float64))


def test_order_stats_strided_channel_and_z_off(gpu):
    """A (z, y, x, 2) image reads its channel at stride 2; a DeviceVolume holding planes [z_off, z_off + n) answers in
    the coordinates of the whole volume."""
    from magellanmapper_amd.volume import DeviceVolume
    vol = fixture_volume("u16_2ch")
    _check_volume(vol, gpu, seed=4)
    big = fixture_volume("u16")
    part = DeviceVolume(big[5:17], z_off=5, full_shape=big.shape)
    plane = big.shape[1] * big.shape[2]
    ranks = [0, 17, plane // 2, plane - 1]
    got, _ = part.order_stats(0, ranks)
    np.testing.assert_array_equal(got, _want(big, 0, [(z, z + 1) for z in range(5, 17)], ranks))
    groups = [(5, 17), (9, 12), (16, 17)]
    got, _ = part.order_stats(0, ranks, groups)
    np.testing.assert_array_equal(got, _want(big, 0, groups, ranks))
    with pytest.raises(ValueError):
        part.order_stats(0, ranks, [(4, 6)])
    with pytest.raises(ValueError):
        part.order_stats(0, [0, 0, 0, plane], [(5, 6)])


def test_order_stats_float64_specials(gpu):
    """-0.0, negatives and infinities sort as np.sort sorts them (-0.0 == 0.0 counts as equal)."""
    rng = np.random.default_rng(9)
    vol = rng.normal(0, 5, (4, 19, 23))
    vol[0].ravel()[:8] = [-0.0, 0.0, -np.inf, np.inf, -1e-310, 1e-310, -1e308, 1e308]
    vol[1] = -np.abs(vol[1])
    vol[2].ravel()[::3] = 0.0
    vol[2].ravel()[1::3] = -0.0
    _check_volume(vol, gpu, seed=10)


def test_nan_plane_is_flagged_and_yields_nan(gpu):
    from magellanmapper_amd import importer
    from magellanmapper_amd.volume import DeviceVolume
    vol = fixture_volume("f64").copy()
    vol[2, 7, 11] = np.nan
    vol[4, 0, 0] = -np.nan
    dv = DeviceVolume(vol)
    plane = vol.shape[1] * vol.shape[2]
    ranks = [3, 4, plane - 2, plane - 1]
    got, has_nan = dv.order_stats(0, ranks)
    np.testing.assert_array_equal(has_nan, [False, False, True, False, True, False])
    np.testing.assert_array_equal(got, _want(vol, 0, [(z, z + 1) for z in range(6)], ranks))
    assert np.isnan(got[2, 3]) and np.isnan(got[4, 3]) and not np.isnan(got[[0, 1, 3, 5]]).any()
    rc, got_abi, nan_abi = _abi(vol, 0, [(z, z + 1) for z in range(6)], ranks, gpu)
    assert rc == 0
    np.testing.assert_array_equal(nan_abi, [0, 0, 1, 0, 1, 0])
    np.testing.assert_array_equal(got_abi, got)
    lows, highs = importer._percentiles_of_groups(dv, 0, [(z, z + 1) for z in range(6)], 0.5, 99.5)
    for z in range(6):
        with np.errstate(all="ignore"):
            want = np.percentile(vol[z], (0.5, 99.5))
        np.testing.assert_array_equal([lows[z], highs[z]], want)
    assert np.isnan(lows[2]) and np.isnan(highs[4]) and not np.isnan(lows[[0, 1, 3, 5]]).any()
    near_min, near_max = importer.measure_near_bounds(vol)
    want_lo = [np.percentile(p, 0.5) for p in vol]
    want_hi = [np.percentile(p, 99.5) for p in vol]
    np.testing.assert_array_equal(near_min, [min(want_lo)])
    np.testing.assert_array_equal(near_max, [max(want_hi)])


@pytest.mark.parametrize("name", NAMES)
def test_bounds_match_reference_and_numpy(gpu, name):
    """calc_intensity_bounds and measure_near_bounds == the real reference's (fixture) == np.percentile here."""
    from magellanmapper_amd import importer
    from magellanmapper_amd.stack_detect import Image5d
    from magellanmapper_amd.volume import DeviceVolume
    vol = fixture_volume(name)
    n_chl = vol.shape[3] if vol.ndim == 4 else 1
    for k, (lower, upper) in enumerate(PCTS):
        lows, highs = importer.calc_intensity_bounds(vol[None], lower, upper)
        assert isinstance(lows, list) and isinstance(highs, list) and len(lows) == n_chl
        np.testing.assert_array_equal(lows, BOUNDS[f"{name}_whole_lows_{k}"])
        np.testing.assert_array_equal(highs, BOUNDS[f"{name}_whole_highs_{k}"])
        want = np.array([np.percentile(_channel(vol, c), (lower, upper)) for c in range(n_chl)])
        np.testing.assert_array_equal(lows, want[:, 0])
        np.testing.assert_array_equal(highs, want[:, 1])
        # one plane at a time, as the reference's metadata upgrade calls it (importer.py:577-581)
        plane_lows, plane_highs = [], []
        for z in range(vol.shape[0]):
            lo, hi = importer.calc_intensity_bounds(vol[z], lower, upper, dim_channel=2)
            plane_lows.append(lo)
            plane_highs.append(hi)
        np.testing.assert_array_equal(np.array(plane_lows), BOUNDS[f"{name}_plane_lows_{k}"])
        np.testing.assert_array_equal(np.array(plane_highs), BOUNDS[f"{name}_plane_highs_{k}"])
        near_mins, near_maxs = importer.calc_near_intensity_bounds([], [], plane_lows, plane_highs)
        np.testing.assert_array_equal(np.asarray(near_mins), BOUNDS[f"{name}_near_min_{k}"])
        np.testing.assert_array_equal(np.asarray(near_maxs), BOUNDS[f"{name}_near_max_{k}"])
        for img in (vol, vol[None] if vol.ndim == 4 else vol, Image5d(vol[None]), DeviceVolume(vol)):
            near_min, near_max = importer.measure_near_bounds(img, lower, upper)
            assert isinstance(near_min, list) and len(near_min) == n_chl
            np.testing.assert_array_equal(near_min, BOUNDS[f"{name}_near_min_{k}"])
            np.testing.assert_array_equal(near_max, BOUNDS[f"{name}_near_max_{k}"])
        chls = [_channel(vol, c) for c in range(n_chl)]
        np.testing.assert_array_equal(near_min, [min(np.percentile(p, lower) for p in ch) for ch in chls])
        np.testing.assert_array_equal(near_max, [max(np.percentile(p, upper) for p in ch) for ch in chls])
    dv = DeviceVolume(vol)
    lows, highs = importer.calc_intensity_bounds(dv)
    np.testing.assert_array_equal(lows, BOUNDS[f"{name}_whole_lows_0"])
    np.testing.assert_array_equal(highs, BOUNDS[f"{name}_whole_highs_0"])


def test_float32_percentiles_and_oversize_images_are_refused(gpu, monkeypatch):
    from magellanmapper_amd import device_image, importer
    vol32 = fixture_volume("f64").astype(np.float32)
    with pytest.raises(NotImplementedError):
        importer.calc_intensity_bounds(vol32[None])
    with pytest.raises(NotImplementedError):
        importer.measure_near_bounds(vol32)
    monkeypatch.setattr(device_image, "free_bytes", lambda: 1000)
    with pytest.raises(ValueError, match="whole-image"):
        importer.calc_intensity_bounds(fixture_volume("u16")[None])


def test_memory_mapped_image_walked_in_chunks(gpu, tmp_path, monkeypatch):
    """A read-only memory-mapped (t, z, y, x) .npy as importer.read_file hands it over, the chunk size forced small: at
    least three z-chunks; the resident result."""
    from magellanmapper_amd import importer, volume
    from magellanmapper_amd.stack_detect import Image5d
    vol = fixture_volume("u16")
    path = tmp_path / "img_image5d.npy"
    np.save(path, vol[None])
    mm = np.load(path, mmap_mode="r")
    assert isinstance(mm, np.memmap) and not mm.flags.writeable
    want = importer.measure_near_bounds(vol)
    chunks = []
    real = volume.DeviceVolume

    class Spy(real):
        def __init__(self, image, *a, **kw):
            chunks.append((kw.get("z_off", 0), image.shape[0]))
            super().__init__(image, *a, **kw)

    monkeypatch.setattr(volume, "DeviceVolume", Spy)
    monkeypatch.setattr(importer, "BOUNDS_CHUNK_BYTES", 5 * vol[0].nbytes)
    got = importer.measure_near_bounds(Image5d(mm))
    assert chunks == [(0, 5), (5, 5), (10, 5), (15, 5), (20, 4)]
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[0], BOUNDS["u16_near_min_0"])
    np.testing.assert_array_equal(got[1], BOUNDS["u16_near_max_0"])
    # the streamed upload path of a chunk (a slab upload in flight while it is counted)
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 2 * vol[0].nbytes)
    del chunks[:]
    got = importer.measure_near_bounds(Image5d(mm))
    assert len(chunks) == 5
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])


def test_measured_near_max_drives_stock_profile_detection(gpu, clean_config, tmp_path, monkeypatch):
    """measure_near_bounds(assign=True), then a stock-profile detect_blobs_blocks == the oracle run with the same
    near_max; the max_thresh rule bites (tiles whose upper percentile lies below near_max * max_thresh_factor) and the
    table differs from the one near_max = [-1.0] gives."""
    from magellanmapper_amd import importer, preprocess, stack_detect, synth
    from oracle import magmap_oracle as mmo
    config = clean_config
    monkeypatch.chdir(tmp_path)
    vol = synth.make_volume(5, (40, 96, 112), 12)
    config.setup_roi_profiles(None)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "bounds"
    config.near_max = [-1.0]
    prof = dict(config.roi_profile)
    assert prof["denoise_size"] == 25 and prof["max_thresh_factor"] == 0.5
    near_min, near_max = importer.measure_near_bounds(vol, assign=True)
    assert config.near_max is near_max and config.near_min is near_min
    np.testing.assert_array_equal(near_min, [min(np.percentile(p, 0.5) for p in vol)])
    np.testing.assert_array_equal(near_max, [max(np.percentile(p, 99.5) for p in vol)])
    # the rule bites: tiles whose own upper percentile lies below the floor
    _, infos = preprocess.preprocess_roi(vol, (25, 25, 25), near_max=[-1.0], return_info=True)
    floor = near_max[0] * prof["max_thresh_factor"]
    (_, info), = infos
    own_vmax = info["vmax"].copy()
    bites = own_vmax < floor
    assert len(own_vmax) == 40 and int(np.sum(bites)) >= 1
    _, infos = preprocess.preprocess_roi(vol, (25, 25, 25), near_max=near_max, return_info=True)
    np.testing.assert_array_equal(infos[0][1]["vmax"], np.maximum(own_vmax, floor))
    _, _, blobs = stack_detect.detect_blobs_blocks("bounds", stack_detect.Image5d(vol[None]), None, None, None,
                                                   False, False, True, False)
    want, _ = mmo.detect_blobs_blocks(vol, None, [prof], config.resolutions, near_max=list(near_max))
    without, _ = mmo.detect_blobs_blocks(vol, None, [prof], config.resolutions, near_max=[-1.0])
    assert want is not None and without is not None
    assert want.shape != without.shape or not np.array_equal(want, without)
    np.testing.assert_array_equal(blobs.blobs, want)


def test_bad_arguments_return_codes_and_write_nothing(gpu):
    from magellanmapper_amd import _native as nat
    vol = fixture_volume("u8")
    n = vol.shape[1] * vol.shape[2]
    L = nat.lib()
    for groups, ranks in (([(0, 1)], [0, 0, 0, n]), ([(0, 1)], [-1, 0, 0, 0]), ([(2, 2)], [0, 0, 0, 0]),
                          ([(3, 2)], [0, 0, 0, 0]), ([(0, 10)], [0, 0, 0, 0]), ([(-1, 1)], [0, 0, 0, 0]),
                          ([(0, 1), (8, 9), (1, 2)], [[0] * 4, [0, 0, n, 0], [0] * 4])):
        rc, stats, nan = _abi(vol, 0, groups, ranks, gpu)
        assert rc == 1, (groups, ranks)             # MMX_ERR_ARG
        assert (stats == -7.0).all() and (nan == -7).all()
    # a short workspace
    t = torch.from_numpy(vol).to(gpu)
    v = nat.Volume(t.data_ptr(), nat.MMX_U8, 0, n, vol.shape[2], 1)
    table = np.zeros(2, dtype=nat.RANK_GROUP_DTYPE)
    table["z1"] = 1
    d_groups = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(gpu)
    d_stats = torch.full((2, 4), -7.0, dtype=torch.float64, device=gpu)
    d_nan = torch.full((2,), -7, dtype=torch.int32, device=gpu)
    wb = int(L.mmx_order_stats_workspace(2))
    assert wb > 0 and int(L.mmx_order_stats_workspace(0)) == 0
    d_work = torch.empty(wb, dtype=torch.uint8, device=gpu)
    args = (v, vol.shape[0], vol.shape[1], vol.shape[2], d_groups.data_ptr(), table.ctypes.data, 2,
            d_stats.data_ptr(), d_nan.data_ptr(), d_work.data_ptr())
    assert L.mmx_order_stats(*args, wb - 1, None) == 4      # MMX_ERR_WORKSPACE
    assert L.mmx_order_stats(v, vol.shape[0], vol.shape[1], vol.shape[2], None, table.ctypes.data, 2,
                             d_stats.data_ptr(), d_nan.data_ptr(), d_work.data_ptr(), wb, None) == 1
    torch.cuda.synchronize()
    assert (d_stats.cpu().numpy() == -7.0).all() and (d_nan.cpu().numpy() == -7).all()
    assert L.mmx_order_stats(*args, wb, None) == 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(d_stats.cpu().numpy(), np.full((2, 4), float(vol[0].min())))


def test_full_size_benchmark_volume(gpu):
    """Per-plane bounds of the 1024 x 2048 x 2048 benchmark volume: 32 seeded planes against np.percentile, near_min /
    near_max against the device's own per-plane values; whole-image mode (one group of 4.3e9 voxels: 64-bit counts)
    against np.partition on the host at its ranks."""
    from magellanmapper_amd import importer, synth
    from magellanmapper_amd.volume import DeviceVolume
    shape = (1024, 2048, 2048)
    t = synth.make_volume_device(shape, 3, gpu)
    dv = DeviceVolume(t)
    groups = [(z, z + 1) for z in range(shape[0])]
    lows, highs = importer._percentiles_of_groups(dv, 0, groups, 0.5, 99.5)
    assert lows.shape == (1024,) and highs.shape == (1024,)
    rng = np.random.default_rng(32)
    for z in sorted(int(v) for v in rng.choice(shape[0], 32, replace=False)):
        plane = t[z].cpu().numpy()
        np.testing.assert_array_equal([lows[z], highs[z]], np.percentile(plane, (0.5, 99.5)), err_msg=f"plane {z}")
    near_min, near_max = importer.measure_near_bounds(dv)
    np.testing.assert_array_equal(near_min, [lows.min()])
    np.testing.assert_array_equal(near_max, [highs.max()])
    n = int(np.prod(shape, dtype=np.int64))
    assert n > 2 ** 32 - 1
    ranks, lo_g, hi_g = importer._bounds_ranks(n, 0.5, 99.5)
    got, has_nan = dv.order_stats(0, ranks, [(0, shape[0])])
    host = t.cpu().numpy().reshape(-1)
    del t, dv
    host.partition(np.unique(ranks))
    np.testing.assert_array_equal(got[0], host[ranks].astype(np.float64))
    assert not has_nan.any()
