"""GPU parity tests of the intensity co-localisation: ``mmx_coloc_means``
through the C ABI + the host thresholds against the golden vectors of the real reference's
``colocalizer.colocalize_blobs`` and against the CPU oracle."""
import numpy as np
import pytest

from conftest import load_golden
from test_oracle_golden import COLOC, coloc_roi, coloc_thresh
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("case", [str(n) for n in COLOC["names"]])
def test_colocalize_blobs_matches_reference(gpu, case):
    from magellanmapper_amd import colocalizer
    got = colocalizer.colocalize_blobs(coloc_roi(COLOC, case), COLOC[case + "_blobs"], coloc_thresh(COLOC, case))
    want = COLOC[case + "_colocs"]
    if want.shape[0] == 0:
        assert got is None
        return
    assert got.dtype == np.uint8
    np.testing.assert_array_equal(got, want)


def test_means_are_bit_equal_to_numpy(gpu):
    """The per-blob means themselves (float64 image: NumPy's pairwise order matters), including
    crowded blobs whose balls overlap and blobs at the ROI corners."""
    import ctypes
    from magellanmapper_amd import _native as nat, blob_log as bl
    from oracle import coloc_oracle
    from scipy import ndimage as ndi
    rng = np.random.default_rng(8)
    roi = rng.random((20, 24, 28, 2)) * 3 - 1
    n = 60
    pts = np.stack([rng.integers(0, s, n) for s in roi.shape[:3]], axis=1)
    pts[:6] = [[0, 0, 0], [19, 23, 27], [0, 1, 1], [5, 5, 5], [5, 6, 6], [5, 5, 5]]
    chl = rng.integers(0, 2, n)
    chl[3:6] = 0
    dvol = bl.DeviceVolume(roi)
    blocks, _ = bl._make_blocks(dvol, 0, [(0, 0, 0)], [roi.shape[:3]])
    d_blocks = bl._to_device_bytes(blocks, gpu)
    rows = np.zeros((n, 5), np.int32)
    rows[:, 1:4] = pts
    rows[:, 4] = chl
    d_rows = torch.from_numpy(rows.reshape(-1)).to(gpu)
    d_off = torch.tensor([0, n], dtype=torch.int32, device=gpu)
    d_mean = torch.empty(n, dtype=torch.float64, device=gpu)
    d_cnt = torch.empty(n, dtype=torch.int32, device=gpu)
    for c in range(2):
        vol = dvol.view(c, False)
        nat.check(nat.lib().mmx_coloc_means(ctypes.byref(vol), d_blocks.data_ptr(), 1, d_rows.data_ptr(),
                                            d_off.data_ptr(), n, d_mean.data_ptr(), d_cnt.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream), "coloc")
        got, cnt = d_mean.cpu().numpy(), d_cnt.cpu().numpy()
        for bc in range(2):                       # label volume of blob channel bc, as the reference builds it
            sel = np.where(chl == bc)[0]
            mask = -np.ones(roi.shape[:3], dtype=int)
            mask[pts[sel, 0], pts[sel, 1], pts[sel, 2]] = sel
            mask = ndi.grey_dilation(mask, footprint=coloc_oracle.ball(2))
            for b in sel:
                vox = roi[mask == b, c]
                assert cnt[b] == vox.size
                if vox.size:
                    assert got[b] == np.mean(vox), (b, c)
                else:
                    assert np.isnan(got[b])


def test_stack_coloc_many_batches_matches_oracle(gpu, monkeypatch, tmp_path):
    """Several device batches (tiny workspace budget), co-localisation on, against the oracle."""
    import functools
    from magellanmapper_amd import blob_log as bl, config, stack_detect
    from oracle import magmap_oracle as mmo
    monkeypatch.chdir(tmp_path)
    g = load_golden("stack_coloc_2ch.npz")
    roi = g["roi"]
    config.setup_roi_profiles(None)
    config.roi_profile.update(num_sigma=3, segment_size=24, denoise_size=None)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "coloc"
    monkeypatch.setattr(bl, "blob_log_blocks", functools.partial(bl.blob_log_blocks, budget_bytes=6 << 20))
    _, _, blobs = stack_detect.detect_blobs_blocks("coloc", stack_detect.Image5d(roi[None]), None, None,
                                                   None, False, False, True, True)
    assert stack_detect.StackDetector.last_stats.n_blocks > 20
    want, st = mmo.detect_blobs_blocks(roi, None, [dict(config.roi_profile)], config.resolutions, coloc=True)
    np.testing.assert_array_equal(blobs.blobs, want)
    np.testing.assert_array_equal(blobs.colocalizations, st["colocs"])
    assert st["colocs"][:, 1].any()


def test_single_channel_coloc_is_switched_off_like_the_reference(gpu, monkeypatch, tmp_path):
    from magellanmapper_amd import config, stack_detect
    monkeypatch.chdir(tmp_path)
    roi = load_golden("stack_coloc_2ch.npz")["roi"][..., 0]
    config.setup_roi_profiles(None)
    config.roi_profile.update(num_sigma=3, segment_size=40, denoise_size=None)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    _, _, blobs = stack_detect.detect_blobs_blocks("c1", stack_detect.Image5d(roi[None]), None, None,
                                                   None, False, False, True, True)
    assert blobs.colocalizations is None and blobs.blobs.shape[1] == 8
    with pytest.raises(ValueError):        # np.hstack((segments, None)) in the reference's detect_sub_roi
        stack_detect.StackDetector.detect_sub_roi((0, 0, 0), (0, 0, 0), (0, 0, 0), None, None, None,
                                                  roi, None, coloc=True)


# ------------------------------------------------------------------------- match-based co-localisation
def _match_config(seg, res=(1.0, 1.0, 1.0)):
    from magellanmapper_amd import config
    config.setup_roi_profiles(None)
    config.roi_profile.update(segment_size=int(seg), num_sigma=3, denoise_size=None)
    config.resolutions = np.array([res])
    config.cpus = 4


def _frame_arrays(bm):
    df = bm.df
    if df is None or not len(df):
        return np.empty((0, 8)), np.empty((0, 8)), np.empty(0)
    return np.vstack(df["Blob1"]), np.vstack(df["Blob2"]), np.asarray(df["Distance"], dtype=float)


def test_find_closest_blobs_cdist_matches_reference(gpu):
    """Device distance matrix + native assignment against the real ``verifier.find_closest_blobs_cdist``
    (``scipy`` cdist + linear_sum_assignment): pairs and float64 distances identical."""
    from magellanmapper_amd import verifier
    g = load_golden("match.npz")
    for k in range(int(g["n_lsap"])):
        thresh = None if np.isnan(g["lsap%d_thresh" % k]) else float(g["lsap%d_thresh" % k])
        rows, cols, dists = verifier.find_closest_blobs_cdist(g["lsap%d_a" % k], g["lsap%d_b" % k], thresh,
                                                              g["lsap%d_scaling" % k])
        np.testing.assert_array_equal(rows, g["lsap%d_rows" % k])
        np.testing.assert_array_equal(cols, g["lsap%d_cols" % k])
        np.testing.assert_array_equal(dists, g["lsap%d_dists" % k])


def test_match_blobs_roi_matches_reference(gpu):
    """All five outputs of ``verifier.match_blobs_roi`` (flags as the reference leaves them) with the device distance
    matrix: anisotropic tolerances, a tiny ROI, base blobs flagged 0 / 1 outside the core."""
    from test_host_logic import _check_match_blobs_roi
    from magellanmapper_amd import detector, verifier
    _match_config(40)
    try:
        _check_match_blobs_roi(load_golden("match.npz"), verifier)
    finally:
        detector.Blobs(np.ones((1, 4))).format_blobs()


def test_colocalize_blobs_match_matches_reference(gpu):
    from magellanmapper_amd import colocalizer, detector
    g = load_golden("match.npz")
    _match_config(40)
    try:
        for k in range(3):
            blobs = detector.Blobs(g["roi_table"].copy())
            got = colocalizer.colocalize_blobs_match(blobs, tuple(g["roi%d_offset" % k]), tuple(g["roi%d_size" % k]),
                                                     g["roi_tol"])
            keys = [tuple(int(v) for v in key) for key in g["roi%d_keys" % k]]
            assert sorted(got) == keys
            for key in keys:
                for name, arr in zip(("blob1", "blob2", "dist"), _frame_arrays(got[key])):
                    np.testing.assert_array_equal(arr, g["roi%d_%d_%d_%s" % (k, *key, name)])
        assert colocalizer.colocalize_blobs_match(None, (0, 0, 0), (1, 1, 1), g["roi_tol"]) is None
    finally:
        detector.Blobs(np.ones((1, 4))).format_blobs()


@pytest.mark.parametrize("name", ["stackA", "stackB"])
def test_stack_colocalizer_matches_reference(gpu, name):
    """``StackColocalizer.colocalize_stack`` (2 and 3 channels, isotropic and anisotropic voxels): every match of
    the real reference, in its order, with its float64 distance."""
    from magellanmapper_amd import colocalizer, detector
    g = load_golden("match.npz")
    _match_config(g[name + "_segment_size"], tuple(g[name + "_res"]))
    try:
        blobs = detector.Blobs(g[name + "_table"].copy())
        got = colocalizer.StackColocalizer.colocalize_stack(tuple(int(v) for v in g[name + "_shape"]), blobs)
        keys = [tuple(int(v) for v in key) for key in g[name + "_keys"]]
        assert sorted(got) == keys
        for key in keys:
            assert isinstance(got[key], colocalizer.BlobMatch)
            for col, arr in zip(("blob1", "blob2", "dist"), _frame_arrays(got[key])):
                np.testing.assert_array_equal(arr, g["%s_%d_%d_%s" % (name, *key, col)])
            assert got[key].get_mean_coords().shape == (len(got[key].df), 3)
    finally:
        detector.Blobs(np.ones((1, 4))).format_blobs()


def test_channels_as_lanes_of_one_pipeline_equal_channel_after_channel(gpu, monkeypatch):
    """``blob_log.blob_log_lanes`` (every channel a lane of ONE pipeline, batch b through all channels before batch b + 1)
    against the channels detected one after the other: a two-channel stack whose channels detect with DIFFERENT profiles
    (scales, threshold, overlap), with per-block preprocessing and co-localisation, small batches (several per channel) --
    identical final tables and flags, both equal to the oracle."""
    from magellanmapper_amd import blob_log as bl, config, stack_detect, synth
    from oracle import magmap_oracle as mmo
    shape = (60, 130, 140)
    c0 = synth.make_volume(21, shape, 90)
    c1 = np.maximum(synth.make_volume(22, shape, 70).astype(np.int32), (c0.astype(np.int32) * 6) // 10).astype(np.uint16)
    vol = np.stack((c0, c1), axis=-1)
    config.setup_roi_profiles(["default"] * 2)
    base = dict(segment_size=44, denoise_size=25, num_sigma=3)
    for p in config.roi_profiles:
        p.update(base)
    config.roi_profile.update(base)
    config.roi_profiles[1].update(num_sigma=4, min_sigma_factor=2.5, max_sigma_factor=4.5, detection_threshold=0.2, overlap=0.3)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "lanes"
    config.near_max = [-1.0, -1.0]
    monkeypatch.setattr(bl, "BUDGET_BYTES", 40 << 20)          # (a few blocks per batch: several batches per channel)
    try:
        got = {}
        for batch_major in (True, False):
            monkeypatch.setattr(bl, "BATCH_MAJOR", batch_major)
            sizes = []
            real = bl._enqueue_detect
            monkeypatch.setattr(bl, "_enqueue_detect", lambda *a, **k: (sizes.append((a[1].channel, len(a[2]))), real(*a, **k))[1])
            _, _, blobs = stack_detect.detect_blobs_blocks("lanes", stack_detect.Image5d(vol[None]), None, None, None,
                                                           False, False, True, True)
            monkeypatch.setattr(bl, "_enqueue_detect", real)
            chans = [c for c, _ in sizes]
            assert len(sizes) >= 6 and set(chans) == {0, 1}
            if batch_major:
                assert chans[:4] == [0, 1, 0, 1]                # batch 0 in both channels, then batch 1 ...
            else:
                assert chans == sorted(chans)                   # all of channel 0, then all of channel 1
            got[batch_major] = (blobs.blobs, blobs.colocalizations)
        np.testing.assert_array_equal(got[True][0], got[False][0])
        np.testing.assert_array_equal(got[True][1], got[False][1])
        profiles = [dict(p) for p in config.roi_profiles]
        want, stages = mmo.detect_blobs_blocks(vol, [0, 1], profiles, config.resolutions, near_max=[-1.0, -1.0], coloc=True)
        assert len(want) > 100 and set(np.unique(want[:, 6])) == {0.0, 1.0}
        np.testing.assert_array_equal(got[True][0], want)
        np.testing.assert_array_equal(got[True][1], stages["colocs"])
    finally:
        config.setup_roi_profiles(None)
