"""GPU tests of the down-sampling stage (``transformer.downsample`` / ``transpose_img`` /
``preprocess.rescale_resize`` over ``csrc/mmx_downsample.hip``) against the CPU chain of ``transform_support`` and the
real reference's fixture.  Every comparison is BIT FOR BIT.  The shapes are the smallest at which each mechanism can go
wrong: 3 x 3 x 3 ragged chunks, extents that round at .5, a unit-thick remainder plane, a radius beyond the extent, an
axis that keeps its length, strided sources, layers that go up one at a time.
"""
import numpy as np
import pytest
import yaml

from conftest import load_golden
from gpu_support import gpu  # noqa: F401
import transform_support as ts

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLD = load_golden("transform.npz")
SHAPE = (13, 29, 27)
MP = (5, 12, 10)
_VOLS = {}
_WANT = {}


def vol_of(dtype, channels=None):
    key = (dtype, channels)
    if key not in _VOLS:
        _VOLS[key] = ts.make_volume(11, SHAPE + ((channels,) if channels else ()), dtype)
        _VOLS[key].setflags(write=False)
    return _VOLS[key]


def want_of(dtype, channels=None, **kw):
    """The CPU chain's result, computed once per case and shared."""
    key = (dtype, channels, tuple(sorted(kw.items())))
    if key not in _WANT:
        _WANT[key] = ts.downsample_cpu(vol_of(dtype, channels), **kw)
        _WANT[key].setflags(write=False)
    return _WANT[key]


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.dtype, want.shape)
    assert np.array_equal(got, want), "max |diff| %g at %d voxels" % (
        np.abs(got.astype(np.float64) - want).max(), (got != want).sum())


@pytest.mark.parametrize("dtype", ts.DTYPES)
def test_rescale_quarter_every_dtype(gpu, dtype):
    """No anti-aliasing: 3 x 3 x 3 chunks with ragged remainders, img_as_float on load, per-chunk clip."""
    from magellanmapper_amd import transformer as tr
    got = tr.downsample(vol_of(dtype), rescale=0.25, max_pixels=MP)
    assert got.shape == (3, 7, 6) and got.dtype == (np.float32 if dtype == "float32" else np.float64)
    same(got, want_of(dtype, rescale=0.25, max_pixels=MP))


def test_rescale_quarter_two_channels_share_the_clip_range(gpu):
    """Channels interleaved in the file (x stride 2), one clip range per chunk over both (an interpolated value cannot
    leave its own channel's range by more than a rounding, so the range shows only in the last bit)."""
    from magellanmapper_amd import transformer as tr
    got = tr.downsample(vol_of("uint16", 2), rescale=0.25, max_pixels=MP)
    assert got.shape == (3, 7, 6, 2)
    same(got, want_of("uint16", 2, rescale=0.25, max_pixels=MP))


@pytest.mark.parametrize("dtype", ["uint16", "float32"])
def test_rescale_half_rounds_at_point_five(gpu, dtype):
    """5 -> 2 (2.5), 3 -> 2 (1.5), 7 -> 4 (3.5): extents that round half to even."""
    from magellanmapper_amd import transformer as tr
    got = tr.downsample(vol_of(dtype), rescale=0.5, max_pixels=MP)
    assert got.shape == (6, 14, 14)
    same(got, want_of(dtype, rescale=0.5, max_pixels=MP))


@pytest.mark.parametrize("dtype", ts.DTYPES)
def test_target_size_anti_aliased(gpu, dtype):
    """The anti-aliased path with the reference's chunk rule: the conversion fused into the first pass (integer
    types), float32 stores per pass (float32), chunks of 5 -> 1 whose radius (8) folds the mirror more than once."""
    from magellanmapper_amd import transformer as tr
    got = tr.downsample(vol_of(dtype), target_size=(9, 10, 4), max_pixels=MP)
    assert got.shape == (3, 9, 9)
    same(got, want_of(dtype, target_size=(9, 10, 4), max_pixels=MP))


def test_rescale_with_a_target_size(gpu):
    """Both given: chunks evened out as for the target size (y 10 / 10 / 9, x 9 / 9 / 9), rescaled by the factor."""
    from magellanmapper_amd import transformer as tr
    got = tr.downsample(vol_of("uint16"), rescale=0.5, target_size=(9, 10, 4), max_pixels=MP)
    assert got.shape == (6, 14, 12)
    same(got, want_of("uint16", rescale=0.5, target_size=(9, 10, 4), max_pixels=MP))


def test_target_size_two_channels(gpu):
    from magellanmapper_amd import transformer as tr
    same(tr.downsample(vol_of("uint8", 2), target_size=(9, 10, 4), max_pixels=MP),
         want_of("uint8", 2, target_size=(9, 10, 4), max_pixels=MP))


def test_unit_thick_remainder_plane(gpu):
    """7 planes in chunks of 3 leave a plane of thickness 1: it stays in 'reflect' mode and SciPy returns its single
    sample along z (with ``rescale=0.25`` such a plane rounds to nothing: the plan refuses it)."""
    from magellanmapper_amd import transformer as tr
    vol = ts.make_volume(12, (7, 13, 11), "uint16")
    for kw in (dict(target_size=(4, 6, 3)), dict(rescale=0.5)):
        if "rescale" in kw:
            with pytest.raises(ValueError, match="chunk 2 along axis 0"):
                tr.downsample(vol, max_pixels=(3, 12, 10), **kw)
            continue
        got = tr.downsample(vol, max_pixels=(3, 12, 10), **kw)
        assert got.shape[0] == 3
        same(got, ts.downsample_cpu(vol, max_pixels=(3, 12, 10), **kw))
    with pytest.raises(ValueError, match=r"chunk 2 along axis 0 \(z\), 1 voxels"):
        tr.downsample(ts.make_volume(12, (11, 29, 27), "uint16"), rescale=0.25, max_pixels=MP)


@pytest.mark.parametrize("dtype", ["float64", "uint16", "float32"])
def test_radius_beyond_the_extent(gpu, dtype):
    """3 x 4 x 5 shrunk to 1 x 2 x 2: sigma 1 / 0.5 / 0.75, radius 4 / 2 / 3 against extents 3 / 4 / 5."""
    from magellanmapper_amd import preprocess
    chunk = ts.make_volume(13, (3, 4, 5), dtype)
    same(preprocess.rescale_resize(chunk, (1, 2, 2)), ts.resize_chunk_cpu(chunk, (1, 2, 2), True))


def test_one_axis_shrinks(gpu):
    """Only x shrinks: z and y get sigma 0 and no pass (their picks are left to the zoom tables), anti-aliasing is
    still on; and a chunk that grows along one axis while it shrinks along another."""
    from magellanmapper_amd import preprocess
    chunk = ts.make_volume(14, (5, 12, 10), "uint16")
    same(preprocess.rescale_resize(chunk, (5, 12, 3)), ts.resize_chunk_cpu(chunk, (5, 12, 3), True))
    same(preprocess.rescale_resize(chunk, (2, 12, 10)), ts.resize_chunk_cpu(chunk, (2, 12, 10), True))
    same(preprocess.rescale_resize(chunk, (7, 5, 10)), ts.resize_chunk_cpu(chunk, (7, 5, 10), True))


def test_rescale_resize_options(gpu):
    """``anti_aliasing`` given explicitly either way, ``order=1`` / ``mode="reflect"`` named, two channels."""
    from magellanmapper_amd import preprocess
    chunk = ts.make_volume(15, (8, 12, 16), "int16")
    same(preprocess.rescale_resize(chunk, 0.25, anti_aliasing=True, order=1, mode="reflect"),
         ts.resize_chunk_cpu(chunk, (2, 3, 4), True))
    same(preprocess.rescale_resize(chunk, (2, 3, 4), anti_aliasing=False), ts.resize_chunk_cpu(chunk, (2, 3, 4), False))
    two = ts.make_volume(16, (8, 12, 16, 2), "uint8")
    same(preprocess.rescale_resize(two, 0.5, True), ts.resize_chunk_cpu(two, (4, 6, 8), False))
    same(preprocess.rescale_resize(two, (3, 5, 4)), ts.resize_chunk_cpu(two, (3, 5, 4), True))


def test_sparse_equals_dense_and_the_existing_kernels(gpu):
    """The picked passes against (a) the same passes evaluated everywhere and (b) the existing composition
    ``mmx_gauss_axis_batch`` + ``mmx_resize_batch_as`` on a float64 copy of the converted chunk, and the CPU chain."""
    from magellanmapper_amd import blob_log as bl, preprocess, transformer as tr
    vol = vol_of("uint16")
    want = want_of("uint16", target_size=(9, 10, 4), max_pixels=MP)
    same(tr.downsample(vol, target_size=(9, 10, 4), max_pixels=MP, sparse=True), want)
    same(tr.downsample(vol, target_size=(9, 10, 4), max_pixels=MP, sparse=False), want)
    chunk = ts.make_volume(17, (12, 20, 18), "uint16")
    new = (4, 6, 5)
    conv = ts.convert_to_float(chunk)
    rs = preprocess.Rescaler(np.ones(3), [0])
    rs.set_blocks([(0, 0, 0)], [chunk.shape], [new])
    rs.run(bl.DeviceVolume(conv), 0, [(0, 0, 0)], [new], 0)
    dense = rs.fetch([new])[0]
    sparse = preprocess.rescale_resize(chunk, new)
    same(sparse, dense)
    same(sparse, ts.resize_chunk_cpu(chunk, new, True))


@pytest.mark.parametrize("plane", ["xz", "yz"])
def test_planes_swap_by_strides(gpu, plane):
    """Strided sources: the swapped volume is read where the file's voxels lie."""
    from magellanmapper_amd import transformer as tr
    mp = (10, 5, 12)
    got = tr.downsample(vol_of("uint16"), rescale=0.25, plane=plane, max_pixels=mp)
    same(got, want_of("uint16", rescale=0.25, plane=plane, max_pixels=mp))
    got = tr.downsample(vol_of("uint16", 2), target_size=(6, 4, 5), plane=plane, max_pixels=mp)
    same(got, want_of("uint16", 2, target_size=(6, 4, 5), plane=plane, max_pixels=mp))


def test_fixtures_of_the_real_reference(gpu, monkeypatch):
    """(i) ``cv_nd.rescale_resize(chunk, 0.25, anti_aliasing=False)`` and (ii) ``cv_nd.rescale_resize(float64 chunk,
    (4, 6, 5))`` of the real reference through the device ((ii) with the half kernels its SciPy built)."""
    from magellanmapper_amd import preprocess, transformer as tr
    for dt in ("uint8", "uint16", "int16", "float64"):
        same(preprocess.rescale_resize(GOLD["noaa_%s_in" % dt], 0.25, anti_aliasing=False), GOLD["noaa_%s_out" % dt])
    monkeypatch.setattr(tr, "AA_WEIGHTS_OVERRIDE", {float(GOLD["aa_sigma"][a]): GOLD["aa_w%d" % a] for a in range(3)})
    same(preprocess.rescale_resize(GOLD["aa_in"], (4, 6, 5)), GOLD["aa_out"])


@pytest.mark.parametrize("plane", [None, "xz", "yz"])
def test_layer_by_layer_equals_resident(gpu, plane, tmp_path):
    """A byte budget below the image: the layers of chunks go up one at a time (z-, y- or x-boxes of the file, from a
    read-only memory map as the importer hands it over) and give the resident run's result; a volume already on the
    device gives it too."""
    from magellanmapper_amd import blob_log as bl, transformer as tr
    mp = MP if plane is None else (10, 5, 12)
    path = str(tmp_path / "vol.npy")
    np.save(path, vol_of("uint16", 2))
    mm = np.load(path, mmap_mode="r")
    for kw in (dict(rescale=0.25), dict(target_size=(6, 4, 5))):
        want = want_of("uint16", 2, plane=plane, max_pixels=mp, **kw)
        same(tr.downsample(mm, plane=plane, max_pixels=mp, layer_bytes=1, **kw), want)
        same(tr.downsample(mm, plane=plane, max_pixels=mp, **kw), want)
    same(tr.downsample(bl.DeviceVolume(vol_of("uint16", 2)), rescale=0.25, plane=plane, max_pixels=mp),
         want_of("uint16", 2, plane=plane, max_pixels=mp, rescale=0.25))


@pytest.mark.parametrize("plane", [None, "xz"])
def test_layers_streamed_beside_the_kernels(gpu, plane, tmp_path, monkeypatch):
    """The layers of a read-only memory map above the streaming threshold (lowered to nothing here) go up on the copy
    stream: the constructor returns with the copy in flight, layer k + 1 is started before layer k's kernels and
    waited for only ahead of its own -- z-boxes and y-boxes of the file, read where they lie; the resident result."""
    from magellanmapper_amd import transformer as tr, volume
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    mp = MP if plane is None else (10, 5, 12)
    path = str(tmp_path / "vol.npy")
    np.save(path, vol_of("uint16", 2))
    mm = np.load(path, mmap_mode="r")
    events, upload, run = [], tr._upload, tr._run_batch

    def spy_upload(*a):
        src = upload(*a)
        events.append(("upload", a[2], src.keep._upload is not None))
        return src

    def spy_run(src, *a, **k):
        events.append(("run", a[1][0][0][0]))
        return run(src, *a, **k)
    monkeypatch.setattr(tr, "_upload", spy_upload)
    monkeypatch.setattr(tr, "_run_batch", spy_run)
    for kw in (dict(rescale=0.25), dict(target_size=(6, 4, 5))):
        del events[:]
        same(tr.downsample(mm, plane=plane, max_pixels=mp, layer_bytes=1, **kw),
             want_of("uint16", 2, plane=plane, max_pixels=mp, **kw))
        order = [(e[0], e[1]) for e in events]
        starts = sorted({e[1] for e in events})
        assert len(starts) == 3
        want_order = [("upload", starts[0])]
        for k, z in enumerate(starts):
            if k + 1 < len(starts):
                want_order.append(("upload", starts[k + 1]))
            want_order.append(("run", z))
        assert order == want_order, order
        assert all(e[2] for e in events if e[0] == "upload"), "a layer went up synchronously"


def test_transpose_img_end_to_end(gpu, tmp_path):
    """``<base>_image5d.npy`` + metadata in, ``<base>_scale0pt25_image5d.npy`` + metadata out: paths, shape, dtype,
    every voxel, and the YAML -- resolutions, sizes, scaling, plane, near_min / near_max of the result."""
    from magellanmapper_amd import config, importer, transformer as tr
    base = str(tmp_path / "brain")
    path_img, path_meta = importer.make_filenames(base)
    vol = vol_of("uint16")
    np.save(path_img, vol[None])
    res = np.array([[5.0, 1.5, 1.25]])
    importer.save_image_info(path_meta, ["brain"], [(1,) + SHAPE], res, 2.0, 1.5, [10.0], [6000.0])
    try:
        out = tr.transpose_img(base, None, rescale=0.25)
        want = ts.downsample_cpu(vol, rescale=0.25)             # (one 100 x 500 x 500 chunk holds the volume)
        out_img, out_meta = importer.make_filenames(base, modifier="scale0pt25")
        assert out_img == str(tmp_path / "brain_scale0pt25_image5d.npy")
        assert out_meta == str(tmp_path / "brain_scale0pt25_meta.yml")
        saved = np.load(out_img, mmap_mode="r")
        assert saved.shape == (1, 3, 7, 7) and saved.dtype == np.float64 and out.shape == saved.shape
        same(np.asarray(saved[0]), want)
        with open(out_meta) as f:
            md = yaml.safe_load(f)
        assert md["resolutions"] == [[20.0, 6.0, 5.0]] and np.array_equal(config.resolutions, res * 4)
        assert md["sizes"] == [[1, 3, 7, 7]]
        assert md["scaling"] == [3 / 13, 7 / 29, 7 / 27]
        assert md["plane"] is None and md["magnification"] == 2.0 and md["zoom"] == 1.5 and md["names"] == ["brain"]
        assert md["near_min"] == [float(np.percentile(want, 0.5))]
        assert md["near_max"] == [float(np.percentile(want, 99.5))]
        # a plane swap and a target size: swapped resolutions scaled by the shape ratios, the modifier of both
        out = tr.transpose_img(base, None, plane="xz", target_size=(9, 4, 10))
        want = ts.downsample_cpu(vol, target_size=(9, 4, 10), plane="xz")
        out_img, out_meta = importer.make_filenames(base, modifier="planeXZresized(9,4,10)")
        same(np.asarray(np.load(out_img, mmap_mode="r")[0]), want)
        assert want.shape == (10, 4, 9)
        with open(out_meta) as f:
            md = yaml.safe_load(f)
        assert md["plane"] == "xz" and md["sizes"] == [[1, 10, 4, 9]]
        assert md["resolutions"] == [list(np.array([1.5, 5.0, 1.25]) * (np.array([29, 13, 27]) / np.array([10, 4, 9])))]
        assert md["scaling"] == [10 / 29, 4 / 13, 9 / 27]
    finally:
        config.resolutions = None
        config.near_min, config.near_max = [0.0], [-1.0]
        config.magnification = config.zoom = 1.0


def test_transpose_img_plane_only_flips(gpu, tmp_path):
    """Without rescaling the planes are copied as the reference copies them: swapped, then ``np.fliplr``."""
    from magellanmapper_amd import config, importer, transformer as tr
    base = str(tmp_path / "img")
    path_img, path_meta = importer.make_filenames(base)
    vol = vol_of("uint16")
    np.save(path_img, vol[None])
    importer.save_image_info(path_meta, ["img"], [(1,) + SHAPE], np.array([[5.0, 1.5, 1.25]]), 1.0, 1.0, [0.0], [1.0])
    try:
        out = tr.transpose_img(base, None, plane="yz")
        assert np.array_equal(out[0], np.fliplr(ts.swap_plane(vol, "yz"))) and out.dtype == np.uint16
        assert np.array_equal(config.resolutions, [[1.25, 5.0, 1.5]])
    finally:
        config.resolutions = None
        config.near_min, config.near_max = [0.0], [-1.0]


MMX_ERR_ARG, MMX_ERR_UNSUPPORTED = 1, 5           # mmx_status (include/mmx.h)
NO_SUCH_DTYPE = (-1, 5)                            # below and above the five mmx_dtype codes


@pytest.mark.parametrize("code", NO_SUCH_DTYPE)
def test_a_code_that_names_no_voxel_type_is_refused_and_nothing_is_written(gpu, code):
    """The two entry points take views of their own (``mmx_ds_view``): a dtype code that names no voxel type -- of the
    source, of the destination or of the raw image -- is ``MMX_ERR_UNSUPPORTED`` before anything is launched; the
    same calls with the codes in place run."""
    import ctypes
    from gpu_support import stream_ptr
    from magellanmapper_amd import _native as nat
    L = nat.lib()
    f64, unsupported, bad_argument = nat.MMX_F64, MMX_ERR_UNSUPPORTED, MMX_ERR_ARG

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(gpu)

    src = torch.arange(64, dtype=torch.float64, device=gpu)                 # a 4 x 4 x 4 source
    out = torch.full((8,), 7.0, dtype=torch.float64, device=gpu)            # a 2 x 2 x 2 destination
    rec = np.zeros(1, dtype=nat.DS_CHUNK_DTYPE)
    rec[0] = (0, 0, 4, 4, 4, 2, 2, 2, 0, 0, 0, 0, (0, 0))
    idx = np.array([[0, 1], [2, 3]], dtype=np.int32)
    wts = np.full((2, 2), 0.5)
    mm = torch.tensor([0.0, 100.0], dtype=torch.float64, device=gpu)
    d_rec, d_idx, d_wts = dev(rec), dev(idx), dev(wts)

    def zoom(src_code, dst_code, raw_code):
        s = nat.DsView(src.data_ptr(), src_code, 0, 16, 4, 1)
        t = nat.DsView(out.data_ptr(), dst_code, 0, 4, 2, 1)
        return L.mmx_ds_zoom_batch(ctypes.byref(s), ctypes.byref(t), 8, d_rec.data_ptr(), rec.ctypes.data, 1,
                                   d_idx.data_ptr(), idx.ctypes.data, 2, d_wts.data_ptr(), mm.data_ptr(), raw_code,
                                   stream_ptr())

    buf = torch.full((32,), 7.0, dtype=torch.float64, device=gpu)           # 2 picked planes of 4 x 4
    prec = np.zeros(1, dtype=nat.DS_CHUNK_DTYPE)
    prec[0] = (0, 0, 4, 4, 4, 2, 4, 4, 0, 0, 0, 0, (0, 0))
    pick, radius, w = np.array([1, 2], dtype=np.int32), np.zeros(1, dtype=np.int32), np.ones((1, 1))
    d_prec, d_pick, d_radius, d_w = dev(prec), dev(pick), dev(radius), dev(w)

    def picked(src_code):
        s = nat.DsView(src.data_ptr(), src_code, 0, 16, 4, 1)
        return L.mmx_ds_gauss_pick_batch(ctypes.byref(s), d_prec.data_ptr(), prec.ctypes.data, 1, 0, d_w.data_ptr(),
                                         d_radius.data_ptr(), radius.ctypes.data, 1, d_pick.data_ptr(),
                                         pick.ctypes.data, 2, 4, 16, 32, buf.data_ptr(), stream_ptr())

    assert zoom(code, f64, f64) == unsupported
    assert zoom(f64, code, f64) == unsupported
    assert zoom(f64, f64, code) == unsupported
    assert picked(code) == unsupported
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((buf == 7.0).all()), "a refused call wrote"
    # a table entry outside the source, a destination too short: refused by the host-side checks
    idx[1, 1] = 4
    assert zoom(f64, f64, f64) == bad_argument
    idx[1, 1] = 3
    pick[1] = 4
    assert picked(f64) == bad_argument
    pick[1] = 2
    assert zoom(f64, f64, f64) == 0 and picked(f64) == 0
    torch.cuda.synchronize()
    cube = np.arange(64.0).reshape(4, 4, 4)
    want = sum(0.125 * cube[np.ix_(idx[:, a], idx[:, b], idx[:, c])] for a in (0, 1) for b in (0, 1) for c in (0, 1))
    assert np.array_equal(out.cpu().numpy().reshape(2, 2, 2), want)
    assert np.array_equal(buf.cpu().numpy().reshape(2, 4, 4), cube[1:3])
