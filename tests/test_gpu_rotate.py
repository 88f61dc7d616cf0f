"""Whole-image rotation on the device against the fixture made from the real reference (``cv_nd.rotate_nd``,
``transformer.rotate_img``, ``transformer.preprocess_img``): every comparison is ``np.array_equal``, no tolerance."""
import ctypes

import numpy as np
import pytest

import rotate_support as sup
from conftest import load_golden
from gpu_support import gpu  # noqa: F401
from magellanmapper_amd import _native as nat
from magellanmapper_amd import config, device_image, importer, preprocess, transformer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return load_golden("rotate.npz")


@pytest.fixture(scope="module")
def inputs():
    out = {}
    for kind, shape, seed, _, _, _ in sup.CASES:
        if (kind, shape, seed) not in out:
            out[(kind, shape, seed)] = sup.make_input(kind, shape, seed)
    return out


def _same(got, want):
    return isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and \
        np.array_equal(got, want)


@pytest.mark.parametrize("group", sorted({(c[0], c[1]) for c in sup.CASES}))
def test_fixture_cases(gpu, fx, inputs, group):
    """Every stored case of one voxel kind and shape (all axes, orders and angles of it) through ``rotate_nd``."""
    n = 0
    for case in sup.CASES:
        kind, shape, seed, axis, order, angle = case
        if (kind, shape) != group:
            continue
        img = inputs[(kind, shape, seed)]
        before = img.copy()
        got = preprocess.rotate_nd(img, angle, axis, order)
        assert _same(got, fx["rot_" + sup.case_name(case)]), case
        assert np.array_equal(img, before)
        n += 1
    assert n


def test_tensor_device_volume_and_2d_inputs(gpu, fx, inputs):
    import torch
    from magellanmapper_amd.volume import DeviceVolume
    for case in [c for c in sup.CASES if c[0] in ("u16m", "u16c2", "f32") and c[1] == sup.SMALL and c[5] == -30]:
        kind, shape, seed, axis, order, angle = case
        img = inputs[(kind, shape, seed)]
        want = fx["rot_" + sup.case_name(case)]
        # (torch has no uint16 arithmetic, but it holds and copies the voxels)
        t = torch.from_numpy(img.view(np.int16) if img.dtype == np.uint16 else img)
        if img.dtype != np.uint16:
            for src in (t, t.to(gpu)):
                got = preprocess.rotate_nd(src, angle, axis, order)
                assert isinstance(got, torch.Tensor) and got.device == src.device and got.dtype == src.dtype
                assert _same(got.cpu().numpy(), want)
        dv = DeviceVolume(img)
        got = preprocess.rotate_nd(dv, angle, axis, order)
        assert isinstance(got, DeviceVolume) and got.np_dtype == img.dtype and got.shape == dv.shape
        assert got.tensor.data_ptr() != dv.tensor.data_ptr()
        assert _same(got.tensor.cpu().numpy().view(img.dtype), want)
        assert np.array_equal(dv.tensor.cpu().numpy().view(img.dtype), img)        # (the source survives)
    # a 2-D image is one plane
    case = ("u16m", sup.SMALL, [c for c in sup.CASES if c[0] == "u16m" and c[1] == sup.SMALL][0][2], 0, 1, 45)
    img = inputs[case[:3]]
    want = fx["rot_" + sup.case_name(case)]
    for z in (0, 5):
        assert _same(preprocess.rotate_nd(np.ascontiguousarray(img[z]), 45), want[z])
    # int16 through a tensor: the torch dtype the voxels really have
    case = [c for c in sup.CASES if c[0] == "i16" and c[3:] == (1, 1, -30)][0]
    got = preprocess.rotate_nd(torch.from_numpy(inputs[case[:3]]).to(gpu), -30, 1, 1)
    assert _same(got.cpu().numpy(), fx["rot_" + sup.case_name(case)])


def test_chain_through_rotate_img(gpu, fx, monkeypatch):
    from magellanmapper_amd.volume import DeviceVolume
    src = sup.make_input("u16m", sup.SMALL, sup.CHAIN_SEED)
    for order in (0, 1):
        settings = {"rotation": sup.CHAIN, "resize": False, "order": order}
        assert _same(transformer.rotate_img(src, settings), fx["chain_o%d" % order])
        # `order` given overrides the settings'; the profile is read when no settings are given
        assert _same(transformer.rotate_img(src, dict(settings, order=1 - order), order=order), fx["chain_o%d" % order])
        monkeypatch.setattr(config, "atlas_profile", {"rotate": settings})
        assert _same(transformer.rotate_img(src), fx["chain_o%d" % order])
    dv = DeviceVolume(src)
    got = transformer.rotate_img(dv, {"rotation": sup.CHAIN, "resize": False, "order": 1})
    assert isinstance(got, DeviceVolume) and _same(got.tensor.cpu().numpy().view(np.uint16), fx["chain_o1"])
    assert np.array_equal(dv.tensor.cpu().numpy().view(np.uint16), src)
    two = sup.make_input("u16c2", sup.SMALL, sup.CHAIN_SEED + 1)
    assert _same(transformer.rotate_img(two, {"rotation": sup.CHAIN, "resize": False, "order": 1}), fx["chain_c2"])
    # no rotation: the one deliberate divergence -- a copy of the image, unchanged (the reference fails on None)
    for settings in ({"rotation": None, "resize": False, "order": 1}, {"rotation": (), "resize": False, "order": 1}):
        got = transformer.rotate_img(src, settings)
        assert _same(got, src) and not np.shares_memory(got, src)


def test_preprocess_img_end_to_end(gpu, fx, tmp_path, monkeypatch):
    saved = (config.roi_profile, config.roi_profiles, config.near_max, config.resolutions)
    try:
        config.setup_roi_profiles(None)
        s = fx["settings"]
        config.roi_profile.update(dict(clip_vmin=float(s[0]), clip_vmax=float(s[1]), max_thresh_factor=float(s[2]),
                                       adapt_hist_lim=float(s[3])))
        config.near_max = [float(v) for v in fx["near_max"]]
        config.resolutions = np.array([[1.0, 1.0, 1.0]])
        monkeypatch.setattr(config, "atlas_profile", {"rotate": {"rotation": sup.CHAIN, "resize": False, "order": 1}})
        src = sup.make_input("u16", sup.SMALL, sup.CHAIN_SEED + 2)
        assert sup.sha(src) == str(fx["e2e_sha"])
        path = str(tmp_path / "stack.czi")
        res = transformer.preprocess_img(src[None], ["saturate", "rotate"], None, path)
        assert res.shape == (1,) + src.shape and res.dtype == np.float64 and np.array_equal(res[0], fx["e2e_out"])
        on_disk = np.load(str(tmp_path / "stack_image5d.npy"), mmap_mode="r")
        assert on_disk.dtype == np.float64 and np.array_equal(on_disk[0], fx["e2e_out"])
        md, _ = importer.load_metadata(str(tmp_path / "stack_meta.yml"))
        assert np.array_equal(md["near_min"], fx["e2e_lows"]) and np.array_equal(md["near_max"], fx["e2e_highs"])
        assert md["sizes"] == [list(res.shape)]
        # the task alone, on the image as it arrives: the image's dtype leaves
        res = transformer.preprocess_img(src[None], "rotate", None, str(tmp_path / "rot"))
        assert res.dtype == np.uint16 and np.array_equal(res[0], sup.rotate_img(src, sup.CHAIN, 1))
        # and ahead of another task: the rotated image stays on the device for it
        res = transformer.preprocess_img(src[None], ["rotate", "saturate"], None, str(tmp_path / "rs"))
        assert res.dtype == np.float64 and res.shape == (1,) + src.shape
    finally:
        config.roi_profile, config.roi_profiles, config.near_max, config.resolutions = saved


def _call(src_t, dst_t, shape3, n_chl, s_strides, d_strides, axis, order, angle, src_off=0, dst_off=0):
    """The two entry points on explicit views of two device tensors (int16 tensors hold uint16 voxels: torch fills
    and compares those, the kernels are told the voxels' real type)."""
    import torch
    L = nat.lib()
    code = nat.MMX_U16 if src_t.dtype == torch.int16 else nat.NP_TO_MMX[device_image.np_dtype_of(src_t)]
    es = src_t.element_size()
    sv = nat.DsView(src_t.data_ptr() + src_off * es, code, 0, *s_strides)
    dv = nat.DsView(dst_t.data_ptr() + dst_off * es, code, 0, *d_strides)
    rows, cols = sup.plane_shape(shape3, axis)
    m = np.ascontiguousarray(preprocess.rotation_matrix(rows, cols, angle).reshape(-1))
    bounds = torch.empty(2 * shape3[axis], dtype=torch.float64, device=src_t.device)
    stream = torch.cuda.current_stream().cuda_stream
    s_elems, d_elems = src_t.numel() - src_off, dst_t.numel() - dst_off
    rc = L.mmx_rotate_minmax(ctypes.byref(sv), s_elems, *shape3, n_chl, axis, bounds.data_ptr(), stream)
    if rc:
        return rc, None
    rc = L.mmx_rotate_warp(ctypes.byref(sv), s_elems, ctypes.byref(dv), d_elems, *shape3, n_chl, axis,
                           nat.as_double_ptr(m), order, bounds.data_ptr(), stream)
    torch.cuda.current_stream().synchronize()
    return rc, bounds.cpu().numpy().reshape(-1, 2)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_views_through_their_strides(gpu, axis):
    """A channel of an interleaved image (stride_x = channels), an axis-swapped view and a destination with strides of
    its own: the entry points address all of them through ``mmx_ds_view``; and what they check before a launch."""
    import torch
    two = sup.make_input("u16c2", (6, 13, 70), 5)
    d_two = torch.from_numpy(two.view(np.int16)).to(gpu)
    shape3 = two.shape[:3]
    for c in (0, 1):
        want = sup.rotate_nd(np.ascontiguousarray(two[..., c]), -30, axis, 1)
        dst = torch.full((2,) + shape3, -7, dtype=torch.int16, device=gpu)
        st = d_two.stride()
        rc, bounds = _call(d_two, dst, shape3, 1, st[:3], dst[1].stride(), axis, 1, -30, src_off=c,
                           dst_off=dst[1].storage_offset())
        assert rc == 0
        assert np.array_equal(dst[1].cpu().numpy().view(np.uint16), want)
        assert (dst[0] == -7).all()
        planes = np.moveaxis(two[..., c], axis, 0).reshape(shape3[axis], -1)
        assert np.array_equal(bounds, np.stack([planes.min(1), planes.max(1)], 1).astype(np.float64))
    # the (y, z, x) view of the image: the same memory, axes 0 and 1 swapped by strides
    img = np.ascontiguousarray(two[..., 1])
    d_img = torch.from_numpy(img.view(np.int16)).to(gpu)
    swapped = np.swapaxes(img, 0, 1)
    want = sup.rotate_nd(swapped, 45, axis, 1)
    dst = torch.zeros(swapped.shape, dtype=torch.int16, device=gpu)
    st = d_img.stride()
    rc, _ = _call(d_img, dst, swapped.shape, 1, (st[1], st[0], st[2]), dst.stride(), axis, 1, 45)
    assert rc == 0 and np.array_equal(dst.cpu().numpy().view(np.uint16), want)
    # both channels at once, the clip range over both
    dst = torch.zeros(two.shape, dtype=torch.int16, device=gpu)
    rc, bounds = _call(d_two, dst, shape3, 2, d_two.stride()[:3], dst.stride()[:3], axis, 1, -30)
    assert rc == 0 and np.array_equal(dst.cpu().numpy().view(np.uint16), sup.rotate_nd(two, -30, axis, 1))
    # refused before a launch: a box that reaches beyond either buffer, the source as its own destination, an order
    # that is not built, float32 at order 1
    L = nat.lib()
    big = (shape3[0] + 1,) + tuple(shape3[1:])
    dst.fill_(3)
    rc, _ = _call(d_two, dst, big, 2, d_two.stride()[:3], dst.stride()[:3], axis, 1, -30)
    assert rc != 0 and "argument" in L.mmx_strerror(rc).decode().lower()
    rc, _ = _call(d_two, d_two, shape3, 2, d_two.stride()[:3], d_two.stride()[:3], axis, 1, -30)
    assert rc != 0
    rc, _ = _call(d_two, dst, shape3, 2, d_two.stride()[:3], dst.stride()[:3], axis, 3, -30)
    assert rc != 0
    f_src, f_dst = torch.zeros(shape3, device=gpu), torch.zeros(shape3, device=gpu)
    rc, _ = _call(f_src, f_dst, shape3, 1, f_src.stride(), f_dst.stride(), axis, 1, -30)
    assert rc != 0
    assert (dst == 3).all()
