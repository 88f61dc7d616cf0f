"""Whole-image rotation on the device: ``cv_nd.rotate_nd`` and the chain of ``transformer.rotate_img``.

Mirror of ``cv_nd.rotate_nd`` (reference magmap/cv/cv_nd.py:81-144): ``skimage.transform.rotate(plane, angle,
order=order, mode="constant", preserve_range=True)`` of every plane along ``axis``, written back into an array of the
image's dtype -- bit for bit what scikit-image 0.18 computes (``csrc/mmx_rotate.hip`` states the arithmetic).  One
rotation is two streaming passes over the resident volume: every plane's minimum and maximum (the clip range, order 1
only) and the warp into a second buffer; a chain of rotations ping-pongs between two buffers and leaves the device once.

The matrix ``T(center) R(angle) T(-center)`` comes from :func:`rotation_matrix`, in scalar arithmetic: scikit-image's own
3 x 3 products go through BLAS, whose fused multiply-adds differ between NumPy builds in the last bit.

Stated limits (``NotImplementedError``, from the arguments alone, ahead of any launch):

* ``resize=True``: the enlarged plane's translation is the minimum corner of ``tform.inverse(corners)``, which goes
  through LAPACK (``np.linalg.inv``) and a matrix product whose last bits differ between NumPy builds;
* any ``order`` other than 0 or 1;
* float32 images at order 1 (scikit-image's float32 interpolation is not reproduced by any float32 or mixed evaluation
  that was tried); float32 at order 0 is built, with float32 coordinates;
* voxel types other than uint8, uint16, int16, float32, float64;
* an image whose source and destination do not fit the device.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Tuple

import numpy as np

try:
    import torch
except ImportError:  # pragma: no cover
    torch = None

from . import _native as nat
from . import equalize

#: bytes of one z-slab of a result on its way into a host array handed as the output
SLAB_BYTES = 256 << 20


def rotation_matrix(rows: int, cols: int, angle: float) -> np.ndarray:
    """The first two rows, ``(2, 3)`` float64, of the matrix ``skimage.transform.rotate`` hands to ``warp`` for a
    ``rows x cols`` plane: ``T(center) R(angle) T(-center)`` with ``center = (cols / 2 - 0.5, rows / 2 - 0.5)``, every
    entry in scalar arithmetic (``math.cos`` / ``math.sin``: NumPy may pick a vectorised routine on another CPU).
    Output pixel ``(tr, tc)`` reads the source at ``c = M00 tc + M01 tr + M02``, ``r = M10 tc + M11 tr + M12``."""
    cx, cy = int(cols) / 2 - 0.5, int(rows) / 2 - 0.5
    a = float(np.deg2rad(angle))
    c, s = math.cos(a), math.sin(a)
    # (-s + 0.0: the products of the three matrices leave +0.0 where the sine is zero)
    return np.array([[c, -s + 0.0, c * (-cx) + (-s) * (-cy) + cx],
                     [s, c, s * (-cx) + c * (-cy) + cy]], dtype=np.float64)


def check_args(dtype, order, resize, what: str = "rotate_nd") -> None:
    """Every refusal that follows from the arguments alone."""
    if resize:
        raise NotImplementedError(f"{what}: resize=True is not built: the enlarged plane's offset goes through LAPACK "
                                  f"(np.linalg.inv of the transform and a matrix product), whose last bits differ "
                                  f"between NumPy builds, so the result cannot be pinned")
    if isinstance(order, bool) or order not in (0, 1):
        raise NotImplementedError(f"{what}: order={order!r} is not built (0 and 1 are)")
    dtype = np.dtype(dtype)
    if dtype not in nat.NP_TO_MMX:
        raise NotImplementedError(f"{what}: {dtype} images are not built "
                                  f"({', '.join(str(d) for d in nat.NP_TO_MMX)} are)")
    if dtype == np.float32 and order == 1:
        raise NotImplementedError(f"{what}: float32 images at order 1 are not built (scikit-image's float32 "
                                  f"interpolation does not reproduce; order 0 is built)")


def _axis_of(axis, ndim: int) -> int:
    a = int(axis)
    if a < 0:
        a += ndim
    if a not in (0, 1, 2):
        raise ValueError(f"axis must be one of the (z, y, x) axes, not {axis!r}")
    return a


def _plane_shape(shape3, axis: int) -> Tuple[int, int]:
    return tuple(int(s) for i, s in enumerate(shape3) if i != axis)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _view_of(t) -> Tuple[nat.DsView, int, Tuple[int, int, int], int]:
    """``(view, elements behind it, (nz, ny, nx), channels)`` of a ``(z, y, x[, c])`` device tensor through its strides;
    the channels of a voxel have to lie beside each other."""
    code = nat.NP_TO_MMX[np.dtype(str(t.dtype).replace("torch.", ""))]
    st = t.stride()
    n_chl = int(t.shape[3]) if t.ndim == 4 else 1
    if t.ndim == 4 and n_chl > 1 and int(st[3]) != 1:
        raise ValueError("the channels of a voxel must lie at consecutive elements")
    elems = 1 + sum((int(n) - 1) * int(s) for n, s in zip(t.shape, st))
    # (an axis of one voxel is never stepped along: whatever stride it reports, a zero included, a valid one is passed)
    sz, sy, sx = (int(s) if int(n) > 1 else max(int(s), n_chl) for n, s in zip(t.shape[:3], st[:3]))
    view = nat.DsView(int(t.data_ptr()), code, 0, sz, sy, sx)
    return view, elems, tuple(int(v) for v in t.shape[:3]), n_chl


def rotate_tensor(src, dst, angle: float, axis: int, order: int) -> None:
    """One rotation of the ``(z, y, x[, c])`` device tensor ``src`` into ``dst`` (same shape and dtype, another
    buffer; any strides whose channels lie beside each other): the two launches, stream-ordered."""
    L = nat.lib()
    sv, s_elems, shape3, n_chl = _view_of(src)
    dv, d_elems, d_shape3, d_chl = _view_of(dst)
    if shape3 != d_shape3 or n_chl != d_chl or src.dtype != dst.dtype:
        raise ValueError("source and destination differ in shape or dtype")
    rows, cols = _plane_shape(shape3, axis)
    m = rotation_matrix(rows, cols, angle)
    if src.dtype == torch.float32:
        m = m.astype(np.float32).astype(np.float64)
    m = np.ascontiguousarray(m.reshape(-1))
    stream = _stream()
    bounds = None
    if order == 1:
        bounds = torch.empty(shape3[axis] * 2, dtype=torch.float64, device=src.device)
        nat.check(L.mmx_rotate_minmax(ctypes.byref(sv), s_elems, *shape3, n_chl, axis, bounds.data_ptr(), stream),
                  "mmx_rotate_minmax")
    nat.check(L.mmx_rotate_warp(ctypes.byref(sv), s_elems, ctypes.byref(dv), d_elems, *shape3, n_chl, axis,
                                nat.as_double_ptr(m), int(order), None if bounds is None else bounds.data_ptr(),
                                stream), "mmx_rotate_warp")


def _into_host(t, out) -> np.ndarray:
    """A device tensor into a host array, z-slab by z-slab (``out``: the array, or a factory ``out(shape, dtype)``)."""
    dtype = np.dtype(str(t.dtype).replace("torch.", ""))
    host = equalize._resolve_out(out, tuple(t.shape), dtype)
    per_plane = max(1, int(np.prod(t.shape[1:], dtype=np.int64)) * dtype.itemsize)
    step = max(1, min(int(t.shape[0]), SLAB_BYTES // per_plane))
    for z0 in range(0, int(t.shape[0]), step):
        host[z0:z0 + step] = t[z0:z0 + step].cpu().numpy()
    return host


def rotate_chain(image, rotation: Sequence[Tuple[float, int]], order: int = 1, resize: bool = False,
                 what: str = "rotate_img", _keep: bool = False, _out=None):
    """``image`` through the rotations ``((angle, axis), ...)`` in order, each on the previous result; the volume stays
    on the device between them (two buffers) and leaves it once.  ``image``: a 3-D or 4-D ``(z, y, x[, c])`` NumPy array
    (a host array comes back), a torch tensor (a tensor on the device comes back) or a ``DeviceVolume`` (a
    ``DeviceVolume`` comes back); never changed.  ``_keep``: the result stays a device tensor whatever came in;
    ``_out``: the host array (or factory) the result is written into."""
    from .volume import DeviceVolume, _require_gpu
    resident = isinstance(image, DeviceVolume)
    is_tensor = torch is not None and isinstance(image, torch.Tensor)
    if resident:
        dtype, shape = image.np_dtype, tuple(image.tensor.shape)
        if image.z_off or image.y_off or tuple(image.tensor.shape[:3]) != tuple(image.shape[:3]):
            raise ValueError("a DeviceVolume that holds a box of its image cannot be rotated")
    elif is_tensor:
        dtype, shape = np.dtype(str(image.dtype).replace("torch.", "")), tuple(image.shape)
    else:
        image = image if isinstance(image, np.ndarray) else np.asarray(image)
        dtype, shape = image.dtype, tuple(image.shape)
    rotation = [(float(r[0]), r[1]) for r in rotation]
    if rotation:
        check_args(dtype, order, resize, what)
    if len(shape) not in (3, 4):
        raise ValueError("image must be (z, y, x) or (z, y, x, c)")
    if min(shape) < 1:
        raise ValueError(f"an image of shape {shape} is empty")
    rotation = [(angle, _axis_of(axis, len(shape))) for angle, axis in rotation]
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    on_device = resident or (is_tensor and image.is_cuda)
    # the source (when it is not there yet) and the destination; a second destination when the source must survive a
    # chain of several rotations
    need = nbytes * ((0 if on_device else 1) + (1 if rotation else 0) + (1 if on_device and len(rotation) > 1 else 0))
    equalize._check_fits(need, what)

    if resident:
        image.wait_all()
        cur = image.tensor
    elif is_tensor:
        cur = image if image.is_cuda else image.to(_require_gpu())
    else:
        cur = torch.from_numpy(np.ascontiguousarray(image)).to(_require_gpu())
    owned = not on_device           # (`cur` is this call's own upload: a chain may write over it)
    spare = None
    for angle, axis in rotation:
        if spare is None:
            spare = torch.empty(shape, dtype=cur.dtype, device=cur.device)
        rotate_tensor(cur, spare, angle, axis, order)
        if owned:
            cur, spare = spare, cur
        else:
            cur, spare, owned = spare, None, True
    if not rotation and (on_device or _keep):
        cur = cur.clone() if on_device else cur
    if _out is not None:
        res = _into_host(cur, _out)
    elif _keep or is_tensor:
        res = cur if (_keep or image.is_cuda) else cur.cpu()
    elif resident:
        res = DeviceVolume(cur)
    else:
        res = _into_host(cur, None)
    torch.cuda.current_stream().synchronize()
    return res


def rotate_nd(img_np, angle: float, axis: int = 0, order: int = 1, resize: bool = False):
    """``cv_nd.rotate_nd``: every 2-D plane of ``img_np`` along ``axis`` rotated by ``angle`` degrees about its centre,
    in the image's dtype and shape.  ``img_np``: a 2-D, 3-D or 4-D ``(z, y, x, c)`` NumPy array (a host array comes
    back), torch tensor or ``DeviceVolume``.  A 2-D image is wrapped into one plane, as the reference does, so its
    ``axis`` should stay 0.  See the module's docstring for what is refused."""
    ndim = len(img_np.shape)
    if ndim == 2:
        if isinstance(img_np, np.ndarray) or (torch is not None and isinstance(img_np, torch.Tensor)):
            return rotate_chain(img_np[None], [(angle, axis)], order, resize, "rotate_nd")[0]
    return rotate_chain(img_np, [(angle, axis)], order, resize, "rotate_nd")
