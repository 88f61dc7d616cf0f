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

import torch

from . import _native as nat
from . import device_image as dimg
from .volume import DeviceVolume


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


def plane_shape(shape3, axis: int) -> Tuple[int, int]:
    return tuple(int(s) for i, s in enumerate(shape3) if i != axis)


def rotate_tensor(src, dst, angle: float, axis: int, order: int) -> None:
    """One rotation of the ``(z, y, x[, c])`` device tensor ``src`` into ``dst`` (same shape and dtype, another
    buffer; any strides whose channels lie beside each other): the two launches, stream-ordered."""
    L = nat.lib()
    if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
        raise ValueError("source and destination differ in shape or dtype")
    sv, s_elems, n_chl = dimg.view(src)
    dv, d_elems, _ = dimg.view(dst)
    shape3 = tuple(int(v) for v in src.shape[:3])
    rows, cols = plane_shape(shape3, axis)
    m = rotation_matrix(rows, cols, angle)
    if src.dtype == torch.float32:
        m = m.astype(np.float32).astype(np.float64)
    m = np.ascontiguousarray(m.reshape(-1))
    stream = dimg.stream()
    bounds = None
    if order == 1:
        bounds = torch.empty(shape3[axis] * 2, dtype=torch.float64, device=src.device)
        nat.check(L.mmx_rotate_minmax(ctypes.byref(sv), s_elems, *shape3, n_chl, axis, bounds.data_ptr(), stream),
                  "mmx_rotate_minmax")
    nat.check(L.mmx_rotate_warp(ctypes.byref(sv), s_elems, ctypes.byref(dv), d_elems, *shape3, n_chl, axis,
                                nat.as_double_ptr(m), int(order), None if bounds is None else bounds.data_ptr(),
                                stream), "mmx_rotate_warp")


def rotate_chain(image, rotation: Sequence[Tuple[float, int]], order: int = 1, resize: bool = False,
                 what: str = "rotate_img", _keep: bool = False, _out=None):
    """``image`` through the rotations ``((angle, axis), ...)`` in order, each on the previous result; the volume stays
    on the device between them (two buffers) and leaves it once.  ``image``: a 3-D or 4-D ``(z, y, x[, c])`` NumPy array
    (a host array comes back), a torch tensor (a tensor on the device comes back) or a ``DeviceVolume`` (a
    ``DeviceVolume`` comes back); never changed.  ``_keep``: the result stays a device tensor whatever came in;
    ``_out``: the host array (or factory) the result is written into."""
    dtype, shape, on_device = dimg.describe(image)
    rotation = [(float(r[0]), r[1]) for r in rotation]
    if rotation:
        check_args(dtype, order, resize, what)

    def check_axes():
        rotation[:] = [(angle, _axis_of(axis, len(shape))) for angle, axis in rotation]
    # beside the source: the destination; a second one when the source must survive a chain of several rotations
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    need = nbytes * ((1 if rotation else 0) + (1 if on_device and len(rotation) > 1 else 0))
    with dimg.open_image(image, what, extra_bytes=need, before_fit=check_axes) as img:
        cur, owned = img.tensor, img.owned      # (owned: this call's own upload, which a chain may write over)
        spare = None
        for angle, axis in rotation:
            if spare is None:
                spare = torch.empty(shape, dtype=cur.dtype, device=cur.device)
            rotate_tensor(cur, spare, angle, axis, order)
            if owned:
                cur, spare = spare, cur
            else:
                cur, spare, owned = spare, None, True
        if not rotation and on_device:
            cur = cur.clone()
        # what comes back: the array or factory given, the kind that came in, or a device tensor for the next task
        resident, is_tensor = isinstance(image, DeviceVolume), isinstance(image, torch.Tensor)
        as_tensor = _out is None and (_keep or resident or is_tensor)
        res = dimg.Result(shape, dtype, as_tensor, _out)
        res.drain(cur)
        torch.cuda.current_stream().synchronize()
    if _keep or not as_tensor:
        return res.value()
    return DeviceVolume(cur) if resident else (cur if on_device else cur.cpu())


def rotate_nd(img_np, angle: float, axis: int = 0, order: int = 1, resize: bool = False):
    """``cv_nd.rotate_nd``: every 2-D plane of ``img_np`` along ``axis`` rotated by ``angle`` degrees about its centre,
    in the image's dtype and shape.  ``img_np``: a 2-D, 3-D or 4-D ``(z, y, x, c)`` NumPy array (a host array comes
    back), torch tensor or ``DeviceVolume``.  A 2-D image is wrapped into one plane, as the reference does, so its
    ``axis`` should stay 0.  See the module's docstring for what is refused."""
    ndim = len(img_np.shape)
    if ndim == 2 and isinstance(img_np, (np.ndarray, torch.Tensor)):
        return rotate_chain(img_np[None], [(angle, axis)], order, resize, "rotate_nd")[0]
    return rotate_chain(img_np, [(angle, axis)], order, resize, "rotate_nd")
