"""The device-image layer under the whole-image tasks: everything between "an image came in" and "a result went out".

The tasks of :mod:`equalize`, :mod:`rotate` and :mod:`transformer` take a host array, a torch tensor or a
``DeviceVolume``, address it through its strides, and hand back a tensor that stays on the device for the next task of a
chain or a host array filled z-slab by z-slab.  That plumbing is stated here once, and nothing here knows a task:
:func:`open_image` (what came in: the shared refusals, then the upload), :func:`view` (the one place where strides become
an ``mmx_ds_view``), :class:`Result` with :func:`slab_step` and :data:`SLAB_BYTES` (where the result goes, what the
caller gets back), and the small helpers.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _native as nat
from .volume import DeviceVolume, _require_gpu

#: bytes of one z-slab of a result on its way to the host
SLAB_BYTES = 256 << 20


def np_dtype_of(tensor) -> np.dtype:
    """The NumPy dtype of a torch tensor's elements."""
    return np.dtype(str(tensor.dtype).replace("torch.", ""))


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def to_dev(arr: np.ndarray, dev):
    """A host table as bytes on the device."""
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).to(dev)


def free_bytes() -> int:
    return int(torch.cuda.mem_get_info()[0])


def check_fits(need: int, what: str) -> None:
    free = free_bytes()
    if need > 0.9 * free:
        raise NotImplementedError(f"{what} needs {need} bytes on the device beside its working buffers, {free} are "
                                  f"free: an image that does not fit the device is not built")


def view(image, channel=None, z0: int = 0):
    """The ``mmx_ds_view`` of a ``(z, y, x[, c])`` device tensor (or of the tensor of a ``DeviceVolume`` or an
    :class:`Image` that holds its whole image) through its strides, from plane ``z0`` on.  ``channel=None``: all
    channels of every voxel -- ``(view, elements behind it, channels)``, what the rotation entries take; a channel
    number: the view of that channel alone.  The channels of a voxel have to lie beside each other."""
    t = getattr(image, "tensor", image)
    st = t.stride()
    n_chl = int(t.shape[3]) if t.ndim == 4 else 1
    if n_chl > 1 and int(st[3]) != 1:
        raise ValueError("the channels of a voxel must lie at consecutive elements")
    if not 0 <= int(z0) < max(1, int(t.shape[0])) or (channel is not None and not 0 <= int(channel) < n_chl):
        raise ValueError(f"plane {z0}, channel {channel} of an image of shape {tuple(t.shape)}")
    # (an axis of one voxel is never stepped along: whatever stride it reports, a zero included, a valid one is passed)
    sz, sy, sx = (int(s) if int(n) > 1 else max(int(s), n_chl) for n, s in zip(t.shape[:3], st[:3]))
    skip = int(z0) * sz + (int(channel) if channel is not None else 0)
    v = nat.DsView(int(t.data_ptr()) + skip * t.element_size(), nat.NP_TO_MMX[np_dtype_of(t)], 0, sz, sy, sx)
    if channel is not None:
        return v
    return v, 1 + sum((int(n) - 1) * int(s) for n, s in zip(t.shape, st)) - skip, n_chl


# ------------------------------------------------------------------------------------------------ what came in
def describe(image) -> Tuple[np.dtype, Tuple[int, ...], bool]:
    """``(voxel dtype, shape, on the device already?)`` of anything :func:`open_image` takes; refuses nothing and
    touches no device."""
    if isinstance(image, DeviceVolume):
        return image.np_dtype, tuple(image.tensor.shape), True
    if isinstance(image, torch.Tensor):
        return np_dtype_of(image), tuple(image.shape), image.is_cuda
    arr = image if isinstance(image, np.ndarray) else np.asarray(image)
    return arr.dtype, tuple(arr.shape), False


class Image:
    """An opened image: ``tensor`` (the ``(z, y, x[, c])`` voxels on the device), ``np_dtype``, ``shape``, ``n_chl``,
    ``multichannel``, ``owned`` (the tensor is this call's own upload: a task may write over it) and ``source`` (the
    caller's object).  As a context manager it closes an upload it made itself and nothing else."""

    def __init__(self, source, tensor, np_dtype, owned: bool, volume=None):
        self.source, self.tensor, self.np_dtype = source, tensor, np.dtype(np_dtype)
        self.owned, self._volume = owned, volume
        self.shape = tuple(int(v) for v in tensor.shape)
        self.multichannel = tensor.ndim == 4
        self.n_chl = self.shape[3] if self.multichannel else 1

    @property
    def volume(self) -> DeviceVolume:
        """The ``DeviceVolume`` of the tensor (the caller's own where it gave one), for the entries that take one."""
        if self._volume is None:
            self._volume = DeviceVolume(self.tensor)
        return self._volume

    def host(self) -> np.ndarray:
        """The image as the host sees it: the caller's own array (not a copy), otherwise a download."""
        return self.source if isinstance(self.source, np.ndarray) else self.tensor.cpu().numpy()

    def close(self) -> None:
        if self.owned and self._volume is not None:
            self._volume.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def open_image(image, what: str, extra_per_voxel: int = 0, extra_bytes: int = 0, before_fit=None) -> Image:
    """``image`` -- a NumPy array, a torch tensor on the host or the device, or a ``DeviceVolume`` -- as an
    :class:`Image` on the device, after the refusals every whole-image task shares, in this order: a ``DeviceVolume``
    that holds a box of its image, a voxel type that is not built, a shape that is not ``(z, y, x[, c])``, an empty
    image (``ValueError`` / ``NotImplementedError``, from the arguments alone); then ``before_fit()``, the caller's last
    checks of its own arguments; then the room: the image itself unless it is there already, ``extra_per_voxel`` bytes
    per (z, y, x) voxel and ``extra_bytes`` (:func:`check_fits`).  A resident volume is waited for, never copied."""
    dtype, shape, on_device = describe(image)
    if isinstance(image, DeviceVolume) and (image.z_off or image.y_off or shape[:3] != tuple(image.shape[:3])):
        raise ValueError(f"{what}: a DeviceVolume that holds a box of its image is not taken")
    if dtype not in nat.NP_TO_MMX:
        raise NotImplementedError(f"{what}: {dtype} images are not built "
                                  f"({', '.join(str(d) for d in nat.NP_TO_MMX)} are)")
    if len(shape) not in (3, 4):
        raise ValueError(f"{what}: image must be (z, y, x) or (z, y, x, c)")
    if min(shape) < 1:
        raise ValueError(f"{what}: an image of shape {shape} is empty")
    if before_fit is not None:
        before_fit()
    nbytes = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
    check_fits((0 if on_device else nbytes) + int(np.prod(shape[:3], dtype=np.int64)) * extra_per_voxel + extra_bytes,
               what)
    if isinstance(image, DeviceVolume):
        image.wait_all()
        return Image(image, image.tensor, dtype, False, image)
    if isinstance(image, torch.Tensor):
        return Image(image, image if on_device else image.to(_require_gpu()), dtype, not on_device)
    vol = DeviceVolume(image if isinstance(image, np.ndarray) else np.asarray(image), streamed=False)
    return Image(image, vol.tensor, dtype, True, vol)


# --------------------------------------------------------------------------------------------- what goes out
def slab_step(shape, itemsize: int) -> Tuple[int, int]:
    """``(planes per z-slab, slabs)`` of a ``(z, y, x[, c])`` result of ``itemsize`` bytes per element that leaves in
    slabs of at most :data:`SLAB_BYTES`; one plane at least."""
    nz = int(shape[0])
    plane = max(1, int(np.prod(shape[1:], dtype=np.int64)) * int(itemsize))
    step = max(1, min(nz, SLAB_BYTES // plane))
    return step, (nz + step - 1) // step


class Result:
    """Where a task's ``shape`` / ``dtype`` result goes and what the caller gets back.  ``keep``: a tensor on ``device``
    for the next task of a chain.  Otherwise a host array: ``out`` itself, what the factory ``out(shape, dtype)`` makes
    (called here, once the result's dtype is known) or a new array; the assignments into it cast as NumPy's do.
    ``zero_fill``: the parts nothing is put into read zero."""

    def __init__(self, shape, dtype, keep: bool = False, out=None, zero_fill: bool = False, device=None):
        self.shape, self.dtype, self.zero_fill, self.device = tuple(shape), np.dtype(dtype), zero_fill, device
        self.tensor = self.host = None
        if keep:
            return
        if out is None:
            self.host = np.empty(self.shape, dtype=self.dtype)
        elif callable(out):
            self.host = out(self.shape, self.dtype)
        elif tuple(out.shape) != self.shape or out.dtype != self.dtype:
            raise ValueError(f"out must be {self.shape} {self.dtype}, not {tuple(out.shape)} {out.dtype}")
        else:
            self.host = out
        if zero_fill:
            self.host[...] = 0

    def put(self, z0: int, z1: int, channel, slab) -> None:
        """Planes ``[z0, z1)`` of the result (of one channel of it) from ``slab``, a tensor of that shape."""
        if self.host is None and self.tensor is None:
            make = torch.zeros if self.zero_fill else torch.empty
            self.tensor = make(self.shape, dtype=getattr(torch, self.dtype.name), device=self.device)
        dst = self.tensor if self.host is None else self.host
        dst = dst[z0:z1] if channel is None else dst[z0:z1, ..., channel]
        if self.host is None:
            dst.copy_(slab)
        else:
            dst[...] = slab.cpu().numpy()

    def drain(self, tensor, channel=None) -> None:
        """A whole tensor into the result (into one channel of it): z-slab by z-slab; a kept result that nothing was
        put into yet IS the tensor, without a copy."""
        if self.host is None and self.tensor is None and channel is None:
            self.tensor = tensor
            return
        nz = int(tensor.shape[0])
        step, _ = slab_step(tensor.shape, tensor.element_size())
        for z0 in range(0, nz, step):
            self.put(z0, min(nz, z0 + step), channel, tensor[z0:z0 + step])

    def value(self):
        return self.tensor if self.host is None else self.host
