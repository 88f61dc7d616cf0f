"""Whole-image preprocessing on the device: ``saturate``, ``denoise`` and ``remap`` of ``mm <img> --proc preprocess=...``.

Mirror of ``plot_3d.saturate_roi`` (reference magmap/plot/plot_3d.py:55-111) and ``plot_3d.remap_intensity`` (:270-317)
-> ``skimage.exposure.equalize_adapthist`` as ``transformer.preprocess_img`` runs them over a whole stack
(magmap/atlas/transformer.py:353-393), bit for bit, quirks included.  The passes over the voxels are HIP kernels
(``csrc/mmx_clahe.hip``); everything that acts on a few thousand values is stated here in NumPy's own expressions and
uploaded as a table, so that no device arithmetic has to be pinned for it:

* the chain voxel -> ``img_as_uint`` -> 14-bit level -> histogram bin is a function of the raw value for the 8- and
  16-bit types and of ``img_as_uint(voxel)`` for float voxels: :func:`level_bin_table`, 65536 entries, built once the
  image's minimum and maximum are known (``mmx_minmax_batch``).  The kernels' share is the table index
  (:func:`key_of_values`): the value, ``value + 32768`` for int16, ``rint(v * 65535)`` clipped for floats;
* ``clip_histogram`` / ``map_histogram`` are tiles x nbins integers of work between two launches: a native host
  function (``mmx_host_eq_maps``), exact by construction (the reference's integer loop, statement by statement);
* the per-axis interpolation tables (:func:`axis_tables`): which two tiles' maps stand below and above a coordinate,
  and the coefficients ``arange(k) / k`` and ``1 - arange(k) / k``;
* ``img_as_float`` and the last ``rescale_intensity`` act on at most 16384 levels: :func:`output_table`, from the
  measured minimum and maximum of the uint16 result, the constant-image branch included.

How an image comes in (a NumPy array, a torch tensor or a ``DeviceVolume``) and how a result goes out is
:mod:`device_image`'s: the float64 result leaves the device in z-slabs of at most ``device_image.SLAB_BYTES``, straight
into the array given as ``out`` (``transformer.preprocess_img`` hands the output file's memory map); between the tasks
of a chain a float64 single-result image stays on the device.

``denoise`` is ``plot_3d.denoise_roi`` (:114-172), :func:`denoise_roi`: the clip, the sigma-8 unsharp mask and the
grey erosion are the passes of ``csrc/mmx_denoise_img.hip`` between two float64 working buffers; the host's share is the
erosion gate ``np.mean(channel) > erosion_threshold``, decided from a device sum (:func:`erosion_gate`).  Its limits:
:func:`denoise_check_args`.

Stated limits (``NotImplementedError``, from the arguments, ahead of any launch): ``nbins > 16384``; a tile of 2^31
voxels or more; ``saturate`` of a float32 image unless ``preprocess.FLOAT32_RULES = "numpy2"``; an image that does not
fit the device beside its working buffers.  A NaN voxel is outside the contract (the reference's result for one is
whatever the platform's float -> uint16 cast gives).  The fixture pins scikit-image 0.18.3.
"""
from __future__ import annotations

import ctypes
import numbers
from typing import Sequence, Tuple

import numpy as np
import torch

from . import _native as nat
from . import config
from . import device_image as dimg

NR_OF_GRAY = 2 ** 14
#: most bins of an equalisation (a bin per 14-bit level)
MAX_NBINS = NR_OF_GRAY


# ------------------------------------------------------------------------------------------------- host tables
def key_of_values(values: np.ndarray) -> np.ndarray:
    """The table index the kernels form for voxels of ``values``' type (``eq_key`` of csrc/mmx_clahe.hip)."""
    values = np.asarray(values)
    dt = values.dtype
    if dt in (np.uint8, np.uint16):
        return values.astype(np.int64)
    if dt == np.int16:
        return values.astype(np.int64) + 32768
    if dt.kind == "f":
        out = np.multiply(values, 65535, dtype=dt)
        np.rint(out, out=out)
        np.clip(out, 0, 65535, out=out)
        return out.astype(np.int64)
    raise NotImplementedError(f"equalisation of {dt} images is not built")


def uint_of_keys(dtype) -> np.ndarray:
    """``img_as_uint`` of the voxel behind every table index, as scikit-image's ``_convert`` computes it: 65536
    entries (uint8: the first 256 are read)."""
    dtype = np.dtype(dtype)
    out = np.zeros(65536, dtype=np.uint16)
    if dtype == np.uint8:
        # _scale(a, 8, 16): an exact upscale by (2**16 - 1) // (2**8 - 1)
        out[:256] = np.multiply(np.arange(256, dtype=np.uint8), 257, dtype=np.uint16)
    elif dtype == np.int16:
        # _scale(a, 15, 16): up to 30 bits in int32, down by 14 bits, then np.maximum(., 0) into uint16
        b = np.multiply(np.arange(-32768, 32768, dtype=np.int32).astype(np.int16), (2 ** 30 - 1) // (2 ** 15 - 1),
                        dtype=np.int32)
        b //= 2 ** 14
        out[:] = np.maximum(b, 0).astype(np.uint16)
    elif dtype == np.uint16 or dtype.kind == "f":
        out[:] = np.arange(65536, dtype=np.uint16)     # (a float voxel's index IS its img_as_uint)
    else:
        raise NotImplementedError(f"equalisation of {dtype} images is not built")
    return out


def level_bin_table(dtype, raw_min, raw_max, nbins: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(levels, bins)``, 65536 uint16 entries each, by table index: the 14-bit level
    ``np.round(rescale_intensity(img_as_uint(image), out_range=(0, 16383))).astype(np.uint16)`` of a voxel of an image
    whose raw extremes are ``raw_min`` / ``raw_max`` (``img_as_uint`` is monotonic: the converted extremes are the
    conversions of these two), and its histogram bin ``level // (1 + 16384 // nbins)``."""
    dtype = np.dtype(dtype)
    u = uint_of_keys(dtype)
    kmin, kmax = (int(key_of_values(np.array([v], dtype=dtype))[0]) for v in (raw_min, raw_max))
    imin, imax = float(u[kmin]), float(u[kmax])
    img = np.clip(u.astype(np.float64), imin, imax)
    if imin != imax:
        img = (img - imin) / (imax - imin)
        img = img * (float(NR_OF_GRAY - 1) - 0.0) + 0.0
    else:
        img = np.clip(img, 0.0, float(NR_OF_GRAY - 1))
    levels = np.round(img).astype(np.uint16)
    lut = np.arange(NR_OF_GRAY)
    lut //= 1 + NR_OF_GRAY // int(nbins)
    return levels, lut[levels].astype(np.uint16)


def output_table(lmin: int, lmax: int) -> np.ndarray:
    """``rescale_intensity(img_as_float(image))`` for every uint16 level below 16384 of an image whose ``_clahe`` result
    has the minimum ``lmin`` and the maximum ``lmax``; a constant image comes back constant (clipped to [0, 1])."""
    lv = np.arange(NR_OF_GRAY, dtype=np.uint16)
    img = np.multiply(lv, 1.0 / 65535, dtype=np.float64)
    imin, imax = float(img[int(lmin)]), float(img[int(lmax)])
    img = np.clip(img, imin, imax)
    if imin != imax:
        img = (img - imin) / (imax - imin)
        return img * (1.0 - 0.0) + 0.0
    return np.clip(img, 0.0, 1.0)


def resolve_kernel(shape3: Sequence[int], kernel_size) -> Tuple[int, int, int]:
    """``equalize_adapthist``'s kernel size: ``shape // 8`` by default, a number for every axis, or one per axis."""
    if kernel_size is None:
        kernel_size = tuple(int(s) // 8 for s in shape3)
    elif isinstance(kernel_size, numbers.Number):
        kernel_size = (kernel_size,) * len(shape3)
    elif len(kernel_size) != len(shape3):
        raise ValueError("Incorrect value of `kernel_size`: {}".format(kernel_size))
    return tuple(int(k) for k in kernel_size)


def plan(shape3: Sequence[int], kernel_size, clip_limit, nbins):
    """``(kernel, tiles per axis, clip count)`` of one equalisation, and every refusal that follows from the
    arguments alone.  An axis shorter than 8 with the default kernel gives a kernel of 0 and the reference's
    ``ZeroDivisionError`` (raised by the same expression)."""
    shape3 = tuple(int(s) for s in shape3)
    if len(shape3) != 3:
        raise ValueError("equalize_adapthist takes one (z, y, x) channel")
    nbins = int(nbins)
    if nbins > MAX_NBINS:
        raise NotImplementedError(f"nbins = {nbins}: more bins than the {MAX_NBINS} grey levels are not built")
    if nbins < 1:
        raise ValueError("nbins must be positive")
    k = resolve_kernel(shape3, kernel_size)
    # (_clahe's padding: the expression that fails for a kernel of 0)
    pad_end = [(kk - s % kk) % kk + int(np.ceil(kk / 2.)) for kk, s in zip(k, shape3)]
    if min(k) < 1:
        raise ValueError(f"kernel_size must be positive, not {k}")
    n_pixels = int(np.prod(k, dtype=object))
    if n_pixels >= 2 ** 31:
        raise NotImplementedError(f"a tile of {n_pixels} voxels (kernel_size {k}): 2^31 and more are not built")
    del pad_end
    nt = tuple(-(-s // kk) for s, kk in zip(shape3, k))
    if clip_limit > 0.0:
        clim = int(np.clip(clip_limit * np.prod(k, dtype=np.int64), 1, None))
    else:
        clim = n_pixels
    return k, nt, clim


def axis_tables(shape3, k, nt) -> Tuple[np.ndarray, np.ndarray]:
    """``(tiles, coef)``, ``[nz + ny + nx][2]`` each: coordinate ``c`` of an axis lies at offset ``o = (c + k // 2) % k``
    of interpolation block ``b = (c + k // 2) // k`` of the padded image; the maps below and above it are those of the
    histogram tiles ``b - 1`` and ``b``, clamped into ``[0, nt)`` (the edge padding of the map array), with the
    coefficients ``1 - arange(k)[o] / k`` and ``arange(k)[o] / k``."""
    tiles, coef = [], []
    for s, kk, n in zip(shape3, k, nt):
        c = np.arange(int(s), dtype=np.int64) + kk // 2
        b, o = c // kk, c % kk
        frac = (np.arange(kk) / kk)[o]
        tiles.append(np.stack([np.clip(b - 1, 0, n - 1), np.clip(b, 0, n - 1)], axis=1))
        coef.append(np.stack([1 - frac, frac], axis=1))
    return (np.ascontiguousarray(np.concatenate(tiles), dtype=np.int32),
            np.ascontiguousarray(np.concatenate(coef), dtype=np.float64))


# --------------------------------------------------------------------------------------------------- the device
def minmax(volume, channel: int) -> Tuple[float, float]:
    """The raw minimum and maximum of one channel of a ``DeviceVolume`` that holds its whole image."""
    L = nat.lib()
    dev = volume.tensor.device
    nz, ny, nx = (int(v) for v in volume.shape[:3])
    blocks = np.zeros(1, dtype=nat.BLOCK_DTYPE)
    blocks[0] = (0, nz, ny, nx, 0, 0, 0)
    d_blocks = dimg.to_dev(blocks, dev)
    d_mm = torch.tensor([np.inf, -np.inf], dtype=torch.float64, device=dev)
    vol = volume.view(channel, False)
    nat.check(L.mmx_minmax_batch(ctypes.byref(vol), d_blocks.data_ptr(), blocks.ctypes.data, 1, d_mm.data_ptr(),
                                 dimg.stream()), "mmx_minmax_batch")
    lo, hi = d_mm.cpu().numpy()
    return float(lo), float(hi)


def _equalize_channel(img, channel: int, kernel_size, clip_limit, nbins, sink, sink_channel, parts=None) -> None:
    """One channel of the opened image through the passes; the float64 result goes to ``sink`` (a
    ``device_image.Result``)."""
    L = nat.lib()
    dev = img.tensor.device
    shape3 = img.shape[:3]
    k, nt, clim = plan(shape3, kernel_size, clip_limit, nbins)
    nbins = int(nbins)
    n_tiles = int(np.prod(nt))
    n_vox = int(np.prod(shape3, dtype=np.int64))
    stream = dimg.stream()

    raw_min, raw_max = minmax(img.volume, channel)
    if img.np_dtype.kind == "f" and (raw_min < -1.0 or raw_max > 1.0):
        raise ValueError("Images of type float must be between -1 and 1.")
    levels, bins = level_bin_table(img.np_dtype, raw_min, raw_max, nbins)
    d_bins = dimg.to_dev(bins, dev)
    src = dimg.view(img, channel)
    geom = nat.EqGeom((ctypes.c_int32 * 3)(*shape3), (ctypes.c_int32 * 3)(*k), (ctypes.c_int32 * 3)(*nt), nbins)

    d_hist = torch.empty(n_tiles * nbins, dtype=torch.int32, device=dev)
    nat.check(L.mmx_eq_hist(ctypes.byref(src), ctypes.byref(geom), d_bins.data_ptr(), d_hist.data_ptr(), stream),
              "mmx_eq_hist")
    hist = d_hist.cpu().numpy().view(np.uint32)
    maps = np.empty(n_tiles * nbins, dtype=np.uint16)
    entered = np.zeros(n_tiles, dtype=np.uint8)
    nat.check(L.mmx_host_eq_maps(hist.ctypes.data, n_tiles, nbins, clim, int(np.prod(k)), maps.ctypes.data,
                                 entered.ctypes.data), "mmx_host_eq_maps")
    d_maps = dimg.to_dev(maps, dev)
    tiles, coef = axis_tables(shape3, k, nt)
    d_tiles, d_coef = dimg.to_dev(tiles, dev), dimg.to_dev(coef, dev)
    d_out = torch.empty(n_vox, dtype=torch.int16, device=dev)
    d_mm = torch.empty(2, dtype=torch.int32, device=dev)
    nat.check(L.mmx_eq_apply(ctypes.byref(src), ctypes.byref(geom), d_bins.data_ptr(), d_maps.data_ptr(),
                             d_tiles.data_ptr(), tiles.ctypes.data, d_coef.data_ptr(), d_out.data_ptr(),
                             d_mm.data_ptr(), stream), "mmx_eq_apply")
    lmin, lmax = (int(v) for v in d_mm.cpu().numpy().view(np.uint32))
    if parts is not None:
        parts.update(kernel=k, tiles=nt, clim=clim, levels_table=levels, bins_table=bins,
                     hist=hist.reshape(n_tiles, nbins).copy(), maps=maps.reshape(n_tiles, nbins).copy(),
                     entered=entered.astype(bool), clahe=d_out.cpu().numpy().view(np.uint16).reshape(shape3),
                     minmax=(lmin, lmax))
    d_table = dimg.to_dev(output_table(lmin, lmax), dev)
    nz, ny, nx = shape3
    step, _ = dimg.slab_step(shape3, 8)
    slab = torch.empty(step * ny * nx, dtype=torch.float64, device=dev)
    for z0 in range(0, nz, step):
        z1 = min(nz, z0 + step)
        n = (z1 - z0) * ny * nx
        nat.check(L.mmx_eq_output(d_out.data_ptr() + 2 * z0 * ny * nx, n, d_table.data_ptr(), slab.data_ptr(), stream),
                  "mmx_eq_output")
        sink.put(z0, z1, sink_channel, slab[:n].view(z1 - z0, ny, nx))
    torch.cuda.current_stream().synchronize()


def equalize_adapthist(image, kernel_size=None, clip_limit=0.01, nbins=256, out=None, parts=None):
    """``skimage.exposure.equalize_adapthist`` of one ``(z, y, x)`` channel -- a NumPy array or a single-channel
    ``DeviceVolume`` of any of the five voxel types: the float64 result, written into ``out`` when given (an array or
    a memory map of the image's shape).  ``parts`` (a dict, for tests and tools) receives the intermediates: the tile
    histograms, the clipped maps, the uint16 image ``_clahe`` returns."""
    shape = tuple(image.shape)
    if len(shape) != 3:
        raise ValueError("equalize_adapthist takes one (z, y, x) channel")
    plan(shape, kernel_size, clip_limit, nbins)                   # (every refusal, ahead of the device)
    res = dimg.Result(shape, np.float64, out=out)                 # (a mismatching `out` is refused here)
    with dimg.open_image(image, "equalize_adapthist", 2 + 2) as img:
        _equalize_channel(img, 0, kernel_size, clip_limit, nbins, res, None, parts)
    return res.value()


def _is_seq(val) -> bool:
    return isinstance(val, (list, tuple)) or np.ndim(val) != 0


def _get_if_within(val, i, default=None):
    """``libmag.get_if_within``: element ``i`` of a sequence (``default`` beyond its end), a scalar as it is."""
    if not _is_seq(val):
        return val
    if len(val) > i:
        return val[i]
    return default


def _setup_channels(shape, channel):
    """``plot_3d.setup_channels`` with the channel axis at 3."""
    multichannel = len(shape) > 3
    if multichannel:
        return True, (range(shape[3]) if channel is None else channel)
    return False, [0]


def remap_intensity(roi, channel=None, _keep=False, _out=None, **kwargs):
    """``plot_3d.remap_intensity``: adaptive histogram equalisation of the channels in ``channel`` (``None``: all).
    ``clip_limit`` defaults to the FIRST processed channel's ``adapt_hist_lim`` and then holds for the later ones;
    every keyword may be a sequence indexed by the channel NUMBER.  A single-channel image returns the float64
    result; a multichannel one returns a copy in the IMAGE's dtype with the float64 results stored into it (an
    integer image keeps 0 and 1) and the other channels untouched."""
    shape = tuple(roi.shape)
    multichannel, channels = _setup_channels(shape, channel)
    todo = []
    for chl in channels:
        if "clip_limit" not in kwargs:
            kwargs["clip_limit"] = config.get_roi_profile(chl)["adapt_hist_lim"]
        args = {key: _get_if_within(v, chl) for key, v in kwargs.items()}
        unknown = set(args) - {"kernel_size", "clip_limit", "nbins"}
        if unknown:
            raise TypeError(f"equalize_adapthist() got an unexpected keyword argument '{sorted(unknown)[0]}'")
        args = dict(kernel_size=args.get("kernel_size"), clip_limit=args.get("clip_limit", 0.01),
                    nbins=args.get("nbins", 256))
        plan(shape[:3], **args)
        todo.append((chl, args))
    with dimg.open_image(roi, "remap_intensity", 2 + 2 + (8 if _keep and not multichannel else 0)) as img:
        if not multichannel:
            res = dimg.Result(shape, np.float64, _keep, _out, device=img.tensor.device)
            _equalize_channel(img, 0, sink=res, sink_channel=None, **todo[0][1])
            return res.value()
        # (a host copy of the image, whatever `_keep` says: the float64 results are stored into its own dtype)
        res = dimg.Result(shape, img.np_dtype, out=_out)
        res.host[...] = img.host()
        for chl, args in todo:
            _equalize_channel(img, chl, sink=res, sink_channel=chl, **args)
        return res.value()


def _saturate_dtype_ok(dtype) -> bool:
    from . import importer
    return importer._bounds_dtype_ok(dtype)


def saturate_roi(roi, clip_vmin=-1, clip_vmax=-1, max_thresh_factor=-1, channel=None, _keep=False, _out=None):
    """``plot_3d.saturate_roi`` of a whole ``(z, y, x[, c])`` image: per channel ``vmin, vmax = np.percentile(chl,
    (clip_vmin, clip_vmax))`` (the profile's values for -1; the order statistics by radix select on the device), the
    channel unchanged where they are equal, otherwise ``vmax = max(vmax, near_max[chl] * max_thresh_factor)`` and
    ``(np.clip(chl, vmin, vmax) - vmin) / (vmax - vmin)`` in float64.  A multichannel result has the dtype of the
    first processed channel's result, and channels not named stay zero."""
    from . import importer
    dtype, shape, _ = dimg.describe(roi)
    if dtype == np.float32 and not _saturate_dtype_ok(dtype):
        raise NotImplementedError('saturate of a float32 image depends on the NumPy release: set '
                                  'preprocess.FLOAT32_RULES = "numpy2" for the rules the reference pins')
    if not _saturate_dtype_ok(dtype):
        raise NotImplementedError(f"saturate of {dtype} images ({importer._BOUNDS_NAMES})")
    multichannel, channels = _setup_channels(shape, channel)
    with dimg.open_image(roi, "saturate_roi", 8 * (shape[3] if multichannel else 1) if _keep else 0) as img:
        L = nat.lib()
        dev = img.tensor.device
        nz, ny, nx = shape[:3]
        res = None
        for chl in channels:
            settings = config.get_roi_profile(chl)
            vmin_pct = settings["clip_vmin"] if clip_vmin == -1 else clip_vmin
            vmax_pct = settings["clip_vmax"] if clip_vmax == -1 else clip_vmax
            factor = settings["max_thresh_factor"] if max_thresh_factor == -1 else max_thresh_factor
            lo, hi = importer._percentiles_of_groups(img.volume, chl, [(0, nz)], vmin_pct, vmax_pct)
            vmin, vmax = lo[0], hi[0]
            stretched = vmin != vmax
            if stretched:
                max_thresh = config.near_max[chl] * factor
                if vmax < max_thresh:
                    vmax = max_thresh
            if res is None:
                # (the first processed channel decides the result's dtype)
                if not multichannel and not stretched:
                    # (unchanged: the image itself for the next task, otherwise a copy of it in its own dtype)
                    if _keep and _out is None:
                        return img.tensor
                    res = dimg.Result(shape, dtype, out=_out)
                    res.host[...] = img.host()
                    return res.value()
                res_dtype = np.dtype(np.float64) if stretched else dtype
                res = dimg.Result(shape, res_dtype, _keep and res_dtype == np.float64, _out, zero_fill=multichannel,
                                  device=dev)
            c_sink = chl if multichannel else None
            if not stretched:
                # (an unchanged channel behind a stretched one: stored with NumPy's cast into the result's dtype)
                src = img.tensor[..., chl] if multichannel else img.tensor
                if res.host is None:
                    src = torch.from_numpy(np.ascontiguousarray(src.cpu().numpy(), dtype=np.float64)).to(dev)
                res.put(0, nz, c_sink, src)
                continue
            step, _ = dimg.slab_step((nz, ny, nx), 8)
            slab = torch.empty(step * ny * nx, dtype=torch.float64, device=dev)
            for z0 in range(0, nz, step):
                z1 = min(nz, z0 + step)
                src = dimg.view(img, chl, z0)
                nat.check(L.mmx_stretch(ctypes.byref(src), z1 - z0, ny, nx, float(vmin), float(vmax), slab.data_ptr(),
                                        dimg.stream()), "mmx_stretch")
                res.put(z0, z1, c_sink, slab[:(z1 - z0) * ny * nx].view(z1 - z0, ny, nx))
            torch.cuda.current_stream().synchronize()
        return None if res is None else res.value()     # (no channel processed: the reference returns None)


# ------------------------------------------------------------------------------------------------------ denoise
def erosion_gate(sum_x, sum_abs, n: int, thr) -> str:
    """Whether ``np.mean(x) > thr`` (``denoise_roi`` erodes iff it holds) as far as the device's sums can tell:
    ``"erode"``, ``"keep"``, or ``"ask"`` -- only NumPy's own summation of the voxels decides.

    Integer voxels (``sum_abs is None``, ``sum_x`` a Python int): ``np.mean`` adds the voxels as float64 in pairwise
    order; every partial sum is an integer below 2^53 and therefore exact in any order, so ``float(sum_x) / n`` IS
    NumPy's mean and the answer is never ``"ask"``.

    float64 voxels (``sum_x``, ``sum_abs``: sum x and sum |x| summed in no particular order): a float64 summation of n
    values in any order returns ``S (1 + d)`` per addition, so its error is at most ``g(n-1) sum|x|`` with ``g(k) = k u
    / (1 - k u)``, ``u = 2^-53`` (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4).  NumPy's sum and
    the device's are two such summations of the same values: they differ by at most ``2 g(n-1) sum|x|``, their means by
    at most that over n plus one rounding of each division, ``2 u |mean| <= 2 u sum|x| / n``:
    ``|m_device - m_numpy| <= ((n - 1) 2^-52 / (1 - n u) + 2^-52) (sum|x| / n) <= n 2^-52 (sum|x| / n) (1 + 2^-20)``
    for ``n < 2^32``.  The device's ``sum|x|`` is itself low by a factor of at most ``1 - g(n)``; the band below carries
    ``(n + 2) (1 + 2^-19)`` for all of it.  Outside the band both means lie on the same side of ``thr``."""
    n = int(n)
    thr = float(thr)
    if sum_abs is None:
        return "erode" if float(int(sum_x)) / float(n) > thr else "keep"
    m = float(sum_x) / n
    band = (n + 2) * 2.0 ** -52 * (float(sum_abs) / n) * (1 + 2.0 ** -19)
    if abs(m - thr) > band:                    # (False for a NaN or an infinite sum: NumPy decides)
        return "erode" if m > thr else "keep"
    return "ask"


def denoise_check_args(dtype, channels, what: str):
    """``[(channel, clip_min, clip_max, unsharp_strength, erosion_threshold)]`` of the channels :func:`denoise_roi`
    would process, the last two ``0.0`` where the reference's truthiness test skips the step -- and every refusal that
    follows from the image's dtype and the profiles alone."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        raise NotImplementedError(f"{what}: float32 images are not built (under NumPy 2 the reference stays in float32 "
                                  f"from the clip onward)")
    if dtype not in nat.NP_TO_MMX:
        raise NotImplementedError(f"{what}: {dtype} images are not built "
                                  f"({', '.join(str(d) for d in nat.NP_TO_MMX)} are)")
    todo = []
    for chl in channels:
        settings = config.get_roi_profile(chl)
        if settings["tot_var_denoise"]:
            raise NotImplementedError(f"{what}: tot_var_denoise of a whole image (channel {chl}) is not built")
        lo, hi = settings["clip_min"], settings["clip_max"]
        if dtype.kind in "iu" and all(isinstance(v, numbers.Integral) for v in (lo, hi)):
            raise NotImplementedError(f"{what}: integer clip bounds ({lo!r}, {hi!r}) keep an integer image in its own "
                                      f"type: not built (the result here is float64)")
        todo.append((chl, float(lo), float(hi), float(settings["unsharp_strength"] or 0.0),
                     float(settings["erosion_threshold"] or 0.0)))
    return todo


def _denoise_channel(img, chl: int, lo, hi, strength, thr, bufs, host_view, stats=None):
    """One channel through the passes: ``(packed float64 image on the device, eroded?)`` -- the unsharp result (or the
    clipped image) in one of ``bufs``; the erosion is the caller's, on the result's way out."""
    from . import preprocess
    L = nat.lib()
    dev = img.tensor.device
    nz, ny, nx = img.shape[:3]
    n_vox = nz * ny * nx
    stream = dimg.stream()
    src = dimg.view(img, chl)
    erode = False
    if thr:
        d_sums = torch.zeros(2, dtype=torch.int64, device=dev)
        nat.check(L.mmx_dn_sum(ctypes.byref(src), nz, ny, nx, d_sums.data_ptr(), stream), "mmx_dn_sum")
        if img.np_dtype.kind == "f":
            sx, sa = (float(v) for v in d_sums.view(torch.float64).cpu().numpy())
            verdict = erosion_gate(sx, sa, n_vox, thr)
        else:
            verdict = erosion_gate(int(d_sums[0].item()), None, n_vox, thr)
        if verdict == "ask":
            verdict = "erode" if np.mean(host_view()) > thr else "keep"
        erode = verdict == "erode"
        if stats is not None:
            stats.setdefault("verdicts", []).append(verdict)
    a, b = bufs[0], bufs[1] if len(bufs) > 1 else None
    if not strength:
        nat.check(L.mmx_dn_clip(ctypes.byref(src), nz, ny, nx, lo, hi, a.data_ptr(), stream), "mmx_dn_clip")
        return a, erode
    w = preprocess.gauss_weights()
    if w.shape != (33,):
        raise ValueError("the sigma-8 half kernel has 33 weights")
    axes = [0, 1] if preprocess.RGB_GUESS and nx == 3 else [0, 1, 2]
    cur, nxt = None, a
    for axis in axes:
        last = axis == axes[-1]
        nat.check(L.mmx_dn_blur(ctypes.byref(src), nz, ny, nx, axis, w.ctypes.data, lo, hi,
                                cur.data_ptr() if cur is not None else None, nxt.data_ptr(), int(last), strength,
                                stream), "mmx_dn_blur")
        cur, nxt = nxt, (b if nxt is a else a)
    return cur, erode


def denoise_roi(roi, channel=None, _keep=False, _out=None, _stats=None):
    """``plot_3d.denoise_roi`` of a whole ``(z, y, x[, c])`` image: per channel ``np.clip`` to the profile's ``clip_min``
    / ``clip_max``, the unsharp mask ``den + (den - unsharp_strength * gaussian(den, 8))`` unless the strength is
    falsy, and the 7-point grey erosion when ``erosion_threshold`` is truthy and ``np.mean`` of the channel exceeds it
    (:func:`erosion_gate`).  float64 for every voxel type.  A multichannel result is zero in the channels not named;
    no channel processed returns ``None``.  A truthy ``tot_var_denoise``, float32 images and an image that does not
    fit the device beside its two float64 working buffers are a ``NotImplementedError`` (:func:`denoise_check_args`).
    ``_keep=True`` leaves a float64 tensor on the device for the next task of a chain, otherwise the result leaves z-slab
    by z-slab, through ``_out`` when given; ``_stats`` (a dict, for tests and tools) receives the gate's verdicts."""
    dtype, shape, _ = dimg.describe(roi)
    multichannel, channels = _setup_channels(shape, channel)
    todo = denoise_check_args(dtype, list(channels), "denoise_roi")
    if len(shape) not in (3, 4):
        raise ValueError("image must be (z, y, x) or (z, y, x, c)")
    if not todo:
        return None                         # (no channel processed: the reference returns None)
    nz, ny, nx = (int(v) for v in shape[:3])
    n_vox = nz * ny * nx
    blurs = any(t[3] for t in todo)
    erodes = any(t[4] for t in todo)
    keep_single = _keep and not multichannel
    # float64 images kept beside the source: the passes' two (one without a blur), the eroded image when it stays on the
    # device as the result (it takes the second), every channel of a multichannel result that stays; and the slab the
    # eroded planes leave through
    n_bufs = 2 if blurs or (keep_single and erodes) else 1
    step, _ = dimg.slab_step((nz, ny, nx), 8)
    slab_bytes = step * ny * nx * 8 if erodes and not keep_single else 0
    with dimg.open_image(roi, "denoise_roi", 8 * n_bufs + (8 * shape[3] if _keep and multichannel else 0),
                         slab_bytes) as img:
        L = nat.lib()
        dev = img.tensor.device
        bufs = [torch.empty(n_vox, dtype=torch.float64, device=dev) for _ in range(n_bufs)]
        out = dimg.Result(shape, np.float64, _keep, _out, zero_fill=multichannel, device=dev)
        slab = torch.empty(slab_bytes // 8, dtype=torch.float64, device=dev) if slab_bytes else None
        for chl, lo, hi, strength, thr in todo:
            def host_view(chl=chl):
                # (the view the reference's np.mean would see: NumPy's summation order depends on the layout)
                arr = img.host()
                return arr[..., chl] if multichannel else arr
            res, erode = _denoise_channel(img, chl, lo, hi, strength, thr, bufs, host_view, _stats)
            c_out = chl if multichannel else None
            if erode and keep_single:
                other = bufs[1] if res is bufs[0] else bufs[0]
                nat.check(L.mmx_dn_erode(res.data_ptr(), nz, ny, nx, 0, nz, other.data_ptr(), dimg.stream()),
                          "mmx_dn_erode")
                res = other
            elif erode:
                for z0 in range(0, nz, step):
                    z1 = min(nz, z0 + step)
                    nat.check(L.mmx_dn_erode(res.data_ptr(), nz, ny, nx, z0, z1, slab.data_ptr(), dimg.stream()),
                              "mmx_dn_erode")
                    out.put(z0, z1, c_out, slab[:(z1 - z0) * ny * nx].view(z1 - z0, ny, nx))
            if keep_single or not erode:
                out.drain(res.view(nz, ny, nx), c_out)      # (kept, single-channel: the working buffer is the result)
            torch.cuda.current_stream().synchronize()
        return out.value()
