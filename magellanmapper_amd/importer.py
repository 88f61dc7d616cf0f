"""On-disk image format on the input side of the detection path.

Mirror of the parts of ``magmap.io.importer`` / ``magmap.io.np_io`` that ``mm <img> --proc detect``
goes through before ``stack_detect.detect_blobs_stack`` (reference magmap/io/importer.py):

* ``<base>_image5d.npy`` -- the ``(t, z, y, x[, c])`` array, opened memory-mapped (:794);
* ``<base>_meta.yml``    -- YAML metadata written by :func:`save_image_info` (:482-522): ``ver``
  (``IMAGE5D_NP_VER`` = 15, :69), ``names``, ``sizes``, ``resolutions``, ``magnification``, ``zoom``,
  ``near_min``, ``near_max``, ``scaling``, ``plane``; pre-v1.4 archives kept the same keys in
  ``<base>_meta.npz`` (:636-650);
* :func:`load_metadata` / :func:`assign_metadata` (:602-745) push ``resolutions``, ``magnification``,
  ``zoom``, ``near_min`` and ``near_max`` into :mod:`config`, which is where the detection path and
  the preprocessing read them.

* :func:`measure_near_bounds` / :func:`calc_intensity_bounds` / :func:`calc_near_intensity_bounds` (:1367-1377,
  1415-1468) measure ``near_min`` / ``near_max`` of an image that carries no metadata, the order statistics on the
  device.

Importing from TIFF / Bio-Formats, metadata version upgrades and ROI loading stay in the reference.
The device side: :class:`blob_log.DeviceVolume` uploads a memory-mapped image plane block by plane
block through a pinned staging buffer, so the host never holds a second copy of the stack.
"""
from __future__ import annotations

import logging
import os
from typing import Any, Dict, Optional, Sequence, Tuple

import numpy as np
import yaml

from . import _native as nat
from . import config, device_image
from .stack_detect import Image5d

_logger = logging.getLogger("magellanmapper_amd")

IMAGE5D_NP_VER = 15
SUFFIX_IMAGE5D = "image5d.npy"
SUFFIX_META = "meta.yml"
_EXTENSIONS_MULTIPLE = (".tar", ".nii")


def splitext(path: str) -> Tuple[str, str]:
    """``libmag.splitext`` (reference libmag.py:272-293): multi-dot extensions stay whole."""
    i = -1
    for ext in _EXTENSIONS_MULTIPLE:
        i = path.rfind(ext)
        if i != -1:
            break
    if i == -1:
        return os.path.splitext(path)
    return path[:i], path[i:]


def combine_paths(base_path: Optional[str], suffix: str, sep: str = "_", keep_ext: bool = False) -> str:
    """``libmag.combine_paths`` (libmag.py:331-369) without the ``ext`` / ``check_dir`` options."""
    if not base_path:
        return suffix
    if not os.path.basename(base_path):
        return os.path.join(base_path, suffix)
    return (base_path if keep_ext else splitext(base_path)[0]) + sep + suffix


def filename_to_base(filename: str, series: Optional[int] = None, modifier: str = "",
                     keep_ext: bool = False) -> str:
    path = filename if keep_ext else splitext(filename)[0]
    if modifier:
        path = combine_paths(path, modifier, keep_ext=True)
    return path


def make_filenames(filename: str, series: Optional[int] = None, modifier: str = "",
                   keep_ext: bool = False) -> Tuple[str, str]:
    """``(path of the image5d array, path of its metadata)`` (importer.py:272-301)."""
    base = filename_to_base(filename, series, modifier, keep_ext)
    return (combine_paths(base, SUFFIX_IMAGE5D, keep_ext=True),
            combine_paths(base, SUFFIX_META, keep_ext=True))


def _primitives(val):
    if isinstance(val, dict):
        return {k: _primitives(v) for k, v in val.items()}
    if isinstance(val, (list, tuple, np.ndarray)):
        return [_primitives(v) for v in val]
    try:
        return val.item()
    except AttributeError:
        return val


def save_image_info(filename_info, names, sizes, resolutions, magnification, zoom, near_min, near_max,
                    scaling=None, plane=None) -> Dict[str, Any]:
    """Write the metadata YAML exactly as the reference does (importer.py:482-522,
    yaml_io.py:94-143 with ``use_primitives=True``)."""
    data = _primitives({
        "ver": IMAGE5D_NP_VER, "names": names, "sizes": sizes, "resolutions": resolutions,
        "magnification": magnification, "zoom": zoom, "near_min": near_min, "near_max": near_max,
        "scaling": scaling, "plane": plane})
    with open(filename_info, "w") as f:
        yaml.dump(data, f)
    return data


def load_metadata(path: str, check_ver: bool = False, img5d: Optional[Image5d] = None):
    """``(metadata dict | None, version)``; YAML first, the pre-v1.4 ``.npz`` as a fallback
    (importer.py:602-664)."""
    ver = -1
    try:
        with open(path) as f:
            docs = [d for d in yaml.load_all(f, Loader=yaml.FullLoader) if d]
        output = docs[0] if docs else None
    except FileNotFoundError:
        path_npz = f"{os.path.splitext(path)[0]}.npz"
        try:
            with np.load(path_npz, allow_pickle=True) as arc:
                output = {k: (v.item() if v.ndim == 0 else v) for k, v in arc.items()}
        except FileNotFoundError:
            _logger.warning("Could not load metadata file '%s', skipping", path_npz)
            return None, ver
    if output is None:
        return None, ver
    try:
        ver = output["ver"]
    except KeyError:
        pass
    if img5d is not None and (not check_ver or ver >= IMAGE5D_NP_VER):
        assign_metadata(img5d, output)
    return output, ver


def assign_metadata(img5d: Image5d, md: Dict[str, Any]) -> None:
    """Push the metadata into the module globals the path reads (importer.py:667-745)."""
    if "sizes" in md:
        img5d.shapes = md["sizes"]
    if "resolutions" in md:
        config.resolutions = np.array(md["resolutions"])
    if "magnification" in md:
        config.magnification = md["magnification"]
    if "zoom" in md:
        config.zoom = md["zoom"]
    if "near_min" in md:
        config.near_min = md["near_min"]
    if "near_max" in md:
        config.near_max = md["near_max"]


def read_file(filename: str, series: Optional[int] = None, offset=None, size=None,
              update_info: bool = True) -> Image5d:
    """Open ``<base>_image5d.npy`` memory-mapped with its metadata (importer.py:748-829).
    A missing image leaves ``img5d.img`` as ``None`` like the reference (the caller raises)."""
    if offset is not None or size is not None:
        raise NotImplementedError("loading only an ROI of the image stays in the reference")
    if series is None:
        series = 0
    path_img, path_meta = make_filenames(filename, series)
    img5d = Image5d(None, path_img, path_meta, "np")
    try:
        md, ver = load_metadata(path_meta, update_info, img5d)
        img5d.meta = md
        if md is not None and update_info and -1 < ver < IMAGE5D_NP_VER:
            raise NotImplementedError(
                f"image5d metadata version {ver} < {IMAGE5D_NP_VER}: upgrade it with the reference")
        img5d.img = np.load(path_img, mmap_mode="r")
    except OSError as err:
        _logger.warning("Could not load image files for %s: %s", filename, err)
    return img5d


# ---- near_min / near_max: the intensity bounds of the WHOLE image that the preprocessing's contrast stretch reads
# (config.near_max[chl] * max_thresh_factor, reference plot_3d.py:98-100).  The reference measures them while it
# imports a stack -- np.percentile of every plane, the smallest low and the largest high per channel
# (importer.py:1367-1377) -- or when it upgrades old metadata (:572-585, calc_intensity_bounds +
# calc_near_intensity_bounds).  Here the order statistics come from the device (DeviceVolume.order_stats) and the
# percentile is assembled from them on the host in NumPy's arithmetic.

#: z-chunk size (bytes) of a host image that `measure_near_bounds` walks in pieces; ``None``: a third of the device
#: memory free at the call, and no chunking at all for an image below that
BOUNDS_CHUNK_BYTES = None

_BOUNDS_DTYPES = nat.voxel_dtypes(integer=True) + (nat.MMX_TO_NP[nat.MMX_F64],)
_BOUNDS_NAMES = "uint8, uint16, int16 and float64 are supported"


def _bounds_dtype_ok(dtype) -> bool:
    """The types above, and float32 once ``preprocess.FLOAT32_RULES`` names NumPy 2's rules (a float32 difference of
    the two order statistics, the rest of ``_lerp`` in float64): the switch the preprocessing reads, at call time."""
    if dtype in _BOUNDS_DTYPES:
        return True
    from . import preprocess
    return np.dtype(dtype) == np.dtype(np.float32) and preprocess.float32_rules() == "numpy2"


def percentile_from_order_stats(a_prev, a_next, gamma, dtype):
    """``np.percentile(a, pct)`` (method "linear") from ``sorted(a)[prev]``, ``sorted(a)[next]`` and ``gamma`` of
    :func:`preprocess.quantile_ranks`, in float64, as NumPy's ``_lerp`` assembles it
    (numpy/lib/_function_base_impl.py): ``a + (b - a) * g``, replaced by ``b - (b - a) * (1 - g)`` where
    ``g >= 0.5``, with ``b - a`` taken in the input type -- for int16 the difference of two order statistics more than
    32767 apart WRAPS, in NumPy and here; for float32 (``preprocess.FLOAT32_RULES = "numpy2"``) it is a float32
    difference, rounded once, while the products and sums are float64.  Scalars or arrays; returns float64."""
    dtype = np.dtype(dtype)
    if not _bounds_dtype_ok(dtype):
        raise NotImplementedError(f"percentiles of {dtype} images ({_BOUNDS_NAMES})")
    a = np.asarray(a_prev).astype(dtype)
    b = np.asarray(a_next).astype(dtype)
    g = np.asarray(gamma, dtype=np.float64)
    with np.errstate(all="ignore"):
        diff = np.subtract(b, a)
        out = np.add(a, diff * g, dtype=np.float64)
        alt = np.subtract(b, diff * (1 - g), dtype=np.float64)
    out = np.where(g >= 0.5, alt, out)
    return out[()] if out.ndim == 0 else out


def _bounds_ranks(n: int, lower, upper):
    from .preprocess import quantile_ranks
    lo_prev, lo_next, lo_g = quantile_ranks(n, lower)
    hi_prev, hi_next, hi_g = quantile_ranks(n, upper)
    return np.array([lo_prev, lo_next, hi_prev, hi_next], dtype=np.int64), lo_g, hi_g


def _percentiles_of_groups(dv, channel: int, groups, lower, upper):
    """``np.percentile(group, (lower, upper))`` of z-ranges of one channel of a device volume: ``(lows, highs)``."""
    if not _bounds_dtype_ok(dv.np_dtype):
        raise NotImplementedError(f"percentiles of {dv.np_dtype} images ({_BOUNDS_NAMES})")
    plane = int(dv.shape[1]) * int(dv.shape[2])
    ranks, gammas = [], []
    for z0, z1 in groups:
        rk, lo_g, hi_g = _bounds_ranks((z1 - z0) * plane, lower, upper)
        ranks.append(rk)
        gammas.append((lo_g, hi_g))
    stats, has_nan = dv.order_stats(channel, np.array(ranks, dtype=np.int64).reshape(-1, 4), groups)
    gam = np.array(gammas, dtype=np.float64).reshape(-1, 2)
    lows = percentile_from_order_stats(stats[:, 0], stats[:, 1], gam[:, 0], dv.np_dtype)
    highs = percentile_from_order_stats(stats[:, 2], stats[:, 3], gam[:, 1], dv.np_dtype)
    lows = np.where(has_nan, np.nan, lows)      # (NumPy: a slice that holds a NaN yields NaN)
    highs = np.where(has_nan, np.nan, highs)
    return lows, highs


def _as_zyxc(arr, multichannel: bool):
    """An image of any rank as ``(z, y, x[, c])`` without copying: the leading spatial axes are folded into z."""
    spatial = arr.shape[:-1] if multichannel else arr.shape
    if len(spatial) == 0:
        raise ValueError("image without spatial axes")
    lead = int(np.prod(spatial[:-2], dtype=np.int64)) if len(spatial) > 2 else 1
    zyx = (lead, spatial[-2] if len(spatial) > 1 else 1, spatial[-1])
    return arr.reshape(zyx + ((arr.shape[-1],) if multichannel else ()))


def calc_intensity_bounds(image5d, lower=0.5, upper=99.5, dim_channel=4):
    """Percentiles of each channel over the WHOLE image (importer.py:1415-1444): ``(lows, highs)``, one entry per
    channel.  The image -- a NumPy array, a memory map or a ``DeviceVolume`` -- is multichannel when it has more than
    ``dim_channel`` axes (the channel is the last one), as ``plot_3d.setup_channels`` decides it.  One order-statistics
    group spans the image, so it has to fit the device: ``ValueError`` otherwise (per-plane bounds,
    :func:`measure_near_bounds`, walk an image of any size)."""
    from .volume import DeviceVolume
    if isinstance(image5d, DeviceVolume):
        dv = image5d
        multichannel = dv.multichannel
    else:
        arr = image5d if isinstance(image5d, np.ndarray) else np.asarray(image5d)
        multichannel = arr.ndim > dim_channel
        if not _bounds_dtype_ok(arr.dtype):
            raise NotImplementedError(f"percentiles of {arr.dtype} images ({_BOUNDS_NAMES})")
        if arr.size == 0:
            raise ValueError("empty image")
        if arr.nbytes > 0.9 * device_image.free_bytes():
            raise ValueError(
                f"whole-image bounds need the image on the device at once: {arr.nbytes} bytes do not fit "
                f"({device_image.free_bytes()} free); measure_near_bounds walks a larger image plane by plane")
        dv = DeviceVolume(_as_zyxc(arr, multichannel), streamed=False)
    z0 = dv.z_off
    group = [(z0, z0 + int(dv.tensor.shape[0]))]
    lows, highs = [], []
    for c in range(dv.n_channels):
        lo, hi = _percentiles_of_groups(dv, c, group, lower, upper)
        lows.append(lo[0])
        highs.append(hi[0])
    return lows, highs


def save_np_image(image, filename, series=None):
    """Save an image as ``<base>_image5d.npy`` with its ``<base>_meta.yml`` (importer.py:1471-1497): the metadata comes
    from the settings in :mod:`config`, the near minimum / maximum from :func:`calc_intensity_bounds` of the image."""
    filename_image5d, filename_info = make_filenames(filename, series)
    with open(filename_image5d, "wb") as out_file:
        np.save(out_file, image)
    lows, highs = calc_intensity_bounds(image)
    save_image_info(filename_info, [os.path.basename(filename)], [image.shape], config.resolutions,
                    config.magnification, config.zoom, lows, highs)


def roi_to_image5d(roi):
    """An ROI in image5d format: a time axis in front (importer.py:1537-1547)."""
    return roi[None]


def calc_scaling(image5d, scaled, image5d_shape=None, scaled_shape=None) -> np.ndarray:
    """``z, y, x`` factors from an image to its rescaled copy (importer.py:1500-1535): shapes of four axes and more
    lose their time axis first; either array may be ``None`` when its shape is given."""
    if image5d_shape is None:
        image5d_shape = image5d.shape
    if scaled_shape is None:
        scaled_shape = scaled.shape
    if len(image5d_shape) >= 4:
        image5d_shape = image5d_shape[1:4]
    if len(scaled_shape) >= 4:
        scaled_shape = scaled_shape[1:4]
    return np.divide(scaled_shape[:3], image5d_shape[:3])


def calc_near_intensity_bounds(near_mins, near_maxs, lows, highs):
    """Near min / max from lists of per-plane ``lows`` / ``highs`` (importer.py:1447-1468; no device): with one
    channel the extremes are APPENDED to the lists given, with several the per-channel minima / maxima come back as
    new arrays."""
    if lows:
        if len(lows[0]) <= 1:
            near_mins.append(min(lows)[0])
            near_maxs.append(max(highs)[0])
        else:
            near_mins = np.amin(np.array(lows), 0)
            near_maxs = np.amax(np.array(highs), 0)
    return near_mins, near_maxs


def measure_near_bounds(img, lower=0.5, upper=99.5, assign=False):
    """``(near_min, near_max)``, one entry per channel, as the reference's import loop measures them
    (importer.py:1367-1377): ``np.percentile(plane, (lower, upper))`` of every z-plane, the smallest low and the
    largest high per channel.

    ``img``: a ``(z, y, x[, c])`` array, memory map or ``DeviceVolume``, a ``(t, z, y, x, c)`` array, or an
    ``Image5d`` (``(t, z, y, x[, c])``); of a time series the first time point is measured, as the reference does.
    A bare four-axis array is read as ``(z, y, x, c)``, like everywhere in this package: a single-channel
    ``(t, z, y, x)`` array goes in as ``Image5d(arr)`` or ``arr[0]``.
    A host image larger than the device (or than ``BOUNDS_CHUNK_BYTES``) is walked in z-chunks of whole planes, the
    next chunk on its way up while the current one is counted.  ``assign``: also store the result in
    ``config.near_min`` / ``config.near_max`` -- what a caller does before ``detect_blobs_stack`` when the image carries
    no reference metadata."""
    from .volume import DeviceVolume
    if isinstance(img, Image5d):
        arr = img.img
        if arr is None:
            raise ValueError("Image5d without an image")
        if arr.ndim not in (4, 5):
            raise ValueError("an Image5d holds (t, z, y, x[, c])")
        arr = arr[0]
    elif isinstance(img, DeviceVolume):
        arr = img
    else:
        arr = img if isinstance(img, np.ndarray) else np.asarray(img)
        if arr.ndim == 5:
            arr = arr[0]
        if arr.ndim not in (3, 4):
            raise ValueError("image must be (z, y, x[, c]) or (t, z, y, x, c)")

    lows, highs = None, None

    def measure(dv):
        z0 = dv.z_off
        groups = [(z, z + 1) for z in range(z0, z0 + int(dv.tensor.shape[0]))]
        for c in range(dv.n_channels):
            lo, hi = _percentiles_of_groups(dv, c, groups, lower, upper)
            lows[c].extend(lo)
            highs[c].extend(hi)

    if isinstance(arr, DeviceVolume):
        lows, highs = [[] for _ in range(arr.n_channels)], [[] for _ in range(arr.n_channels)]
        measure(arr)
    else:
        if not _bounds_dtype_ok(arr.dtype):
            raise NotImplementedError(f"percentiles of {arr.dtype} images ({_BOUNDS_NAMES})")
        if arr.size == 0:
            raise ValueError("empty image")
        n_chl = arr.shape[3] if arr.ndim == 4 else 1
        lows, highs = [[] for _ in range(n_chl)], [[] for _ in range(n_chl)]
        nz = arr.shape[0]
        limit = BOUNDS_CHUNK_BYTES if BOUNDS_CHUNK_BYTES is not None else device_image.free_bytes() // 3
        plane_bytes = max(1, arr.nbytes // nz)
        step = nz if arr.nbytes <= limit else max(1, int(limit // plane_bytes))
        starts = list(range(0, nz, step))

        def upload(z0):
            return DeviceVolume(arr[z0:min(z0 + step, nz)], streamed=len(starts) > 1 or None, z_off=z0,
                                full_shape=arr.shape[:3])

        nxt = upload(starts[0])
        for k in range(len(starts)):
            cur, nxt = nxt, (upload(starts[k + 1]) if k + 1 < len(starts) else None)
            try:
                measure(cur)
            except BaseException:
                if nxt is not None:
                    nxt.close()
                raise
            finally:
                cur.close()
    near_min = [min(v) for v in lows]
    near_max = [max(v) for v in highs]
    if assign:
        config.near_min = near_min
        config.near_max = near_max
    return near_min, near_max
