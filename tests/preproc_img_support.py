"""Test support for whole-image preprocessing: a pure-NumPy restatement of ``skimage.exposure.equalize_adapthist``
(scikit-image 0.18.3, ``exposure/_adapthist.py``, with ``img_as_uint`` / ``img_as_float`` of ``util/dtype.py`` and
``rescale_intensity`` of ``exposure/exposure.py``) for one single-channel n-D image.  Test infrastructure, NOT product
code: the fixture's maker (``golden/make_golden_preproc_img.py``) holds it against the real functions on random shapes
and parameters, the host tests hold it against the fixture, the GPU tests take the tile histograms and clipped maps
from it.  Every dtype is stated explicitly, so NumPy 1.26 and 2.2 evaluate it alike.

The cases of the fixture are stated here, once, for the maker and the tests.
"""
from __future__ import annotations

import numpy as np

NR_OF_GRAY = 2 ** 14
DTYPES = ("uint8", "uint16", "int16", "float32", "float64")


# ------------------------------------------------------------------------------------------------- dtype conversion
def img_as_uint(image: np.ndarray) -> np.ndarray:
    """``skimage.util.img_as_uint`` for the five voxel types."""
    image = np.asarray(image)
    dt = image.dtype
    if dt == np.uint16:
        return image
    if dt == np.uint8:                        # _scale(a, 8, 16): an exact upscale, (2**16 - 1) // (2**8 - 1) = 257
        return np.multiply(image, 257, dtype=np.uint16)
    if dt == np.int16:                        # _scale(a, 15, 16): up to 30 bits in int32, down by 14, negatives to 0
        b = np.multiply(image, (2 ** 30 - 1) // (2 ** 15 - 1), dtype=np.int32)
        b //= 2 ** 14
        return np.maximum(b, 0).astype(np.uint16)
    if dt.kind == "f":
        if np.min(image) < -1.0 or np.max(image) > 1.0:
            raise ValueError("Images of type float must be between -1 and 1.")
        out = np.multiply(image, 65535, dtype=dt)      # (computed in the image's own float type)
        np.rint(out, out=out)
        np.clip(out, 0, 65535, out=out)
        return out.astype(np.uint16)
    raise TypeError(dt)


def levels_of_uint(u: np.ndarray, imin: int, imax: int) -> np.ndarray:
    """``np.round(rescale_intensity(u, out_range=(0, 16383))).astype(np.uint16)`` of a uint16 array whose image has the
    minimum ``imin`` and the maximum ``imax``."""
    imin, imax = float(imin), float(imax)
    img = np.clip(u.astype(np.float64), imin, imax)
    if imin != imax:
        img = (img - imin) / (imax - imin)
        img = img * (float(NR_OF_GRAY - 1) - 0.0) + 0.0
    else:
        img = np.clip(img, 0.0, float(NR_OF_GRAY - 1))
    return np.round(img).astype(np.uint16)


def output_of_levels(lv: np.ndarray, lmin: int, lmax: int) -> np.ndarray:
    """``rescale_intensity(img_as_float(lv))`` of a uint16 array whose image has the minimum ``lmin`` and the maximum
    ``lmax``."""
    img = np.multiply(lv, 1.0 / 65535, dtype=np.float64)
    imin, imax = (float(np.multiply(np.uint16(v), 1.0 / 65535, dtype=np.float64)) for v in (lmin, lmax))
    img = np.clip(img, imin, imax)
    if imin != imax:
        img = (img - imin) / (imax - imin)
        return img * (1.0 - 0.0) + 0.0
    return np.clip(img, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------------- _adapthist
def resolve_kernel(shape, kernel_size):
    if kernel_size is None:
        kernel_size = tuple(s // 8 for s in shape)
    elif np.isscalar(kernel_size):
        kernel_size = (kernel_size,) * len(shape)
    return [int(k) for k in kernel_size]


def clip_limit_count(clip_limit, kernel_size) -> int:
    n = int(np.prod(kernel_size, dtype=np.int64))
    if clip_limit > 0.0:
        return int(np.clip(clip_limit * n, 1, None))
    return n


def clip_histogram(hist: np.ndarray, clip_limit: int):
    """``clip_histogram``; returns ``(hist, entered)``: whether the redistribution loop was entered."""
    hist = hist.astype(np.int64)
    excess_mask = hist > clip_limit
    excess = hist[excess_mask]
    n_excess = excess.sum() - excess.size * clip_limit
    hist[excess_mask] = clip_limit
    bin_incr = n_excess // hist.size
    upper = clip_limit - bin_incr
    low_mask = hist < upper
    n_excess -= hist[low_mask].size * bin_incr
    hist[low_mask] += bin_incr
    mid_mask = np.logical_and(hist >= upper, hist < clip_limit)
    mid = hist[mid_mask]
    n_excess += mid.sum() - mid.size * clip_limit
    hist[mid_mask] = clip_limit
    entered = bool(n_excess > 0)
    while n_excess > 0:
        prev_n_excess = n_excess
        for index in range(hist.size):
            under_mask = hist < clip_limit
            step_size = max(1, np.count_nonzero(under_mask) // n_excess)
            under_mask = under_mask[index::step_size]
            hist[index::step_size][under_mask] += 1
            n_excess -= np.count_nonzero(under_mask)
            if n_excess <= 0:
                break
        if prev_n_excess == n_excess:
            break
    return hist, entered


def map_histogram(hist: np.ndarray, min_val: int, max_val: int, n_pixels: int) -> np.ndarray:
    out = np.cumsum(hist, axis=-1).astype(np.float64)
    out *= (max_val - min_val) / n_pixels
    out += min_val
    np.clip(out, a_min=None, a_max=max_val, out=out)
    return out.astype(np.int64)


def clahe(image: np.ndarray, kernel_size, clip_limit, nbins, parts=None) -> np.ndarray:
    """``_clahe``: the uint16 result of a uint16 image of 14-bit levels.  ``parts`` (a dict): receives ``hist`` (tiles x
    nbins counts), ``maps`` (tiles x nbins clipped, cumulated maps), ``entered`` (per tile) and ``ns_hist``."""
    ndim = image.ndim
    dtype = image.dtype
    pad_start = [k // 2 for k in kernel_size]
    pad_end = [(k - s % k) % k + int(np.ceil(k / 2.)) for k, s in zip(kernel_size, image.shape)]
    image = np.pad(image, [[a, b] for a, b in zip(pad_start, pad_end)], mode="reflect")
    bin_size = 1 + NR_OF_GRAY // nbins
    lut = np.arange(NR_OF_GRAY)
    lut //= bin_size
    image = lut[image]

    ns_hist = [int(s / k) - 1 for s, k in zip(image.shape, kernel_size)]
    hist_blocks_shape = np.array([ns_hist, kernel_size]).T.flatten()
    order = np.array([np.arange(0, ndim * 2, 2), np.arange(1, ndim * 2, 2)]).flatten()
    hist_slices = [slice(k // 2, k // 2 + n * k) for k, n in zip(kernel_size, ns_hist)]
    hist_blocks = image[tuple(hist_slices)].reshape(hist_blocks_shape)
    hist_blocks = np.transpose(hist_blocks, axes=order)
    assembled = hist_blocks.shape
    hist_blocks = hist_blocks.reshape((int(np.prod(ns_hist)), -1))
    n_pixels = int(np.prod(kernel_size, dtype=np.int64))
    clim = clip_limit_count(clip_limit, kernel_size)

    hist = np.stack([np.bincount(b, minlength=nbins) for b in hist_blocks])
    clipped = [clip_histogram(h, clim) for h in hist]
    maps = map_histogram(np.stack([c[0] for c in clipped]), 0, NR_OF_GRAY - 1, n_pixels)
    if parts is not None:
        parts.update(hist=hist, maps=maps, entered=np.array([c[1] for c in clipped]), ns_hist=tuple(ns_hist))
    maps = maps.reshape(assembled[:ndim] + (-1,))
    map_array = np.pad(maps, [[1, 1] for _ in range(ndim)] + [[0, 0]], mode="edge")

    ns_proc = [int(s / k) for s, k in zip(image.shape, kernel_size)]
    blocks_shape = np.array([ns_proc, kernel_size]).T.flatten()
    blocks = image.reshape(blocks_shape)
    blocks = np.transpose(blocks, axes=order)
    blocks_flat_shape = blocks.shape
    blocks = np.reshape(blocks, (int(np.prod(ns_proc)), int(np.prod(blocks.shape[ndim:]))))

    coeffs = np.meshgrid(*tuple([np.arange(k) / k for k in kernel_size[::-1]]), indexing="ij")
    coeffs = [np.transpose(c).flatten() for c in coeffs]
    inv_coeffs = [1 - c for c in coeffs]

    result = np.zeros(blocks.shape, dtype=np.float32)
    for edge in np.ndindex(*([2] * ndim)):
        edge_maps = map_array[tuple([slice(e, e + n) for e, n in zip(edge, ns_proc)])]
        edge_maps = edge_maps.reshape((int(np.prod(ns_proc)), -1))
        edge_mapped = np.take_along_axis(edge_maps, blocks, axis=-1)
        edge_coeffs = np.prod([[inv_coeffs, coeffs][e][d] for d, e in enumerate(edge[::-1])], 0)
        result += (edge_mapped * edge_coeffs).astype(result.dtype)
    result = result.astype(dtype)

    result = result.reshape(blocks_flat_shape)
    rebuild = np.array([np.arange(0, ndim), np.arange(ndim, ndim * 2)]).T.flatten()
    result = np.transpose(result, axes=rebuild)
    result = result.reshape(image.shape)
    unpad = tuple([slice(a, s - b) for a, b, s in zip(pad_start, pad_end, image.shape)])
    return result[unpad]


def equalize_adapthist(image, kernel_size=None, clip_limit=0.01, nbins=256, parts=None) -> np.ndarray:
    """``skimage.exposure.equalize_adapthist`` of one single-channel image; ``parts`` as for :func:`clahe`, plus
    ``levels`` (the 14-bit image that goes in) and ``clahe`` (the uint16 image that comes out of ``_clahe``)."""
    u = img_as_uint(np.asarray(image))
    lv = levels_of_uint(u, int(u.min()), int(u.max()))
    kernel_size = resolve_kernel(lv.shape, kernel_size)
    out = clahe(lv, kernel_size, clip_limit, nbins, parts)
    if parts is not None:
        parts.update(levels=lv, clahe=out)
    return output_of_levels(out, int(out.min()), int(out.max()))


# ------------------------------------------------------------------------------------------------------- the cases
def nuclei(seed: int, shape, n_blobs=None) -> np.ndarray:
    """The nuclei-like synthetic: background N(500, 50), Gaussian blobs of amplitude 40000, uint16."""
    from magellanmapper_amd import synth
    return synth.make_volume(seed, shape, n_blobs, margin=2)


def as_dtype(vol_u16: np.ndarray, dtype) -> np.ndarray:
    """The uint16 synthetic in another voxel type (int16: shifted below zero; floats: in [0, 1], a few below 0)."""
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return vol_u16
    if dtype == np.uint8:
        return np.minimum(vol_u16 // 16, 255).astype(np.uint8)
    if dtype == np.int16:
        return (vol_u16.astype(np.int32) - 600).clip(-32768, 32767).astype(np.int16)
    out = (vol_u16 / 65535.0).astype(dtype)
    out.flat[3] = -0.25                       # (img_as_uint clips a negative float to 0)
    return out


#: the single-channel equalisation cases: name -> (input key, kernel_size, clip_limit, nbins)
SMALL = (16, 24, 33)
EQ_CASES = {
    "nodiv": ("u16_17_40_51", None, 0.01, 256),                 # default kernel (2, 5, 6): no axis divides
    "nodiv_c10": ("u16_17_40_51", None, 0.1, 256),
    "odd": ("u16_16_24_33", (5, 7, 9), 0.01, 256),              # odd kernels, padding longer than a tile
    "k1": ("u16_8_8_8", None, 0.01, 256),                       # kernel 1
    "wide": ("u16_33_70_130", (16, 35, 65), 0.01, 256),         # a tile over several waves and workgroups
    "clip0": ("u16_16_24_33", None, 0, 256),
    "clip10": ("u16_16_24_33", None, 0.1, 256),
    "clip100": ("u16_16_24_33", None, 1.0, 256),
    "bins64": ("u16_16_24_33", None, 0.01, 64),
    "bins16384": ("u16_16_24_33", None, 0.01, 16384),
    "const": ("const_16_24_33", None, 0.01, 256),
    "uint8": ("uint8_16_24_33", None, 0.01, 256),
    "int16": ("int16_16_24_33", None, 0.01, 256),
    "float32": ("float32_16_24_33", None, 0.01, 256),
    "float64": ("float64_16_24_33", None, 0.01, 256),
    "scalar_kernel": ("u16_16_24_33", 4, 0.05, 128),
}
#: inputs regenerated from their seed instead of stored (the fixture holds their SHA-256)
SEEDED = {"u16_33_70_130": (7, (33, 70, 130), 12)}


def make_input(key: str) -> np.ndarray:
    kind, *dims = key.split("_")
    shape = tuple(int(d) for d in dims)
    if kind == "const":
        return np.full(shape, 7, dtype=np.uint16)
    if key in SEEDED:
        seed, shp, n_blobs = SEEDED[key]
        return nuclei(seed, shp, n_blobs)
    base = nuclei(11 + sum(shape), shape, 4)
    return as_dtype(base, "uint16" if kind == "u16" else kind)


def pack_float(levels: np.ndarray, result: np.ndarray):
    """A float64 result that is a function of its uint16 image, as ``(distinct levels, their float64 values)``."""
    uniq, first = np.unique(levels.ravel(), return_index=True)
    vals = result.ravel()[first]
    assert np.array_equal(vals[np.searchsorted(uniq, levels)], result)
    return uniq, vals


def unpack_float(levels: np.ndarray, uniq: np.ndarray, vals: np.ndarray) -> np.ndarray:
    return vals[np.searchsorted(uniq, levels)]


# ------------------------------------------------------------------------------------ the product's tables, in NumPy
def load_case(fx, name):
    """``(input, kernel_size, clip_limit, nbins, clahe, result)`` of one stored equalisation case."""
    import hashlib
    key, ks, cl, nb = EQ_CASES[name]
    if key in SEEDED:
        img = make_input(key)
        digest = hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest()
        assert digest == str(fx["eq_%s_sha" % name]), "the seeded input %s is not the one the fixture was made from" % key
    else:
        img = fx["in_%s" % key]
    lv = fx["eq_%s_clahe" % name]
    return img, ks, cl, nb, lv, unpack_float(lv, fx["eq_%s_uniq" % name], fx["eq_%s_vals" % name])


def emulate_apply(bins_img: np.ndarray, maps: np.ndarray, tiles: np.ndarray, coef: np.ndarray, nt, nbins) -> np.ndarray:
    """What ``eq_apply_kernel`` computes from the product's tables, operation for operation: the eight float64 products
    rounded to float32 and added in float32 in ``np.ndindex(2, 2, 2)`` order, truncated to uint16."""
    nz, ny, nx = bins_img.shape
    tz, ty, tx = tiles[:nz], tiles[nz:nz + ny], tiles[nz + ny:]
    cz, cy, cx = coef[:nz], coef[nz:nz + ny], coef[nz + ny:]
    m4 = maps.reshape(tuple(nt) + (nbins,)).astype(np.float64)
    r = np.zeros(bins_img.shape, np.float32)
    for ez, ey, ex in np.ndindex(2, 2, 2):
        mv = m4[tz[:, ez][:, None, None], ty[:, ey][None, :, None], tx[:, ex][None, None, :], bins_img]
        c = (cx[:, ex][None, None, :] * cy[:, ey][None, :, None]) * cz[:, ez][:, None, None]
        r += (mv * c).astype(np.float32)
    return r.astype(np.uint16)
