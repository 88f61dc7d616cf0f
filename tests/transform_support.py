"""Test support for the down-sampling stage: the CPU restatement the tests compare against (test infrastructure, NOT
product code), built from SciPy calls the way the pinned scikit-image release (>= 0.19, pinned 0.25.2) chains them.

Per chunk (``cv_nd.rescale_resize`` -> ``skimage.transform.rescale`` / ``resize``, ``preserve_range=False``):

1. ``convert_to_float``: ``img_as_float`` by dtype (:func:`convert_to_float`);
2. ``rescale``: no anti-aliasing (its default from 0.19 on);
3. ``resize``: a chunk that shrinks along any axis is filtered with ``ndi.gaussian_filter(image, max(0, (in / out - 1)
   / 2), mode="mirror")``;
4. ``ndi.zoom(order=1, mode="mirror", grid_mode=True)`` to the output extent;
5. the clip to the min / max of the converted, unfiltered chunk over all of its channels.

Two points rest on the pinned release's source as restated here and are NOT pinned by a fixture, because the only
release that runs beside the reference in the build container (0.18.3) differs there: it anti-aliases ``rescale`` by
default, and it filters integer images before converting them.  Everything else is pinned by ``golden/transform.npz``.

:func:`emulate_chunk` walks the product's own tables in NumPy, operation for operation as the kernels do: host tests
hold the tables and the index-set compaction against SciPy with it, without a device.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage as ndi

from magellanmapper_amd import chunking

DTYPES = ("uint8", "uint16", "int16", "float32", "float64")


def make_volume(seed: int, shape, dtype) -> np.ndarray:
    """A seeded volume of any of the five voxel types: smooth background, bright specks, the type's extremes."""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    vol = rng.normal(0.35, 0.12, shape) + (rng.random(shape) < 0.03) * rng.uniform(0.2, 0.6, shape)
    if dtype.kind == "u":
        out = np.clip(vol * np.iinfo(dtype).max, 0, np.iinfo(dtype).max).astype(dtype)
        out.flat[0], out.flat[-1] = np.iinfo(dtype).max, 0
        return out
    if dtype.kind == "i":
        out = np.clip((vol - 0.4) * 60000, -32768, 32767).astype(dtype)
        out.flat[0], out.flat[-1] = -32768, 32767
        return out
    return ((vol - 0.3) * 900.0).astype(dtype)


def convert_to_float(arr: np.ndarray) -> np.ndarray:
    """``skimage.util.img_as_float`` (skimage/util/dtype.py ``_convert``) for the five voxel types."""
    if arr.dtype.kind == "u":
        return np.multiply(arr, 1.0 / np.iinfo(arr.dtype).max, dtype=np.float64)
    if arr.dtype.kind == "i":
        out = np.add(arr, 0.5, dtype=np.float64)
        out *= 2 / (float(np.iinfo(arr.dtype).max) - float(np.iinfo(arr.dtype).min))
        return out
    return arr


def resize_chunk_cpu(chunk: np.ndarray, out_shape, antialias: bool) -> np.ndarray:
    """Steps 1-5 for one ``(z, y, x[, c])`` chunk; per channel, one clip range."""
    out_shape = tuple(int(v) for v in out_shape)
    img = convert_to_float(chunk)
    chans = [img[..., c] for c in range(img.shape[3])] if img.ndim == 4 else [img]
    factors = np.divide(chunk.shape[:3], out_shape)
    outs = []
    for ch in chans:
        filtered = ch
        if antialias and any(o < i for o, i in zip(out_shape, ch.shape)):
            filtered = ndi.gaussian_filter(ch, np.maximum(0, (factors - 1) / 2), cval=0, mode="mirror")
        out = ndi.zoom(filtered, [1 / f for f in factors], order=1, mode="mirror", cval=0, grid_mode=True)
        assert out.shape == out_shape and out.dtype == ch.dtype
        outs.append(out)
    res = np.stack(outs, axis=-1) if img.ndim == 4 else outs[0]
    np.clip(res, img.min(), img.max(), out=res)
    return res


def swap_plane(img: np.ndarray, plane) -> np.ndarray:
    """The reference's axis swaps (transformer.py:209-218) as a view."""
    if plane in (None, "xy"):
        return img
    out = np.swapaxes(img, 0, 1)
    if plane == "yz":
        out = np.swapaxes(out, 0, 2)
    return out


def downsample_cpu(img: np.ndarray, rescale=None, target_size=None, plane=None, max_pixels=(100, 500, 500)):
    """The reference's loop (transformer.py:220-285) over the CPU chain: plan, chunk by chunk, merge."""
    vol = swap_plane(img, plane)
    sub_roi_size = None
    if target_size:                     # (beside, not behind, the test for rescale: transformer.py:229)
        tsz = list(target_size)[::-1]
        shape = vol.shape[:3]
        num_chunks = np.ceil(np.divide(shape, max_pixels))
        max_pixels = np.ceil(np.divide(shape, num_chunks)).astype(int)
        sub_roi_size = np.floor(np.divide(tsz, num_chunks)).astype(int)
    slices, _ = chunking.stack_splitter(vol.shape, max_pixels)
    subs = np.zeros(slices.shape, dtype=object)
    for coord in np.ndindex(*slices.shape):
        chunk = vol[slices[coord]]
        if rescale is not None:
            new = np.round(rescale * np.array(chunk.shape[:3])).astype(int)
        else:
            new = sub_roi_size
        subs[coord] = resize_chunk_cpu(chunk, new, rescale is None)
    return np.concatenate([np.concatenate([np.concatenate(list(subs[z, y]), axis=2) for y in range(subs.shape[1])],
                                          axis=1) for z in range(subs.shape[0])], axis=0)


def emulate_chunk(chunk: np.ndarray, out_shape, antialias: bool, sparse: bool = True) -> np.ndarray:
    """One single-channel chunk through the product's tables, in NumPy, as the kernels walk them."""
    from magellanmapper_amd import kernels1d, transformer as tr  # noqa: F401
    cur = convert_to_float(chunk)
    store = cur.dtype if cur.dtype == np.float32 else np.float64
    lo, hi = cur.min(), cur.max()
    tabs = []
    sig = tr.aa_sigmas(chunk.shape, out_shape) if antialias else np.zeros(3)
    for a in range(3):
        idx, wts = tr.axis_table(chunk.shape[a], out_shape[a])
        if sig[a] > 1e-15:
            pick, idx_c = tr.compact_axis_table(idx) if sparse else (np.arange(chunk.shape[a]), idx)
            r = kernels1d.kernel_radius(sig[a])
            w = tr.aa_weights(sig[a], r)
            n = cur.shape[a]
            line = np.moveaxis(cur, a, 0).astype(np.float64)

            def ext(i):
                if n == 1:
                    return 0
                m = i % (2 * n - 2)
                return 2 * n - 2 - m if m >= n else m
            acc = np.stack([line[c] * w[0] for c in pick])
            for k in range(r, 0, -1):
                acc = acc + np.stack([line[ext(c - k)] + line[ext(c + k)] for c in pick]) * w[k]
            cur = np.moveaxis(acc.astype(store), 0, a)
            idx = idx_c
        tabs.append((idx, wts))
    (iz, wz), (iy, wy), (ix, wx) = tabs
    v = cur.astype(np.float64)
    acc = np.zeros(tuple(out_shape))
    for a in range(2):
        for b in range(2):
            for c in range(2):
                s = v[iz[:, a][:, None, None], iy[:, b][None, :, None], ix[:, c][None, None, :]]
                acc = acc + ((s * wz[:, a][:, None, None]) * wy[:, b][None, :, None]) * wx[:, c][None, None, :]
    return np.clip(acc, lo, hi).astype(store)
