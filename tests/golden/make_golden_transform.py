#!/opt/conda/bin/python3.9
"""Generate ``transform.npz``: the down-sampling stage's fixtures from the REAL reference.

Run in the build container only (it needs ``/root/reference`` and the conda interpreter that has scikit-image
0.18.3), in the manner of ``make_golden.py``::

    /opt/conda/bin/python3.9 tests/golden/make_golden_transform.py

It makes a scratch, importable copy of ``/root/reference/magmap`` under ``/tmp`` and calls the real
``cv_nd.rescale_resize``, ``chunking.stack_splitter`` / ``get_split_stack_total_shape``, the three
``transformer.make_modifier_*``, ``importer.calc_scaling`` and ``skimage.util.img_as_float``.  Only inputs, parameters
and results are stored.  No reference source is copied into the repository.

(i)   ``noaa_<dtype>_in`` / ``_out``: ``cv_nd.rescale_resize(chunk, 0.25, anti_aliasing=False)`` of 12 x 20 x 18 chunks
      (uint8 / uint16 / int16 / float64).  All three axes change, so 0.18.3 resizes through ``map_coordinates`` with
      the arithmetic of the pinned release's ``zoom``.
(ii)  ``aa_in`` / ``aa_out``: ``cv_nd.rescale_resize(float64 chunk, (4, 6, 5))``, the anti-aliased chain; ``aa_sigma``
      and ``aa_w<axis>``: the sigmas and the half kernels SciPy built for its three passes under this NumPy.
(iii) ``asfloat_<dtype>_in`` / ``_out``: ``img_as_float`` at about 300 values per integer type, the extremes included.
(iv)  the plan for ``plan_shapes`` / ``plan_max_pixels``: ``plan<k>_starts`` / ``_stops`` (``stack_splitter``'s slices per
      axis, padded with -1), ``plan<k>_round<j>`` (``np.round(scale * chunk extents)`` for ``plan_scales[j]``, as
      ``skimage.transform.rescale`` rounds), ``plan<k>_total<j>`` (``get_split_stack_total_shape`` of chunks of those
      extents); ``mod_*`` the modifiers; ``scaling_*`` ``calc_scaling``.

Two things differ in 0.18.3 and cannot be pinned by it: it anti-aliases ``rescale`` by default (hence the explicit
``anti_aliasing=False`` in (i)), and it filters integer images before converting them (hence the float64 chunk in (ii)).
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCRATCH = "/tmp/mmx_refcopy_transform"


def _bootstrap():
    if os.path.isdir(SCRATCH):
        shutil.rmtree(SCRATCH)
    os.makedirs(SCRATCH)
    shutil.copytree("/root/reference/magmap", os.path.join(SCRATCH, "magmap"))
    for rel in ("magmap/io/np_io.py", "magmap/io/importer.py", "magmap/cv/cv_nd.py", "magmap/atlas/transformer.py"):
        path = os.path.join(SCRATCH, rel)
        with open(path) as f:
            src = f.read()
        with open(path, "w") as f:
            f.write("from __future__ import annotations\n" + src)
    sys.path.insert(0, SCRATCH)


_bootstrap()

import warnings  # noqa: E402

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

import scipy  # noqa: E402
import skimage  # noqa: E402
from scipy.ndimage import filters as ndi_filters  # noqa: E402
from skimage.util import img_as_float  # noqa: E402

from magmap.atlas import transformer  # noqa: E402
from magmap.cv import chunking, cv_nd  # noqa: E402
from magmap.io import importer  # noqa: E402

CHUNK = (12, 20, 18)
PLAN_SHAPES = ((13, 29, 27), (11, 29, 27), (1024, 2048, 2048), (7, 1000, 501))
PLAN_MAX_PIXELS = ((5, 12, 10), (5, 12, 10), (100, 500, 500), (3, 500, 500))
PLAN_SCALES = (0.25, 0.5)


def make_chunk(seed, dtype):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    vol = rng.normal(0.35, 0.12, CHUNK) + (rng.random(CHUNK) < 0.03) * rng.uniform(0.2, 0.6, CHUNK)
    if dtype.kind == "u":
        return np.clip(vol * np.iinfo(dtype).max, 0, np.iinfo(dtype).max).astype(dtype)
    if dtype.kind == "i":
        return np.clip((vol - 0.4) * 60000, -32768, 32767).astype(dtype)
    return ((vol - 0.3) * 900.0).astype(dtype)


def main():
    out = {"versions": np.array(repr(dict(numpy=np.__version__, scipy=scipy.__version__,
                                          skimage=skimage.__version__, python=sys.version.split()[0])))}
    for k, dt in enumerate(("uint8", "uint16", "int16", "float64")):
        chunk = make_chunk(300 + k, dt)
        res = cv_nd.rescale_resize(chunk, 0.25, anti_aliasing=False)
        out["noaa_%s_in" % dt] = chunk
        out["noaa_%s_out" % dt] = res
        print("(i)  %-8s -> %s %s" % (dt, res.shape, res.dtype))
    chunk = make_chunk(310, "float64")
    res = cv_nd.rescale_resize(chunk, (4, 6, 5))
    out["aa_in"], out["aa_out"] = chunk, res
    # the half kernels this SciPy / NumPy gave the three passes (np.exp is not bit-stable across NumPy releases)
    sig = np.maximum(0, (np.divide(chunk.shape, res.shape) - 1) / 2)
    out["aa_sigma"] = sig
    for a in range(3):
        radius = int(4.0 * sig[a] + 0.5)
        out["aa_w%d" % a] = ndi_filters._gaussian_kernel1d(sig[a], 0, radius)[radius:]
    print("(ii) float64 -> %s %s" % (res.shape, res.dtype))
    rng = np.random.default_rng(320)
    for dt in ("uint8", "uint16", "int16"):
        info = np.iinfo(dt)
        vals = np.unique(np.concatenate((rng.integers(info.min, info.max, 296, endpoint=True),
                                         [info.min, info.min + 1, info.max - 1, info.max, 0, 1]))).astype(dt)
        out["asfloat_%s_in" % dt] = vals
        out["asfloat_%s_out" % dt] = img_as_float(vals)
    out["plan_shapes"] = np.array(PLAN_SHAPES)
    out["plan_max_pixels"] = np.array(PLAN_MAX_PIXELS)
    out["plan_scales"] = np.array(PLAN_SCALES)
    for k, (shape, mp) in enumerate(zip(PLAN_SHAPES, PLAN_MAX_PIXELS)):
        slices, _ = chunking.stack_splitter(shape, list(mp))
        grid = slices.shape
        starts = -np.ones((3, max(grid)), dtype=np.int64)
        stops = -np.ones((3, max(grid)), dtype=np.int64)
        for a in range(3):
            for i in range(grid[a]):
                coord = [0, 0, 0]
                coord[a] = i
                starts[a, i] = slices[tuple(coord)][a].start
                stops[a, i] = slices[tuple(coord)][a].stop
        out["plan%d_starts" % k], out["plan%d_stops" % k] = starts, stops
        for j, scale in enumerate(PLAN_SCALES):
            rounded = -np.ones((3, max(grid)), dtype=np.int64)
            subs = np.zeros(grid, dtype=object)
            for coord in np.ndindex(*grid):
                ext = np.array([s.stop - s.start for s in slices[coord]])
                new = np.round(np.atleast_1d(scale) * ext)       # skimage.transform.rescale (_warps.py)
                subs[coord] = np.broadcast_to(np.zeros(1), tuple(int(v) for v in new))
                for a in range(3):
                    rounded[a, coord[a]] = int(new[a])
            out["plan%d_round%d" % (k, j)] = rounded
            out["plan%d_total%d" % (k, j)] = np.array(chunking.get_split_stack_total_shape(subs))
    out["mod_plane"] = np.array([transformer.make_modifier_plane(p) for p in ("xy", "xz", "yz")])
    out["mod_scale_args"] = np.array([0.25, 0.5, 2.0, 0.125])
    out["mod_scale"] = np.array([transformer.make_modifier_scale(float(s)) for s in out["mod_scale_args"]])
    out["mod_resized_args"] = np.array([[9, 10, 4], [512, 512, 256]])
    out["mod_resized"] = np.array([transformer.make_modifier_resized(list(t)) for t in out["mod_resized_args"]])
    out["mod_path"] = np.array([transformer.get_transposed_image_path("/a/b/img.czi", 0.25),
                                transformer.get_transposed_image_path("/a/b/img.czi", None, [9, 10, 4]),
                                transformer.get_transposed_image_path("/a/b/img", 0.5),
                                transformer.get_transposed_image_path("/a/b/img.czi")])
    out["scaling_shapes"] = np.array([[[1, 13, 29, 27], [1, 3, 7, 6]], [[1, 1024, 2048, 2048], [1, 256, 512, 512]]])
    out["scaling"] = np.array([importer.calc_scaling(None, None, tuple(a), tuple(b)) for a, b in out["scaling_shapes"]])
    path = os.path.join(HERE, "transform.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
