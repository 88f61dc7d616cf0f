#!/opt/conda/bin/python3.9
"""Generate ``bounds.npz``: intensity bounds from the REAL reference.

Run in the build container only (it needs ``/root/reference`` and the conda interpreter that has scikit-image), in
the manner of ``make_golden.py``::

    /opt/conda/bin/python3.9 tests/golden/make_golden_bounds.py

It makes a scratch, importable copy of ``/root/reference/magmap`` under ``/tmp``, imports the real
``magmap.io.importer`` and calls its ``calc_intensity_bounds`` and ``calc_near_intensity_bounds`` on seeded volumes
that a test regenerates from ``(seed, shape, dtype)`` alone (:func:`make_bounds_volume`, restated in the tests; a
CRC-32 of every volume is stored so that a generator that drifted is noticed).  Only parameters and results are
stored.  No reference source is copied into the repository.

Per case ``<name>``: ``_seed``, ``_shape``, ``_dtype``, ``_crc``; for every percentile pair ``k`` of ``pcts``:
``_whole_lows_k`` / ``_whole_highs_k`` (``calc_intensity_bounds`` on the ``(t, z, y, x[, c])`` image),
``_plane_lows_k`` / ``_plane_highs_k`` (``calc_intensity_bounds(image5d[0, i], dim_channel=2)`` for every plane, as
the metadata upgrade calls it, importer.py:572-581) and ``_near_min_k`` / ``_near_max_k``
(``calc_near_intensity_bounds`` on those lists).
"""
import os
import shutil
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
SCRATCH = "/tmp/mmx_refcopy_bounds"


def _bootstrap():
    if os.path.isdir(SCRATCH):
        shutil.rmtree(SCRATCH)
    os.makedirs(SCRATCH)
    shutil.copytree("/root/reference/magmap", os.path.join(SCRATCH, "magmap"))
    for rel in ("magmap/io/np_io.py", "magmap/io/importer.py"):
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

from magmap.io import importer  # noqa: E402

PCTS = ((0.5, 99.5), (0.0, 100.0), (5.0, 50.0))
CASES = (("u16", 101, (24, 96, 112), "uint16"),
         ("u8", 102, (9, 37, 53), "uint8"),
         ("u16_2ch", 103, (12, 40, 48, 2), "uint16"),
         ("f64", 104, (6, 33, 47), "float64"))


def make_bounds_volume(seed, shape, dtype):
    """A seeded image with a narrow background histogram and a sparse bright tail (what a microscope plane looks
    like to a percentile); float64 volumes are centred on zero, so that they hold negative values."""
    rng = np.random.default_rng(seed)
    vol = rng.normal(500.0, 50.0, shape)
    bright = rng.random(shape) < 0.02
    vol = vol + bright * rng.uniform(0.0, 40000.0, shape)
    dtype = np.dtype(dtype)
    if dtype == np.uint16:
        return np.clip(vol, 0, 65535).astype(np.uint16)
    if dtype == np.uint8:
        return np.clip(vol / 16.0, 0, 255).astype(np.uint8)
    if dtype == np.float64:
        return (vol - 520.0) / 97.0
    raise ValueError(dtype)


def main():
    out = {"names": np.array([c[0] for c in CASES]), "pcts": np.array(PCTS),
           "versions": np.array(repr(dict(numpy=np.__version__, python=sys.version.split()[0])))}
    for name, seed, shape, dtype in CASES:
        vol = make_bounds_volume(seed, shape, dtype)
        image5d = vol[None]
        out[name + "_seed"] = np.array(seed)
        out[name + "_shape"] = np.array(shape)
        out[name + "_dtype"] = np.array(dtype)
        out[name + "_crc"] = np.array(zlib.crc32(np.ascontiguousarray(vol).tobytes()), dtype=np.uint32)
        for k, (lower, upper) in enumerate(PCTS):
            lows, highs = importer.calc_intensity_bounds(image5d, lower, upper)
            out["%s_whole_lows_%d" % (name, k)] = np.array(lows, dtype=np.float64)
            out["%s_whole_highs_%d" % (name, k)] = np.array(highs, dtype=np.float64)
            plane_lows, plane_highs = [], []
            for i in range(len(image5d[0])):
                low, high = importer.calc_intensity_bounds(image5d[0, i], lower, upper, dim_channel=2)
                plane_lows.append(low)
                plane_highs.append(high)
            near_mins, near_maxs = importer.calc_near_intensity_bounds([], [], plane_lows, plane_highs)
            out["%s_plane_lows_%d" % (name, k)] = np.array(plane_lows, dtype=np.float64)
            out["%s_plane_highs_%d" % (name, k)] = np.array(plane_highs, dtype=np.float64)
            out["%s_near_min_%d" % (name, k)] = np.array(near_mins, dtype=np.float64)
            out["%s_near_max_%d" % (name, k)] = np.array(near_maxs, dtype=np.float64)
        print("%-8s %s %s: near_min %s near_max %s" % (name, shape, dtype, out[name + "_near_min_0"],
                                                        out[name + "_near_max_0"]))
    np.savez_compressed(os.path.join(HERE, "bounds.npz"), **out)


if __name__ == "__main__":
    main()
