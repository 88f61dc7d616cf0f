#!/opt/conda/bin/python3.9
"""Generate ``rotate.npz``: the whole-image rotation fixtures from the REAL reference.

Run in the build container only (it needs ``/root/reference`` and the conda interpreter that has scikit-image
0.18.3), in the manner of ``make_golden_preproc_img.py``::

    /opt/conda/bin/python3.9 tests/golden/make_golden_rotate.py

It makes a scratch, importable copy of ``/root/reference/magmap`` under ``/tmp`` and calls the real
``cv_nd.rotate_nd``, ``transformer.rotate_img`` and ``transformer.preprocess_img``.  Only inputs, parameters and
results are stored.  No reference source is copied into the repository.

(i)   ``rot_<case>`` for every case of ``rotate_support.CASES``: ``cv_nd.rotate_nd(input, angle, axis, order)`` in full;
      ``sha_<kind>_<shape>_<seed>``: the SHA-256 of the input (the tests regenerate it from its seed).
(ii)  ``mat_keys`` (n, 3: rows, cols, angle) / ``mat_vals`` (n, 2, 3): the first two rows of the matrix
      ``skimage.transform.rotate`` builds for every plane shape and angle used.
(iii) ``chain_o<order>``: ``transformer.rotate_img`` of the uint16 input ``chain_in`` (seed ``CHAIN_SEED``) for the stock
      rotation ``rotate_support.CHAIN`` at orders 0 and 1; ``chain_c2``: of a two-channel image at order 1.
(iv)  ``e2e_*``: ``transformer.preprocess_img(image5d, ["saturate", "rotate"], None, path)`` with that rotation in the
      atlas profile: the float64 result, ``lows`` / ``highs`` of the metadata written; ``settings`` / ``near_max`` as
      in ``preproc_img.npz``.

Asserted while it runs: the NumPy restatement of ``tests/rotate_support.py`` equals the real functions on every stored
case, on 300 random ``rotate_nd`` calls and on the chains; and, so that no case passes vacuously,

* every order-1 case whose angle is no multiple of 90 differs from the order-0 result in at least a quarter of its
  voxels and reads outside its planes (fill) somewhere.  The shapes with degenerate planes (2 x 3, 3 x 70, ...: an
  extent below 9) are the exception: a 3 x 70 plane turned by 30 degrees is seven eighths fill in both orders, and a
  shape large enough for a quarter of the whole would no longer be degenerate; there the quarter is taken of the voxels
  the order-0 result reads inside the plane;
* every "minimum > 0" volume (``u16m``, ``f64``, ``u16c2``) holds, over the order-1 cases of its shape at -30 or 45
  degrees, voxels clipped up to the minimum and voxels put back to 0, and each single such case whose planes are at
  least 9 x 9 holds both on its own (a 2 x 3 plane turned by 30 degrees has no pixel with all four reads outside:
  no shape cures that, so the degenerate planes are counted with their volume);
* the int16 order-1 cases hold negative non-integer interpolants (what the truncation toward zero acts on).
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCRATCH = "/tmp/mmx_refcopy_rotate"


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
    sys.path.insert(0, os.path.dirname(HERE))                       # tests/: rotate_support


_bootstrap()

import contextlib  # noqa: E402
import io  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

import skimage  # noqa: E402
from skimage import transform as sk_transform  # noqa: E402

from magmap.atlas import transformer  # noqa: E402
from magmap.cv import cv_nd  # noqa: E402
from magmap.io import cli  # noqa: E402
from magmap.settings import config  # noqa: E402

import rotate_support as sup  # noqa: E402

CHAIN_SEED = sup.CHAIN_SEED
NEAR_MAX = [30000.0, 70000.0]


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def real_matrix(rows, cols, angle):
    """The matrix ``rotate`` hands to ``warp`` (scikit-image's own construction)."""
    center = np.array((cols, rows)) / 2. - 0.5
    t1 = sk_transform.SimilarityTransform(translation=center)
    t2 = sk_transform.SimilarityTransform(rotation=np.deg2rad(angle))
    t3 = sk_transform.SimilarityTransform(translation=-center)
    return (t3 + t2 + t1).params


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def main():
    out = {"versions": np.array(repr(dict(numpy=np.__version__, skimage=skimage.__version__,
                                          python=sys.version.split()[0])))}
    inputs, results, infos_of = {}, {}, {}
    mats = {}
    for case in sup.CASES:
        kind, shape, seed, axis, order, angle = case
        key = (kind, shape, seed)
        if key not in inputs:
            inputs[key] = sup.make_input(kind, shape, seed)
            out["sha_%s_%s_%d" % (kind, "x".join(str(s) for s in shape), seed)] = np.array(sup.sha(inputs[key]))
        img = inputs[key]
        want = quiet(cv_nd.rotate_nd, img, angle, axis, order)
        infos = []
        got = sup.rotate_nd(img, angle, axis, order, infos)
        assert same(got, want), case
        assert want.dtype == img.dtype and want.shape == img.shape, case
        results[case], infos_of[case] = want, infos
        out["rot_" + sup.case_name(case)] = want
        rows, cols = sup.plane_shape(shape, axis)
        m = real_matrix(rows, cols, angle)
        assert np.array_equal(m[2], [0, 0, 1])
        assert np.array_equal(sup.rotation_matrix(rows, cols, angle), m[:2]), (rows, cols, angle)
        mats[(rows, cols, float(angle))] = m[:2]
    print("(i)   %d cases, restatement == cv_nd.rotate_nd on all" % len(sup.CASES))

    # ---- the conditions that keep a case from passing vacuously
    both_of_volume = {}
    for case in sup.CASES:
        kind, shape, seed, axis, order, angle = case
        if order != 1 or angle % 90 == 0:
            continue
        nearest = results[(kind, shape, seed, axis, 0, angle)]
        rows, cols = sup.plane_shape(shape, axis)
        differ = np.count_nonzero(nearest != results[case])
        if min(rows, cols) >= 9:
            assert differ >= 0.25 * nearest.size, (case, differ)
        else:
            inside = sum(int((~i["fill"]).sum()) for i in infos_of[(kind, shape, seed, axis, 0, angle)])
            inside *= sup.KINDS[kind][1]
            assert differ >= 0.25 * inside and differ > 0, (case, differ, inside)
        fill = sum(int(i["fill"].sum()) for i in infos_of[case])
        assert fill > 0, case
        img = inputs[(kind, shape, seed)]
        if kind in ("u16m", "f64", "u16c2") and angle in (-30, 45):
            up = back = 0
            for p, info in enumerate(infos_of[case]):
                sl = [slice(None)] * img.ndim
                sl[axis] = p
                lo = img[tuple(sl)].min()
                raw = info["raw"]
                up += int(((raw > 0) & (raw < lo)).sum())
                back += int((raw == 0).sum())
            rows, cols = sup.plane_shape(shape, axis)
            if min(rows, cols) >= 9:
                assert up > 0 and back > 0, (case, up, back)
            acc = both_of_volume.setdefault((kind, shape, seed), [0, 0])
            acc[0] += up
            acc[1] += back
        if kind == "i16":
            neg = sum(int(((i["raw"] < 0) & (i["raw"] != np.trunc(i["raw"]))).sum()) for i in infos_of[case])
            assert neg > 0, case
    for key, (up, back) in both_of_volume.items():
        assert up > 0 and back > 0, (key, up, back)
        print("      %-26s clipped up to min: %d, put back to 0: %d" % (key[:2], up, back))

    # ---- the restatement against the real function beyond the stored cases
    rng = np.random.default_rng(0)
    kinds = [k for k in sup.KINDS]
    for i in range(300):
        kind = kinds[i % len(kinds)]
        shape = tuple(int(v) for v in rng.integers(1, 24, 3))
        img = sup.make_input(kind, shape, 1000 + i)
        angle = float(rng.choice([-30, -5, -4, -2, -1, -0.4, 0.22, 1, 1.5, 2, 45, 90, 180, 270,
                                  rng.uniform(-360, 360)]))
        axis = int(rng.integers(0, 3))
        order = 0 if kind == "f32" else int(rng.integers(0, 2))
        if i % 10 == 9 and kind != "u16c2":
            img, axis = img[0], 0                                    # (a 2-D image)
        want = quiet(cv_nd.rotate_nd, img, angle, axis, order)
        assert same(sup.rotate_nd(img, angle, axis, order), want), (kind, shape, angle, axis, order)
        rows, cols = img.shape if img.ndim == 2 else sup.plane_shape(shape, axis)
        assert np.array_equal(sup.rotation_matrix(rows, cols, angle), real_matrix(rows, cols, angle)[:2])
    print("      restatement == cv_nd.rotate_nd on 300 random cases")

    keys = sorted(mats)
    out["mat_keys"] = np.array(keys, dtype=np.float64)
    out["mat_vals"] = np.array([mats[k] for k in keys], dtype=np.float64)

    # (iii) the stock chain through the reference's rotate_img
    chain_in = sup.make_input("u16m", sup.SMALL, CHAIN_SEED)
    out["chain_sha"] = np.array(sup.sha(chain_in))
    for order in (0, 1):
        rot = {"rotation": sup.CHAIN, "resize": False, "order": order}
        want = quiet(transformer.rotate_img, chain_in, rot)
        assert same(sup.rotate_img(chain_in, sup.CHAIN, order), want)
        assert want.any() and not np.array_equal(want, chain_in)
        out["chain_o%d" % order] = want
    two = sup.make_input("u16c2", sup.SMALL, CHAIN_SEED + 1)
    out["chain_c2_sha"] = np.array(sup.sha(two))
    want = quiet(transformer.rotate_img, two, {"rotation": sup.CHAIN, "resize": False, "order": 1})
    assert same(sup.rotate_img(two, sup.CHAIN, 1), want)
    out["chain_c2"] = want

    # (iv) end to end through the reference's own task loop
    quiet(cli.setup_roi_profiles, None)
    config.near_max = list(NEAR_MAX)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    prof = config.get_roi_profile(0)
    out["settings"] = np.array([prof["clip_vmin"], prof["clip_vmax"], prof["max_thresh_factor"],
                                prof["adapt_hist_lim"]], dtype=np.float64)
    out["near_max"] = np.array(NEAR_MAX)
    config.atlas_profile = {"rotate": {"rotation": sup.CHAIN, "resize": False, "order": 1}}
    src = sup.make_input("u16", sup.SMALL, CHAIN_SEED + 2)
    out["e2e_sha"] = np.array(sup.sha(src))
    base = os.path.join(SCRATCH, "e2e")
    res5d = quiet(transformer.preprocess_img, src[None], ["saturate", "rotate"], None, base)
    assert res5d.shape == (1,) + src.shape and res5d.dtype == np.float64
    from magmap.plot import plot_3d
    sat = quiet(plot_3d.saturate_roi, src, channel=None)
    assert sat.dtype == np.float64 and same(sup.rotate_img(sat, sup.CHAIN, 1), res5d[0])
    out["e2e_out"] = res5d[0]
    import yaml
    with open(base + "_meta.yml") as f:
        meta = yaml.safe_load(f)
    out["e2e_lows"], out["e2e_highs"] = np.array(meta["near_min"]), np.array(meta["near_max"])

    path = os.path.join(HERE, "rotate.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < 800 * 1024


if __name__ == "__main__":
    main()
