#!/opt/conda/bin/python3.9
"""Generate ``denoise_img.npz``: the whole-image denoise fixtures from the REAL reference.

Run in the build container only (it needs ``/root/reference`` and the conda interpreter that has scikit-image
0.18.3), in the manner of ``make_golden_preproc_img.py``::

    /opt/conda/bin/python3.9 tests/golden/make_golden_denoise_img.py

It makes a scratch, importable copy of ``/root/reference/magmap`` under ``/tmp`` and calls the real
``plot_3d.denoise_roi`` and ``transformer.preprocess_img``.  Only inputs, parameters and results are stored.  No
reference source is copied into the repository.

(i)   ``gauss8_weights``: the full sigma-8 kernel (65 taps) SciPy built in this run (``np.exp`` differs by an ulp between
      NumPy releases; the tests install its upper half through ``preprocess.GAUSS_WEIGHTS_OVERRIDE`` and the whole
      through the oracle's ``GAUSS_WEIGHTS``).
(ii)  ``<case>_sha`` / ``<case>_out`` for every case of ``denoise_img_support.CASES``: the SHA-256 of the seeded input
      (the tests regenerate it and compare the digest) and ``plot_3d.denoise_roi``'s result; ``<case>_mean``: ``np.mean``
      of every processed channel as the reference saw it.
(iii) ``chain_sha`` / ``chain_out`` / ``chain_lows`` / ``chain_highs`` / ``chain_near_max``:
      ``transformer.preprocess_img(image5d, ["saturate", "denoise"], None, path)`` of a small uint16 stack and the
      intensity bounds of the metadata written.

Asserted while it runs: ``oracle.preprocess_oracle.denoise_roi`` equals the real function on every stored case and on 48
further random shapes, voxel types and settings; erosion is on in the default cases and off in ``f64_noero``.
"""
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCRATCH = "/tmp/mmx_refcopy_denoise_img"


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
    sys.path.insert(0, os.path.dirname(HERE))                       # tests/: denoise_img_support
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the repository: oracle


_bootstrap()

import contextlib  # noqa: E402
import io  # noqa: E402
import warnings  # noqa: E402

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

import skimage  # noqa: E402
from scipy.ndimage import filters as ndi_filters  # noqa: E402

from magmap.atlas import transformer  # noqa: E402
from magmap.io import cli  # noqa: E402
from magmap.plot import plot_3d  # noqa: E402
from magmap.settings import config  # noqa: E402

import denoise_img_support as sup  # noqa: E402
from oracle import preprocess_oracle as ppo  # noqa: E402

CHAIN_NEAR_MAX = [4000.0]


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def profiles(over):
    return sup.set_profiles(config, lambda names: quiet(cli.setup_roi_profiles, names), over)


def both(img, over, channel):
    """The real function's result, asserted equal to the oracle's."""
    profs = profiles(over)
    want = quiet(plot_3d.denoise_roi, img, channel)
    got = ppo.denoise_roi(img, profs, channel)
    assert want.dtype == np.float64 and got.dtype == want.dtype and want.shape == img.shape
    assert np.array_equal(got, want), (img.shape, img.dtype, over, channel)
    return want


def main():
    out = {"versions": np.array(repr(dict(numpy=np.__version__, skimage=skimage.__version__,
                                          python=sys.version.split()[0])))}
    weights = ndi_filters._gaussian_kernel1d(8.0, 0, 32)[::-1]
    assert weights.shape == (65,) and np.array_equal(weights, weights[::-1])
    out["gauss8_weights"] = weights
    ppo.GAUSS_WEIGHTS = weights

    # (ii) the function-level cases
    for name, (make, over, channel) in sup.CASES.items():
        img = make()
        res = both(img, over, channel)
        out[name + "_sha"] = np.array(sup.sha(img))
        out[name + "_out"] = res
        chls = [0] if img.ndim == 3 else (range(img.shape[3]) if channel is None else channel)
        out[name + "_mean"] = np.array([np.mean(img[..., c] if img.ndim == 4 else img) for c in chls])
        print("(ii)  %-14s %s %s mean %s" % (name, img.shape, img.dtype, out[name + "_mean"]))
    # erosion on / off where the cases say so, and the RGB guess of scikit-image 0.18
    profs = profiles([{}])
    img = sup.f64_image(1, sup.SHAPE)
    assert not np.array_equal(out["f64_default_out"], out["f64_noero_out"])
    assert np.array_equal(ppo.denoise_roi(img, [dict(profs[0], erosion_threshold=0)]), out["f64_noero_out"])
    assert out["two_c1_out"][..., 0].max() == 0 and np.all(out["two_c1_out"][..., 1] != 0)
    assert np.array_equal(out["two_c1_out"][..., 1], out["two_all_out"][..., 1])

    # the oracle against the real function beyond the stored cases
    rng = np.random.default_rng(0)
    dtypes = ("float64", "uint16", "int16", "uint8")
    for i in range(48):
        shape = tuple(int(v) for v in rng.integers(1, 40, 3))
        if i % 8 == 0:
            shape = shape[:2] + (3,)
        dt = dtypes[i % 4]
        img = sup.f64_image(100 + i, shape) if dt == "float64" else sup.int_image(100 + i, shape, dt)
        over = dict(clip_min=float(rng.choice([0.0, 0.1, 0.2, 0.5])), clip_max=float(rng.choice([0.7, 1.0, 2.5])),
                    unsharp_strength=rng.choice([0, 0.3, 1.5]).item(),
                    erosion_threshold=rng.choice([0, 0.2, 0.35, 5.0]).item())
        both(img, [over], None)
    print("      oracle == plot_3d.denoise_roi on 48 random cases")

    # (iii) the chain, end to end through the reference's own task loop
    profiles([{}])
    config.near_max = list(CHAIN_NEAR_MAX)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    src = sup.chain_image()
    base = os.path.join(SCRATCH, "chain")
    res5d = quiet(transformer.preprocess_img, src[None], ["saturate", "denoise"], None, base)
    assert res5d.shape == (1,) + src.shape and res5d.dtype == np.float64
    sat = quiet(plot_3d.saturate_roi, src, channel=None)
    assert sat.dtype == np.float64 and np.mean(sat) > 0.2
    assert np.array_equal(ppo.denoise_roi(sat, [dict(config.roi_profile)]), res5d[0])
    out["chain_sha"] = np.array(sup.sha(src))
    out["chain_out"] = np.array(res5d)
    out["chain_near_max"] = np.array(CHAIN_NEAR_MAX)
    import yaml
    with open(base + "_meta.yml") as f:
        meta = yaml.safe_load(f)
    out["chain_lows"], out["chain_highs"] = np.array(meta["near_min"]), np.array(meta["near_max"])

    path = os.path.join(HERE, "denoise_img.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote %s (%d bytes)" % (path, size))
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
