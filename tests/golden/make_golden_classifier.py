#!/opt/conda/bin/python3.9
"""Generate ``classifier.npz`` from the REAL ``magmap.cv.classifier``.

Run in the build container only (it needs ``/root/reference`` and the conda interpreter, like ``make_golden.py``,
whose bootstrap this repeats)::

    /opt/conda/bin/python3.9 tests/golden/make_golden_classifier.py

The reference loads its model with ``tensorflow.keras.models.load_model``; TensorFlow is not installed, so a stand-in
module of that name is put into ``sys.modules`` whose model's ``predict(x)`` returns the centre voxel of each patch --
no arithmetic, so the expected ``confirmed`` columns are exact.  Everything else that runs is the reference's own code.
Only inputs and outputs (``.npz`` data) are stored.

``classifier.npz``:

* ``vol`` (230, 40, 36) uint16 and ``vol_ch1`` (a second channel): 16 grey levels, an all-zero 20 x 20 corner in a few
  planes (patches whose maximum is 0: 0 / 0); ``crop_u8`` / ``crop_f32`` / ``crop_f64``: casts of planes 0..11, the
  float ones with a NaN voxel.
* ``table`` (~300, 8): blobs on and beside the y / x rim of both patch sizes, in the zero corner, at z = 0, 99, 100, 229,
  outside the volume, of both channels; ``crop_table``: interior blobs of the crop.
* ``patches_<dtype>_<size>``: ``extract_patches`` of the crop (and of its channel 1 as ``patches_u16c1_<size>``) for
  sizes 16, 5 and 2; ``patches_vol_<size>``: of the whole volume for the interior rows ``interior_<size>`` of ``table``.
* ``roi<k>_*``: ``setup_classification_roi`` for the whole image and two sub-images.
* ``confirmed_16`` / ``confirmed_5`` (``channels=[0]``) and ``confirmed_16_ch1`` (the two-channel volume,
  ``channels=[1]``): the column after ``ClassifyImage.classify_whole_image``.
"""
import contextlib
import io
import os
import shutil
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
SCRATCH = "/tmp/mmx_refcopy_classifier"


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


class CentreModel:
    """The stand-in model: the score of a patch is its centre voxel (the blob's own voxel over the patch maximum)."""

    def predict(self, x):
        return x[:, x.shape[1] // 2, x.shape[2] // 2, 0]


def _stub_tensorflow():
    tf = types.ModuleType("tensorflow")
    keras = types.ModuleType("tensorflow.keras")
    models = types.ModuleType("tensorflow.keras.models")
    models.load_model = lambda path: CentreModel()
    tf.keras, keras.models = keras, models
    sys.modules.update({"tensorflow": tf, "tensorflow.keras": keras, "tensorflow.keras.models": models})


_bootstrap()
_stub_tensorflow()

import warnings  # noqa: E402

import numpy as np  # noqa: E402

warnings.filterwarnings("ignore")

from magmap.settings import config  # noqa: E402
from magmap.io import cli  # noqa: E402
from magmap.cv import chunking, classifier, detector  # noqa: E402

COLS = ["z", "y", "x", "radius", "confirmed", "truth", "channel", "region"]
SHAPE = (230, 40, 36)
SIZES = (16, 5, 2)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def make_volumes():
    rng = np.random.default_rng(2024)
    vols = []
    for _ in range(2):
        v = (rng.integers(0, 16, SHAPE) * 4000).astype(np.uint16)
        for z in (0, 3, 5, 99, 100, 229):
            v[z, :20, :20] = 0
        vols.append(v)
    return vols


def make_table(rng):
    nz, ny, nx = SHAPE
    rows = []
    rim_y = [7, 8, 31, 32, 1, 2, 37, 38]                # size // 2 - 1, size // 2, n - size // 2 - 1, n - size // 2
    rim_x = [7, 8, 27, 28, 1, 2, 33, 34]
    for y in rim_y:
        for x in rim_x:
            rows.append((int(rng.integers(0, nz)), y, x))
    for z in (0, 99, 100, 229):
        rows += [(z, 9, 9), (z, 10, 11), (z, 3, 3), (z, 25, 20), (z, 8, 8), (z, 31, 27)]
    rows += [(3, 9, 10), (5, 11, 9), (3, 2, 2), (5, 4, 5)]                    # the zero corner
    rows += [(230, 20, 20), (-1, 20, 20), (10, 40, 20), (10, 20, 36), (10, -1, 20), (231, 8, 8)]   # outside the volume
    n_rand = 300 - len(rows)
    rand = np.stack([rng.integers(0, n, n_rand) for n in SHAPE], axis=1)
    table = np.full((300, 8), -1.0)
    table[:, :3] = np.concatenate((np.array(rows, dtype=float), rand))
    table[:, 3] = 5.196152422706632
    table[:, 6] = rng.integers(0, 2, len(table))
    table[::17, 4] = 1                                   # a few rows come with a classification already
    table[5::23, 4] = 0
    return table


def run_whole(image5d, table, channels, patch_size):
    blobs = detector.Blobs(table.copy(), cols=COLS)
    quiet(classifier.ClassifyImage.classify_whole_image, "stand-in", image5d, channels, blobs, patch_size=patch_size)
    return blobs.blobs[:, 4].copy()


def main():
    out = {}
    config.cpus = 4
    quiet(cli.setup_roi_profiles, ["/root/reference/profiles/roi_blobs.yaml"])     # (the start method is a profile setting)
    quiet(chunking.set_mp_start_method)
    vol, vol_ch1 = make_volumes()
    rng = np.random.default_rng(7)
    table = make_table(rng)
    out["vol"], out["vol_ch1"], out["table"], out["cols"] = vol, vol_ch1, table, np.array(COLS)

    crop = vol[:12]
    crop_u8 = (crop // 256).astype(np.uint8)
    crop_f32 = (crop / 65535.0).astype(np.float32)
    crop_f64 = crop / 65535.0 * 1.7 + 0.01
    crop_f32[6, 20, 18] = np.nan
    crop_f64[7, 22, 16] = np.nan
    crop_f64[2, 30:, 24:] *= -1.0                        # an all-negative corner: the maximum is the least negative
    out.update(crop_u8=crop_u8, crop_f32=crop_f32, crop_f64=crop_f64)
    crop_rows = [(0, 8, 8), (11, 31, 28), (3, 9, 10), (5, 11, 9), (6, 20, 18), (6, 27, 25), (7, 22, 16), (7, 15, 9),
                 (2, 31, 28), (2, 30, 27)]
    crop_rand = np.stack([rng.integers(0, 12, 33), rng.integers(8, 32, 33), rng.integers(8, 29, 33)], axis=1)
    crop_table = np.concatenate((np.array(crop_rows), crop_rand)).astype(float)
    out["crop_table"] = crop_table
    crop2 = np.stack((crop, vol_ch1[:12]), axis=-1)
    for size in SIZES:
        for name, roi in (("u16", crop), ("u8", crop_u8), ("f32", crop_f32), ("f64", crop_f64),
                          ("u16c1", crop2[..., 1])):
            x = classifier.extract_patches(roi, crop_table, size)
            out["patches_%s_%d" % (name, size)] = x
            print("patches %-6s size %2d: %s %s, %d NaN" % (name, size, x.shape, x.dtype, int(np.isnan(x).sum())))

    image5d = vol[None]
    blobs = detector.Blobs(table.copy(), cols=COLS)
    for size in SIZES:
        _, mask, _ = classifier.setup_classification_roi(image5d, (0, 0, 0), SHAPE, blobs, size)
        out["interior_%d" % size] = mask
        out["patches_vol_%d" % size] = classifier.extract_patches(vol, table[mask], size)
        print("whole image, size %d: %d of %d blobs inside the rim" % (size, int(mask.sum()), len(mask)))

    subimgs = [((0, 0, 0), SHAPE, 16), ((10, 5, 4), (6, 20, 16), 16), ((220, 25, 20), (20, 30, 30), 5)]
    for k, (offset, size3, patch) in enumerate(subimgs):
        roi, mask, shift = classifier.setup_classification_roi(image5d, offset, size3, blobs, patch)
        out["roi%d_offset" % k], out["roi%d_size" % k], out["roi%d_patch" % k] = (
            np.array(offset), np.array(size3), np.array(patch))
        out["roi%d_shape" % k] = np.array(roi.shape)
        if k:
            out["roi%d_roi" % k] = roi
        else:
            assert np.array_equal(roi, vol)
        out["roi%d_mask" % k], out["roi%d_shift" % k] = mask, np.asarray(shift)
        print("roi %d: %s, %d blobs, shift %s" % (k, roi.shape, int(mask.sum()), shift))

    out["confirmed_16"] = run_whole(image5d, table, [0], 16)
    out["confirmed_5"] = run_whole(image5d, table, [0], 5)
    out["confirmed_16_ch1"] = run_whole(np.stack((vol, vol_ch1), axis=-1)[None], table, [1], 16)
    for k in ("confirmed_16", "confirmed_5", "confirmed_16_ch1"):
        print(k, {int(v): int(n) for v, n in zip(*np.unique(out[k], return_counts=True))})
    out["versions"] = np.array(repr(dict(numpy=np.__version__, python=sys.version.split()[0])))
    path = os.path.join(HERE, "classifier.npz")
    np.savez_compressed(path, **out)
    print("classifier.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
