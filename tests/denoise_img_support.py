"""Shared by ``tests/golden/make_golden_denoise_img.py`` and the whole-image denoise tests: the seeded inputs, the
fixture's cases and the profile set-up -- pure NumPy, importable by the fixture generator's interpreter."""
import hashlib

import numpy as np

#: axes shorter than the kernel radius 32, between R and 2R, and longer than 2R
SHAPE = (9, 37, 70)
SHAPE2 = (9, 20, 33, 2)
SHAPE_RGB = (8, 9, 3)
SHAPE_CHAIN = (9, 12, 33)


def f64_image(seed: int, shape) -> np.ndarray:
    """float64 in [0, 1): the square of a uniform draw (one exact IEEE product; mean 1/3, above the default
    ``erosion_threshold`` 0.2, a fifth of the voxels below the default ``clip_min`` 0.2)."""
    u = np.random.default_rng(seed).random(shape)
    return u * u


def int_image(seed: int, shape, dtype) -> np.ndarray:
    """Small integers around the clip bounds: 0..3 (uint8, uint16), -2..3 (int16)."""
    dtype = np.dtype(dtype)
    lo = -2 if dtype.kind == "i" else 0
    return np.random.default_rng(seed).integers(lo, 4, shape).astype(dtype)


def chain_image() -> np.ndarray:
    """The small uint16 stack of the ``["saturate", "denoise"]`` chain: a dense nuclei-like synthetic whose stretched
    mean lies above the erosion threshold."""
    rng = np.random.default_rng(77)
    return rng.integers(300, 3000, SHAPE_CHAIN).astype(np.uint16)


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


#: settings of the second channel's profile in the two-channel cases (the first keeps the defaults)
CHANNEL1 = dict(clip_min=0.1, clip_max=0.9, unsharp_strength=0.5, erosion_threshold=0.3)

#: the fixture's function-level cases: name -> (input maker, profile settings per channel, ``channel``)
CASES = {
    "f64_default": (lambda: f64_image(1, SHAPE), [{}], None),
    "f64_noero": (lambda: f64_image(1, SHAPE), [dict(erosion_threshold=0.9)], None),
    "f64_nounsharp": (lambda: f64_image(1, SHAPE), [dict(unsharp_strength=0)], None),
    "u16": (lambda: int_image(2, SHAPE, np.uint16), [{}], None),
    "i16": (lambda: int_image(3, SHAPE, np.int16), [{}], None),
    "two_all": (lambda: f64_image(4, SHAPE2), [{}, CHANNEL1], None),
    "two_c1": (lambda: f64_image(4, SHAPE2), [{}, CHANNEL1], [1]),
    "rgb": (lambda: f64_image(5, SHAPE_RGB), [{}], None),
}


def set_profiles(config, setup, over):
    """One default profile per entry of ``over`` with its settings stored: ``setup`` is ``config.setup_roi_profiles`` here
    and ``cli.setup_roi_profiles`` in the reference."""
    setup(["default"] * len(over) if len(over) > 1 else None)
    for prof, settings in zip(config.roi_profiles, over):
        for k, v in settings.items():
            prof[k] = v
    return [dict(p) for p in config.roi_profiles]
