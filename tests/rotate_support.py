"""Pure-NumPy restatement of the reference's whole-image rotation, and the cases of ``tests/golden/rotate.npz``.

``cv_nd.rotate_nd`` (reference magmap/cv/cv_nd.py:81-144) runs ``skimage.transform.rotate(plane, angle, order=order,
mode="constant", preserve_range=True)`` over every plane along ``axis``; ``transformer.rotate_img`` (transformer.py:
326-350) chains it over ``rotate["rotation"]``.  What scikit-image 0.18.3 computes for one plane, stated here:

* the matrix ``T(center) R(angle) T(-center)`` with ``center = (cols / 2 - 0.5, rows / 2 - 0.5)``, in scalar arithmetic
  (:func:`rotation_matrix`); float32 planes use it rounded to float32;
* output pixel ``(tr, tc)`` reads the source at ``c = M00 tc + M01 tr + M02``, ``r = M10 tc + M11 tr + M12``, left to
  right, nothing fused;
* order 1: the bilinear mix of the four pixels at ``floor`` / ``ceil`` of ``(r, c)``, pixels outside the plane reading
  0; then the clip to the plane's own minimum and maximum (all channels of the plane), exact zeros put back when 0
  lies outside that range;
* order 0: the pixel at scikit-image's ``round`` of ``(r, c)`` (:func:`sk_round`), no clip;
* the float64 plane is stored into the image's dtype with a C cast (truncation toward zero).

``tests/golden/make_golden_rotate.py`` asserts all of this equal to the real functions on every stored case and on a
few hundred random ones.  float32 images at order 1 and ``resize=True`` are not restated (they do not reproduce).
"""
import hashlib
import math

import numpy as np

# ------------------------------------------------------------------------------------------------------ the cases
SMALL = (9, 14, 11)
ROW = (2, 3, 70)          # degenerate planes, a row longer than a wave
COL = (70, 3, 2)
TILES = (5, 67, 130)      # more than one tile both ways for any tile up to 64 x 128
ANGLES = (0, 0.22, -30, 45, 90, 180)
CHAIN = ((-5, 1), (-1, 2), (-30, 0))      # a stock profile's rotation
#: seeds of the chain inputs (uint16 with a minimum > 0; + 1: two channels; + 2: the end-to-end image)
CHAIN_SEED = 77

#: voxel kinds: (dtype, channels)
KINDS = {
    "u8": (np.uint8, 1),
    "u16": (np.uint16, 1),          # minimum 0
    "u16m": (np.uint16, 1),         # minimum > 0: the put-back of zeros, the clip up to the minimum at the border
    "i16": (np.int16, 1),           # negative values: truncation toward zero
    "f64": (np.float64, 1),         # a range that does not contain 0
    "f32": (np.float32, 1),         # order 0 only
    "u16c2": (np.uint16, 2),        # two channels of different ranges: the clip range is per plane across channels
}


def make_input(kind, shape, seed):
    """The input of a case, from its seed."""
    rng = np.random.default_rng(seed)
    dtype, n_chl = KINDS[kind]
    shape = tuple(shape)
    if kind == "u8":
        a = rng.integers(0, 256, shape)
        a.flat[0], a.flat[-1] = 0, 255
    elif kind == "u16":
        a = rng.integers(0, 60000, shape)
        a.flat[0] = 0
    elif kind == "u16m":
        a = rng.integers(20000, 50000, shape)
    elif kind == "i16":
        a = rng.integers(-30000, 30000, shape)
    elif kind == "f64":
        a = 100.0 + 50.0 * rng.random(shape)
    elif kind == "f32":
        a = (rng.random(shape) * 2 - 0.5).astype(np.float32)
    elif kind == "u16c2":
        a = np.stack([rng.integers(3000, 4000, shape), rng.integers(9000, 65000, shape)], axis=-1)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a.astype(dtype))


def _cases():
    out = []
    seed = 0

    def add(kind, shape, axes, orders, angles):
        nonlocal seed
        seed += 1
        for axis in axes:
            for order in orders:
                for angle in angles:
                    out.append((kind, tuple(shape), seed, axis, order, angle))

    add("u16", SMALL, (0, 1, 2), (0, 1), ANGLES)
    add("u8", SMALL, (0, 1, 2), (0, 1), (-30, 90))
    add("u16m", SMALL, (0, 1, 2), (0, 1), (-30, 45, 180))
    add("i16", SMALL, (0, 1, 2), (0, 1), (-30, 90))
    add("f64", SMALL, (0, 1, 2), (0, 1), (-30,))
    add("f64", SMALL, (0,), (0, 1), (90, 0.22))
    add("f32", SMALL, (0, 1, 2), (0,), (-30, 45, 90))
    add("u16c2", SMALL, (0, 1, 2), (0, 1), (-30, 90))
    add("u16m", ROW, (0, 1, 2), (0, 1), ANGLES)
    add("u16m", COL, (0, 1, 2), (0, 1), ANGLES)
    add("u8", TILES, (0, 1, 2), (0, 1), (-30,))
    return out


#: (kind, shape, seed, axis, order, angle)
CASES = _cases()


def case_name(case):
    kind, shape, seed, axis, order, angle = case
    return "%s_%s_a%d_o%d_%s" % (kind, "x".join(str(s) for s in shape), axis, order,
                                 ("%g" % angle).replace("-", "m").replace(".", "p"))


def plane_shape(shape, axis):
    """``(rows, cols)`` of the planes of a ``(z, y, x[, c])`` image along ``axis``."""
    return tuple(int(s) for i, s in enumerate(shape[:3]) if i != axis)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the restatement
def rotation_matrix(rows, cols, angle):
    """The first two rows of ``rotate``'s matrix, (2, 3) float64, in scalar arithmetic."""
    cx, cy = cols / 2 - 0.5, rows / 2 - 0.5
    a = float(np.deg2rad(angle))
    c, s = math.cos(a), math.sin(a)
    # (-s + 0.0: the products of the three matrices leave +0.0 where the sine is zero)
    return np.array([[c, -s + 0.0, c * (-cx) + (-s) * (-cy) + cx],
                     [s, c, s * (-cx) + c * (-cy) + cy]], dtype=np.float64)


def sk_round(v):
    """scikit-image's own ``round`` (``_shared/interpolation.pxd``): ``(r + .5) if r > 0 else (r - .5)``, evaluated in
    float64 (the literal is a C double, a float32 coordinate is promoted) and truncated by the cast to an index.  It is
    C's ``round`` except where the sum itself rounds: -0.49999999999999994 - 0.5 gives -1."""
    v = v.astype(np.float64)
    return np.trunc(np.where(v > 0, v + 0.5, v - 0.5))


def _pixels(img, r, c):
    """``img[r, c]`` (r, c integral floats), 0 outside; also the mask of the reads that fell outside."""
    rows, cols = img.shape
    outside = (r < 0) | (r >= rows) | (c < 0) | (c >= cols)
    ri = np.where(outside, 0, r).astype(np.int64)
    ci = np.where(outside, 0, c).astype(np.int64)
    return np.where(outside, img.dtype.type(0), img[ri, ci]), outside


def warp_channel(img, m, order, info=None):
    """One 2-D float plane through ``_warp_fast``: ``m`` (2, 3) in the plane's dtype."""
    ft = img.dtype.type
    rows, cols = img.shape
    tr, tc = np.meshgrid(np.arange(rows).astype(ft), np.arange(cols).astype(ft), indexing="ij")
    c = m[0, 0] * tc + m[0, 1] * tr + m[0, 2]
    r = m[1, 0] * tc + m[1, 1] * tr + m[1, 2]
    assert c.dtype == img.dtype
    if order == 0:
        out, outside = _pixels(img, sk_round(r), sk_round(c))
        if info is not None:
            info["fill"] = outside
        return out
    minr, minc, maxr, maxc = np.floor(r), np.floor(c), np.ceil(r), np.ceil(c)
    dr, dc = r - minr, c - minc
    tl, o1 = _pixels(img, minr, minc)
    tr_, o2 = _pixels(img, minr, maxc)
    bl, o3 = _pixels(img, maxr, minc)
    br, o4 = _pixels(img, maxr, maxc)
    top = (1 - dc) * tl + dc * tr_
    bottom = (1 - dc) * bl + dc * br
    if info is not None:
        info["fill"] = o1 | o2 | o3 | o4
    return (1 - dr) * top + dr * bottom


def rotate_plane(plane, angle, order, info=None):
    """``skimage.transform.rotate(plane, angle, order=order, mode="constant", preserve_range=True)`` of a ``(rows,
    cols[, c])`` plane: float64, or float32 for a float32 plane.  ``info`` (a dict) receives ``fill`` (reads outside
    the plane), ``raw`` (the result before the clip)."""
    plane = np.asarray(plane)
    if order not in (0, 1):
        raise NotImplementedError("orders 0 and 1 are restated")
    if plane.dtype == np.float32 and order == 1:
        raise NotImplementedError("float32 at order 1 does not reproduce")
    img = plane if plane.dtype.char in "df" else plane.astype(np.float64)
    m = rotation_matrix(plane.shape[0], plane.shape[1], angle).astype(img.dtype)
    infos = [dict() for _ in range(img.shape[2] if img.ndim == 3 else 1)]
    if img.ndim == 2:
        out = warp_channel(img, m, order, infos[0])
    else:
        out = np.dstack([warp_channel(img[..., k], m, order, infos[k]) for k in range(img.shape[2])])
    if info is not None:
        info["fill"] = infos[0]["fill"]
        info["raw"] = out.copy()
    if order != 0:
        lo, hi = img.min(), img.max()
        preserve = not (lo <= 0 <= hi)
        if preserve:
            zero = out == 0
        out = np.clip(out, lo, hi)
        if preserve:
            out[zero] = 0
    return out


def rotate_nd(img_np, angle, axis=0, order=1, infos=None):
    """``cv_nd.rotate_nd`` with ``resize=False``; ``infos`` (a list) receives every plane's ``info``."""
    img_np = np.asarray(img_np)
    is_2d = img_np.ndim == 2
    if is_2d:
        img_np = img_np[None]
    rotated = np.copy(img_np)
    slices = [slice(None)] * img_np.ndim
    for i in range(img_np.shape[axis]):
        slices[axis] = i
        info = {} if infos is not None else None
        rotated[tuple(slices)] = rotate_plane(img_np[tuple(slices)], angle, order, info)
        if infos is not None:
            infos.append(info)
    return rotated[0] if is_2d else rotated


def rotate_img(roi, rotation, order=1):
    """``transformer.rotate_img`` for ``rotate = {"rotation": rotation, "resize": False, "order": order}``."""
    roi = np.copy(roi)
    for angle, axis in rotation:
        roi = rotate_nd(roi, angle, axis, order)
    return roi
