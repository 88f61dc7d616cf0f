"""The cases and CPU references of the table-side kernels that read image voxels -- ``mmx_unmix_batch`` (reference
magmap/cv/detector.py:910-921) and ``mmx_coloc_means`` / ``mmx_coloc_voxels`` (magmap/cv/colocalizer.py:372-441) --
and the host tests that show each case DISCRIMINATES: the GPU module (``test_gpu_table_kernels.py``) runs the same
cases on the device.  Every reference is the NumPy expression of the reference's source line, evaluated in the
image's own dtype: what matters is float32, which NumPy keeps in float32 (product, difference, clip; pairwise sum,
quotient, percentile) where uint8 / uint16 promote to float64."""
import functools
import types
import warnings

import numpy as np
import pytest

from oracle import coloc_oracle

DTYPES = ("uint8", "uint16", "float32", "float64")
SENTINEL = -7.25           # no unmixed voxel is negative, and no source voxel reaches below -1


def make_image(dtype: str, shape, seed: int) -> np.ndarray:
    """A random image of the voxel type: whole range for integers, [-1, 2) for floats (negative voxels: the clip)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    if dt.kind == "u":
        return rng.integers(0, int(np.iinfo(dt).max) + 1, shape).astype(dt)
    return (rng.random(shape) * 3 - 1).astype(dt)


def assert_bits_equal(got: np.ndarray, want: np.ndarray, err_msg: str = "") -> None:
    """Same dtype, same values and -- floats -- the same bits (``assert_array_equal`` alone takes -0.0 for 0.0)."""
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape, err_msg)
    np.testing.assert_array_equal(got, want, err_msg=err_msg)
    if got.dtype.kind == "f":
        as_int = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        np.testing.assert_array_equal(np.ascontiguousarray(got).view(as_int), np.ascontiguousarray(want).view(as_int),
                                      err_msg=err_msg)


# ------------------------------------------------------------------------------------------ spectral unmixing
UNMIX_SHAPE = (15, 14, 70, 3)              # (z, y, x, c): interleaved channels, the kernels' stride_x is 3
UNMIX_CHANNEL = 1
UNMIX_ORIGINS = [(1, 2, 3), (7, 0, 5), (2, 9, 11), (11, 3, 4)]
UNMIX_EXTENTS = [(5, 6, 7), (1, 1, 1), (9, 4, 33), (3, 8, 65)]       # widths around the 32-float row pitch
UNMIX_MAX = 8                              # MMX_UNMIX_MAX
UNMIX_CASES = {
    "none": [],
    "one": [(0, 0.4)],
    "two_clip_between": [(0, 1.5), (2, -0.5)],
    "same_channel_twice": [(0, 0.3), (0, 0.3)],
    "negative_factor": [(2, -0.7)],
    "eight": [(0, 0.11), (2, 0.07), (0, -0.05), (2, 0.13), (1, 0.02), (0, 0.09), (2, -0.03), (0, 0.01)],
}
UNMIX_NINE = UNMIX_CASES["eight"] + [(2, 0.05)]


def unmix_reference(roi: np.ndarray, channel: int, subtract, clip_every_step: bool = True) -> np.ndarray:
    """detector.py:910-921 on one ``(z, y, x, c)`` block, in NumPy's own promotion of the image's dtype.
    ``clip_every_step=False``: the clip once, after the last subtraction (NOT the reference; to tell the two apart)."""
    x = roi[..., channel]
    for k, fac in subtract:
        x = np.subtract(x, fac * roi[..., k])
        if clip_every_step:
            x[x < 0] = 0
    if subtract and not clip_every_step:
        x[x < 0] = 0
    return x


def unmix_float64_formula(roi: np.ndarray, channel: int, subtract) -> np.ndarray:
    """The same steps with every operand widened to float64 first (what a float32 image must NOT go through)."""
    x = roi[..., channel].astype(np.float64)
    for k, fac in subtract:
        x = x - fac * roi[..., k].astype(np.float64)
        x[x < 0] = 0
    return x


def unmix_blocks(img: np.ndarray):
    return [img[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]] for o, s in zip(UNMIX_ORIGINS, UNMIX_EXTENTS)]


@functools.lru_cache(maxsize=None)
def unmix_image(dtype: str) -> np.ndarray:
    img = make_image(dtype, UNMIX_SHAPE, 31)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("dtype", DTYPES)
def test_unmix_reference_dtypes(dtype):
    """What NumPy makes of the reference's line: float32 stays float32, everything else becomes float64."""
    blocks = unmix_blocks(unmix_image(dtype))
    for name, subtract in UNMIX_CASES.items():
        for blk in blocks:
            out = unmix_reference(blk, UNMIX_CHANNEL, subtract)
            if not subtract:
                assert out.dtype == np.dtype(dtype)
            else:
                assert out.dtype == (np.float32 if dtype == "float32" else np.float64), name
                assert out.min() >= 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_unmix_clip_between_the_steps_changes_the_result(dtype):
    """The two-step case tells a clip after every subtraction from one clip at the end."""
    subtract = UNMIX_CASES["two_clip_between"]
    differ = 0
    for blk in unmix_blocks(unmix_image(dtype)):
        differ += int(np.count_nonzero(unmix_reference(blk, UNMIX_CHANNEL, subtract)
                                       != unmix_reference(blk, UNMIX_CHANNEL, subtract, clip_every_step=False)))
    assert differ > 100


@pytest.mark.parametrize("case", [c for c in UNMIX_CASES if c != "none"])
def test_unmix_float32_cases_differ_from_the_float64_formula(case):
    """Every float32 case with a subtraction tells NumPy's float32 arithmetic from float64 arithmetic rounded at the
    end (``none`` subtracts nothing: a copy is a copy in either)."""
    subtract = UNMIX_CASES[case]
    differ = 0
    for blk in unmix_blocks(unmix_image("float32")):
        want = unmix_reference(blk, UNMIX_CHANNEL, subtract)
        assert want.dtype == np.float32
        differ += int(np.count_nonzero(want != unmix_float64_formula(blk, UNMIX_CHANNEL, subtract).astype(np.float32)))
    assert differ >= 1, case


def test_unmix_float32_synthetic_volumes_differ_in_a_sixth_of_the_voxels():
    """Two scaled synthetic channels, factor 0.4: NumPy's float32 result against the float64 formula rounded to
    float32 -- thousands of voxels differ, a blob table need not."""
    from magellanmapper_amd import synth
    roi = np.stack([synth.make_volume(s, (24, 32, 40), 20) / 65535 for s in (1, 2)], axis=-1).astype(np.float32)
    want = unmix_reference(roi, 0, [(1, 0.4)])
    other = unmix_float64_formula(roi, 0, [(1, 0.4)]).astype(np.float32)
    assert want.dtype == np.float32 and np.count_nonzero(want != other) > want.size // 20


def _stub_volume(dtype):
    return types.SimpleNamespace(tensor=types.SimpleNamespace(ndim=4), n_channels=2, np_dtype=np.dtype(dtype),
                                 multichannel=True, shape=(8, 8, 8, 2))


@pytest.mark.parametrize("dtype", ["uint8", "uint16"])
@pytest.mark.parametrize("factor", [1, np.int64(2), True])
def test_integer_unmixing_factor_on_an_integer_image_is_refused(dtype, factor):
    """``1 * roi[..., k]`` of an integer image stays in the image's integer type in the reference, and the subtraction
    wraps around: not what the device computes, so the profile is refused where it is read -- before any device work
    (the volume here is a stand-in without a device)."""
    from magellanmapper_amd import config, detector
    config.setup_roi_profiles(None)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.roi_profile.spectral_unmixing = {0: {1: factor}}
    try:
        with pytest.raises(NotImplementedError, match="integer factor"):
            detector.detect_blobs_blocks_device(_stub_volume(dtype), None, [(0, 0, 0)], [(8, 8, 8)])
    finally:
        config.roi_profile.spectral_unmixing = None
    # the wrap-around it refuses to imitate: NumPy stays in the integer type
    a = np.array([3, 200], dtype=dtype)
    assert np.subtract(a[:1], 1 * a[1:]).dtype == np.dtype(dtype)


# ------------------------------------------------------------------------------------- intensity co-localisation
COLOC_SHAPE = (20, 18, 30, 2)
COLOC_ORIGINS = [(2, 3, 4), (6, 1, 9)]
COLOC_EXTENTS = [(12, 14, 16), (9, 12, 14)]
#: rows of block 0 whose owned voxel counts are known numbers: interior, face x = 0, x = 1, edge, corner
COLOC_KNOWN_COUNTS = {0: 33, 1: 23, 2: 32, 3: 16, 4: 11}


def coloc_tables():
    """``(z, y, x, channel)`` int rows per block, block-relative: block 0 hand-placed, block 1 random and crowded."""
    first = [
        (6, 7, 8, 0),          # 0 interior
        (6, 7, 0, 0),          # 1 on the face x = 0
        (6, 7, 1, 1),          # 2 at x = 1, the other channel: its ball overlaps row 1's across channels
        (0, 0, 8, 0),          # 3 on the edge z = 0, y = 0
        (0, 0, 0, 1),          # 4 in the corner
        (9, 3, 12, 0),         # 5 and 6: one centre twice in one channel (the later row owns it all)
        (9, 3, 12, 0),
        (3, 11, 4, 1),         # 7 and 8: balls that overlap within a channel
        (3, 12, 5, 1),
        (4, 11, 4, 0),         # 9: overlaps 7 and 8 across channels
        (12, 7, 8, 0),         # 10 outside the block (z = nz)
        (-1, 5, 5, 1),         # 11 outside the block (z < 0)
        (11, 13, 15, 0),       # 12 in the far corner
    ]
    rng = np.random.default_rng(17)
    nz, ny, nx = COLOC_EXTENTS[1]
    second = [(int(rng.integers(0, nz)), int(rng.integers(0, ny)), int(rng.integers(0, nx)), int(rng.integers(0, 2)))
              for _ in range(28)]
    second[5] = (nz - 1, ny - 1, nx - 1, 1)
    second[9] = (4, 0, 7, 0)
    second[20] = (4, 5, nx, 1)          # outside (x = nx)
    return [np.array(first, dtype=np.int64), np.array(second, dtype=np.int64)]


def coloc_reference(roi: np.ndarray, rows: np.ndarray):
    """The reference's label volumes (row index at the centre, -1 elsewhere, grey-dilated with ball(2), one volume per
    blob channel) and, per image channel ``c`` and blob ``b``: the selection ``roi[mask == b, c]`` in the image's
    dtype, its size and ``np.mean`` of it.  -> ``(counts[n], means[c][n] float64, voxels[c][n] list of arrays)``."""
    from scipy import ndimage as ndi
    n, shape3, n_chl = len(rows), roi.shape[:3], roi.shape[3]
    inside = np.all((rows[:, :3] >= 0) & (rows[:, :3] < np.array(shape3)), axis=1)
    counts = np.zeros(n, dtype=np.int32)
    means = np.full((n_chl, n), np.nan)
    voxels = [[np.empty(0, roi.dtype)] * n for _ in range(n_chl)]
    for bc in np.unique(rows[inside, 3]):
        sel = np.flatnonzero(inside & (rows[:, 3] == bc))
        mask = -np.ones(shape3, dtype=int)
        mask[rows[sel, 0], rows[sel, 1], rows[sel, 2]] = sel        # (one centre twice: the later row wins)
        mask = ndi.grey_dilation(mask, footprint=coloc_oracle.ball(2))
        for b in sel:
            owned = mask == b
            counts[b] = np.count_nonzero(owned)
            for c in range(n_chl):
                vox = roi[owned, c]
                assert vox.dtype == roi.dtype
                voxels[c][b] = vox
                if vox.size:
                    m = np.mean(vox)
                    assert m.dtype == (np.float32 if roi.dtype == np.float32 else np.float64)
                    means[c, b] = np.float64(m)
    return counts, means, voxels


@functools.lru_cache(maxsize=None)
def coloc_case(dtype: str):
    """The image of one voxel type and the reference of both blocks, computed once."""
    img = make_image(dtype, COLOC_SHAPE, 5)
    img.setflags(write=False)
    refs = []
    for o, s, rows in zip(COLOC_ORIGINS, COLOC_EXTENTS, coloc_tables()):
        refs.append(coloc_reference(img[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]], rows))
    return img, refs


def test_coloc_known_counts_and_empty_owners():
    """The hand-placed centres own what the ball's geometry says: 33 voxels inside, 23 on a face, 32 one voxel off it,
    16 on an edge, 11 in a corner; the earlier of two identical centres and the centres outside own nothing."""
    _, refs = coloc_case("uint8")
    counts, means, _ = refs[0]
    for row, n in COLOC_KNOWN_COUNTS.items():
        assert counts[row] == n, row
    for row in (5, 10, 11):
        assert counts[row] == 0 and np.isnan(means[:, row]).all()
    # the later twin owns the whole ball; row 8 (one voxel off the face y = ny - 1) takes what it shares with row 7
    assert counts[6] == 33 and 0 < counts[7] < counts[8] == 32
    assert np.count_nonzero(refs[1][0] < 33) > 10          # the random block is crowded


def pairwise_mean_f32(vals: np.ndarray) -> np.float32:
    """NumPy's sum of n <= 33 contiguous float32 values -- one pairwise block: eight accumulators, their tree, the
    tail, behind the reduction's initial 0 -- and the float32 quotient, written out step by step: the order
    ``coloc_means_kernel<float>`` follows."""
    f = np.float32
    n = len(vals)
    with np.errstate(all="ignore"):
        if n < 8:
            res = f(0)
            for v in vals:
                res = f(res + v)
        else:
            r = [f(v) for v in vals[:8]]
            i = 8
            while i < n - n % 8:
                for j in range(8):
                    r[j] = f(r[j] + vals[i + j])
                i += 8
            res = f(f(f(r[0] + r[1]) + f(r[2] + r[3])) + f(f(r[4] + r[5]) + f(r[6] + r[7])))
            for v in vals[i:]:
                res = f(res + v)
        return f(f(f(0) + res) / f(n))


def test_float32_mean_order_is_numpys():
    """``np.mean`` of a float32 selection of every size a blob can own equals the written-out float32 order, and
    (for most sizes) not the float64 mean rounded to float32: float32 means need float32 arithmetic in that order."""
    rng = np.random.default_rng(2)
    off_f64 = 0
    for n in range(1, 34):
        for _ in range(20):
            vals = (rng.random(n) * 3 - 1).astype(np.float32)
            got = np.mean(vals)
            assert got.dtype == np.float32 and got == pairwise_mean_f32(vals), n
            off_f64 += int(got != np.float32(np.mean(vals.astype(np.float64))))
    assert off_f64 > 50


def test_float32_means_of_the_coloc_case_differ_from_float64_means():
    """The float32 case of the device test discriminates: some blob's float32 mean is not the float64 mean."""
    _, refs = coloc_case("float32")
    differ = 0
    for counts, means, voxels in refs:
        for c in range(2):
            for b in np.flatnonzero(counts):
                differ += int(means[c, b] != np.mean(voxels[c][b].astype(np.float64)))
    assert differ >= 5


# ---- the float32 tie: two means that are distinct reals and one float32
TIE_A, TIE_B = (5, 5, 12), (5, 5, 1)


def tie_roi() -> np.ndarray:
    roi = np.zeros((12, 12, 24, 2), np.float32)
    roi[..., 0] = 100
    roi[..., 1] = 62500
    roi[TIE_A][1] = 62501
    roi[TIE_B][1] = 62501
    return roi


def tie_blobs() -> np.ndarray:
    blobs = np.zeros((2, 11))
    blobs[0, :3], blobs[0, 6] = TIE_A, 0
    blobs[1, :3], blobs[1, 6] = TIE_B, 1
    blobs[:, 3] = 2
    blobs[:, 7:10] = blobs[:, :3]
    return blobs


def tie_means(dtype) -> np.ndarray:
    """``means[b, c]`` of the tie's two blobs as NumPy gives them for the ROI in ``dtype``, widened to float64."""
    roi = tie_roi().astype(dtype)
    _, means, _ = coloc_reference(roi, np.column_stack([tie_blobs()[:, :3], tie_blobs()[:, 6]]).astype(np.int64))
    return np.ascontiguousarray(means.T)


def test_float32_tie_discriminates():
    """A owns 33 voxels (mean 2062501 / 33), B 32 (mean 2000001 / 32): A's mean of channel 1 is below B's -- channel
    1's threshold -- as a real and as a float64, and equal to it as a float32.  The oracle flags A in channel 1 on the
    float32 ROI and not on its float64 copy."""
    roi, blobs = tie_roi(), tie_blobs()
    m32, m64 = tie_means(np.float32), tie_means(np.float64)
    assert m32[0, 1] == m32[1, 1] and m64[0, 1] < m64[1, 1]
    assert m32[1, 1] == np.float64(np.float32(2000001) / np.float32(32))
    np.testing.assert_array_equal(coloc_oracle.colocalize_blobs(roi, blobs), [[1, 1], [1, 1]])
    np.testing.assert_array_equal(coloc_oracle.colocalize_blobs(roi.astype(np.float64), blobs), [[1, 0], [1, 1]])


def test_float32_tie_through_the_host_flag_rules():
    """``_flags_from_means`` and ``mmx_host_coloc_flags`` compare the float32 means widened to float64, which is the
    float32 comparison: the tie is flagged from the float32 means and not from the float64 ones."""
    from magellanmapper_amd import _native as nat, colocalizer
    blobs = tie_blobs()
    shape3 = tie_roi().shape[:3]
    rows5 = np.ascontiguousarray(np.column_stack([np.zeros(2), blobs[:, :3], blobs[:, 6]]), dtype=np.int32)
    off = np.array([0, 2], dtype=np.int64)
    chans = np.array([0, 1], dtype=np.int32)
    shp = np.array([shape3], dtype=np.int32)
    for dtype, want in ((np.float32, [[1, 1], [1, 1]]), (np.float64, [[1, 0], [1, 1]])):
        means = tie_means(dtype)
        np.testing.assert_array_equal(colocalizer._flags_from_means(blobs, means, shape3, 2), want)
        by_channel = np.ascontiguousarray(means.T)           # [channel][row]
        flags = np.zeros((2, 2))
        nat.check(nat.lib().mmx_host_coloc_flags(by_channel.ctypes.data, chans.ctypes.data, 2, 2, rows5.ctypes.data,
                                                 off.ctypes.data, 1, shp.ctypes.data, 2, flags.ctypes.data, 2), "flags")
        np.testing.assert_array_equal(flags, want)


def test_float32_percentile_is_a_float32():
    """``np.percentile`` of a float32 selection interpolates in float32: the threshold the device path must use is
    the one of the values cast back to the image's dtype, not of their float64 copies."""
    vals = np.random.default_rng(0).random(200).astype(np.float32)
    differ = 0
    for q in (5, 30, 50, 99):
        got = np.percentile(vals, q)
        assert got.dtype == np.float32
        differ += int(np.float64(got) != np.percentile(vals.astype(np.float64), q))
    assert differ >= 1


def random_blobs(shape3, n: int, seed: int, n_channels: int = 2) -> np.ndarray:
    """An 11-column table of ``n`` random blobs, two of them outside the ROI."""
    rng = np.random.default_rng(seed)
    blobs = np.zeros((n, 11))
    blobs[:, :3] = np.stack([rng.integers(0, s, n) for s in shape3], axis=1)
    blobs[:, 3] = 2
    blobs[:, 6] = rng.integers(0, n_channels, n)
    blobs[3, 0] = shape3[0]
    blobs[7, 2] = -1
    blobs[:, 7:10] = blobs[:, :3]
    return blobs


def percentile_case(dtype: str):
    """A random ROI with 40 random blobs; the first blob sits in a patch of the image's largest value in both
    channels, so that even the 99th percentile of a channel's owned voxels -- that very value -- is reached by a mean
    (exactly: the mean of equal voxels)."""
    roi = make_image(dtype, (16, 20, 24, 2), 41)
    blobs = random_blobs(roi.shape[:3], 40, 42)
    z, y, x = (int(v) for v in blobs[0, :3])
    roi[max(z - 2, 0):z + 3, max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] = 255 if dtype == "uint8" else 10
    return roi, blobs


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
def test_percentile_case_flags_some_blobs_and_not_all(dtype):
    roi, blobs = percentile_case(dtype)
    for q in (5, 50, 99):
        want = oracle_flags(roi, blobs, q)
        assert 0 < want.sum() < want.size, q
    assert want[0].all()


def oracle_flags(roi, blobs, thresh=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return coloc_oracle.colocalize_blobs(roi, blobs, thresh)
