"""The inputs of tests/test_gpu_wide_rows.py, checked on the CPU: every block those tests run is wider than one panel of
the tiled path's voxel copy (512 columns), and the oracle alone must find peaks on both sides of every panel seam the
block has -- otherwise a copy that garbles a seam could go unnoticed.  The volumes are ``synth.make_volume`` from fixed
seeds plus blobs stamped at named columns around the seams and at the end of the row (the last, partial group of a row
and the zero fill past it)."""
import numpy as np
import pytest

PANEL = 512                             # columns of one panel of the copy (csrc/mmx_fused4.hip: zx6_pack_kernel)
SEAM_REACH = 8                          # "near a seam": within this many voxels of it
SEAM_OFFSETS = (-7, -5, -3, -1, 0, 0, 2, 4, 7)          # columns, relative to a seam, of the blobs stamped around it
#: the two-scale ladder of the peak tests (kernel radii 6 and 10: inside every block, whatever its thickness)
SIGMAS = (1.5, 2.5, 2)
THRESHOLD, OVERLAP = 0.05, 0.5

#: name -> (seed, volume shape, [(origin, block shape), ...]): each entry of the list is one batch of one block, except
#: "mixed", whose two blocks are one batch (two width classes, odd origins: the uint16 copy's unaligned branch)
CASES = {
    "513": (101, (20, 24, 530), [((0, 0, 0), (20, 24, 513))]),
    # (26 planes: the depth from which a 513 voxels wide block fits the slot ``blob_log`` gives it -- the odd number of
    #  column tiles on the tiled path through ``blob_log_blocks`` too)
    "513x26": (102, (26, 30, 1040), [((0, 0, 0), (26, 30, 513))]),
    "530": (101, (20, 24, 530), [((0, 0, 0), (20, 24, 530))]),
    "1024": (102, (26, 30, 1040), [((0, 0, 0), (26, 30, 1024))]),
    "1025": (102, (26, 30, 1040), [((0, 0, 0), (26, 30, 1025))]),
    "1040": (102, (26, 30, 1040), [((0, 0, 0), (26, 30, 1040))]),
    "2049": (103, (26, 30, 2049), [((0, 0, 0), (26, 30, 2049))]),
    "mixed": (104, (27, 33, 541), [((1, 3, 11), (26, 30, 530)), ((1, 1, 5), (26, 30, 200))]),
}
#: the stack of the end-to-end test: 1 um / px, ``segment_size`` 560 -> two blocks along x, 565 and 540 voxels wide, the
#: second from x = 560; sigma factors 3 .. 4 in 2 scales, the default profile's threshold and overlap
STACK_SHAPE, STACK_SEGMENT = (40, 60, 1100), 560
STACK_BLOCKS = [((0, 0, 0), (40, 60, 565)), ((0, 0, 560), (40, 60, 540))]
STACK_SIGMAS, STACK_THRESHOLD = (3.0, 4.0, 2), 0.1
_VOLUMES = {}
_PEAKS = {}


def seams(nx):
    """Columns at which a row of ``nx`` voxels passes from one panel of the copy to the next."""
    return list(range(PANEL, nx, PANEL))


def _stamp(vol, centre, amp, width, reach=6):
    """A Gaussian blob of integer voxels, cut off ``reach`` voxels from its centre -- the larger of it and what is
    there."""
    lo = [max(0, c - reach) for c in centre]
    hi = [min(n, c + reach + 1) for c, n in zip(centre, vol.shape)]
    zz, yy, xx = np.meshgrid(*(np.arange(a, b) for a, b in zip(lo, hi)), indexing="ij")
    d2 = (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2
    blob = np.where(d2 <= reach * reach, amp * np.exp(-d2 / (2.0 * width * width)), 0).astype(np.uint16)
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    vol[sl] = np.maximum(vol[sl], blob)


def volume(name):
    """The uint16 volume of a case (once per seed and shape): background blobs, then around every seam a lattice of
    stamped blobs at the columns seam - 7 .. seam + 7, and three at the end of the row."""
    from magellanmapper_amd import synth
    seed, shape, blocks = CASES[name]
    key = (seed, shape)
    if key in _VOLUMES:
        return _VOLUMES[key]
    vol = synth.make_volume(seed, shape, max(6, shape[2] // 60), blob_sigma=2.0)
    nz, ny, nx = shape
    spots = [(z, y) for z in (4, nz // 2, nz - 5) for y in (4, ny // 2, ny - 5)]
    x0 = max(o[2] for o, _ in blocks)                    # (the seams of a block at an x origin lie at origin + 512 k)
    for i, s in enumerate(seams(nx - x0)):
        for j, ((z, y), dx) in enumerate(zip(spots, SEAM_OFFSETS)):
            _stamp(vol, (z, y, x0 + s + dx), 21000 + 1900 * j + 700 * i, 1.6 + 0.1 * (j % 3))
    for j, dx in enumerate((-1, -3, -6)):
        _stamp(vol, (*spots[4 * j], nx - 1 + dx), 26000 + 1300 * j, 1.7)
    _VOLUMES[key] = vol
    return vol


def stack_volume():
    """The uint16 stack of the end-to-end test (once): background blobs, and around the panel seam of either block
    (local x = 512: columns 512 and 560 + 512 of the stack) a lattice of nine stamped blobs of the ladder's size."""
    from magellanmapper_amd import synth
    if "stack" not in _VOLUMES:
        vol = synth.make_volume(31, STACK_SHAPE, 24)
        spots = [(z, y) for z in (8, 20, 31) for y in (10, 30, 49)]
        for i, (origin, shape) in enumerate(STACK_BLOCKS):
            for s in seams(shape[2]):
                for j, ((z, y), dx) in enumerate(zip(spots, SEAM_OFFSETS)):
                    _stamp(vol, (z, y, origin[2] + s + dx), 30000 + 1500 * j + 600 * i, 3.0 + 0.1 * (j % 3), reach=9)
        _VOLUMES["stack"] = vol
    return _VOLUMES["stack"]


def block_image(name, i=0):
    """Block ``i`` of a case as an image of its own (what the oracle sees: reflect boundaries at the block's faces)."""
    o, s = CASES[name][2][i]
    return volume(name)[o[0]:o[0] + s[0], o[1]:o[1] + s[1], o[2]:o[2] + s[2]]


def oracle_peaks(name, i=0):
    """``oracle.blob_log_oracle.blob_log`` of a block on the two-scale ladder (once): the pruned rows, the ordered raw
    peaks ``(z, y, x, scale)`` and their float64 values."""
    from oracle import blob_log_oracle as blo
    if (name, i) not in _PEAKS:
        res, st = blo.blob_log(block_image(name, i), *SIGMAS, THRESHOLD, OVERLAP, return_stages=True)
        _PEAKS[(name, i)] = (res, st["peaks"].reshape(-1, 4), st["peak_values"].astype(np.float64))
    return _PEAKS[(name, i)]


def _check_seams(what, peaks, nx):
    """At least 6 peaks within 8 voxels of every seam of a row of ``nx`` voxels (columns s - 8 .. s + 7), at least 2 on
    either side (x < s, x >= s)."""
    assert nx > PANEL and seams(nx), "no seam"
    for s in seams(nx):
        near = np.abs(peaks[:, 2] - s + 0.5) < SEAM_REACH
        left, right = near & (peaks[:, 2] < s), near & (peaks[:, 2] >= s)
        print("%s: seam %d: %d peaks on the left, %d on the right" % (what, s, left.sum(), right.sum()))
        assert near.sum() >= 6 and left.sum() >= 2 and right.sum() >= 2, (what, s, left.sum(), right.sum())


@pytest.mark.parametrize("i", range(len(STACK_BLOCKS)))
def test_the_oracle_finds_peaks_on_both_sides_of_the_seam_of_either_stack_block(i):
    """The same for the two blocks of the stack test, each as the image the detection sees (raw voxels, the stack's own
    ladder, threshold and overlap); and the block layout is the one ``segment_size`` 560 gives."""
    from magellanmapper_amd import config
    from oracle import blob_log_oracle as blo, magmap_oracle as mmo
    config.setup_roi_profiles(None)
    prof = dict(config.roi_profile, segment_size=STACK_SEGMENT)
    layout = mmo.setup_blocks(prof, STACK_SHAPE, np.array([[1.0, 1.0, 1.0]]))
    slices = [tuple((a.start, a.stop) for a in sl) for sl in np.asarray(layout["sub_roi_slices"]).ravel()]
    assert slices == [tuple((o, o + n) for o, n in zip(*b)) for b in STACK_BLOCKS]
    assert (prof["detection_threshold"], prof["overlap"]) == (STACK_THRESHOLD, OVERLAP)
    o, shp = STACK_BLOCKS[i]
    img = stack_volume()[o[0]:o[0] + shp[0], o[1]:o[1] + shp[1], o[2]:o[2] + shp[2]]
    _, st = blo.blob_log(img, *STACK_SIGMAS, STACK_THRESHOLD, OVERLAP, return_stages=True)
    _check_seams("stack block %d" % i, st["peaks"].reshape(-1, 4), shp[2])


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_oracle_finds_peaks_on_both_sides_of_every_seam(name):
    """At least 6 oracle peaks within 8 voxels of each panel seam of the case's widest block, at least 2 of them on
    either side (x < seam, x >= seam); and the ladder's radii are the ones the GPU tests count on."""
    from magellanmapper_amd import blob_log as bl
    assert [int(r) for r in bl.ScaleSpace.make(*SIGMAS).radii] == [6, 10]
    _, shape, blocks = CASES[name]
    nx = blocks[0][1][2]
    _, peaks, values = oracle_peaks(name, 0)
    assert len(peaks) == len(values) and len(peaks) > 0
    _check_seams(name, peaks, nx)
    # ... and something at the end of the row, where the last partial group and the zero fill are
    assert (peaks[:, 2] >= nx - 8).sum() >= 1
