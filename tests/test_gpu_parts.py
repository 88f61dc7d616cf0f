"""GPU tests of blocks detected in parts: ``mmx_fold_parts`` on its own, and whole detections with
``blob_log.MAX_SLOT_ELEMS`` lowered so that small blocks are cut -- against the CPU oracle, against the same call with the
default limit, and against the stored tables of the real scikit-image / MagellanMapper.  Exactness is the contract: every
comparison is ``assert_array_equal``.  Needs a real MI355X (``-m gpu``); the conditions on the inputs are CPU tests."""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from gpu_support import gpu  # noqa: F401

torch = pytest.importorskip("torch")


# ---------------------------------------------------------------- 1. mmx_fold_parts alone
def _fold_case(n, seed):
    """Three parts of two parents and ``n`` candidates over them: voxels on the first and the last layer of a core, one
    layer outside it, anywhere in the box, and a few entries whose slot is no part.  Returns the parts, the table and
    the table the fold must leave (in any order)."""
    from magellanmapper_amd import _native as nat
    parts = np.zeros(3, dtype=nat.PART_DTYPE)
    box = np.array([[30, 40, 50], [30, 33, 50], [21, 25, 64]])
    parts["parent"] = [0, 0, 1]
    parts["off"] = [[0, 0, 0], [0, 27, 0], [9, 100, 7]]
    parts["core_lo"] = [[0, 0, 0], [0, 8, 0], [4, 5, 6]]
    parts["core_hi"] = [[30, 35, 50], [30, 33, 50], [17, 20, 58]]
    rng = np.random.default_rng(seed)
    c = np.zeros(n, dtype=nat.CAND_DTYPE)
    c["slot"] = rng.integers(0, 3, n)
    c["s"] = rng.integers(0, 5, n)
    zyx = np.stack([rng.integers(0, box[c["slot"], ax]) for ax in range(3)], axis=1)
    lo, hi = parts["core_lo"][c["slot"]], parts["core_hi"][c["slot"]]
    kind = np.arange(n) % 8          # 0, 1: first / last core layer; 2, 3: one layer outside; else anywhere
    ax = rng.integers(0, 3, n)
    rows = np.arange(n)
    inside = np.clip(zyx, lo, hi - 1)
    for k, val in ((0, lo), (1, hi - 1), (2, lo - 1), (3, hi)):
        sel = kind == k
        zyx[sel] = inside[sel]
        zyx[rows[sel], ax[sel]] = val[rows[sel], ax[sel]]
    c["z"], c["y"], c["x"] = zyx[:, 0], zyx[:, 1], zyx[:, 2]
    c["slot"][5::41] = [-1, 3, 7, -100][:len(c["slot"][5::41])] if n < 200 else np.resize([-1, 3, 7, -100], len(c["slot"][5::41]))
    c["flags"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    c["v"] = rng.random(n).astype(np.float32)
    c["nbr_max"] = rng.random(n).astype(np.float32)
    c["v64"] = rng.random(n)
    c["band"] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    ok = (c["slot"] >= 0) & (c["slot"] < 3)
    slot = np.where(ok, c["slot"], 0)
    zyx = np.stack([c["z"], c["y"], c["x"]], axis=1)
    keep = ok & ((zyx >= parts["core_lo"][slot]) & (zyx < parts["core_hi"][slot])).all(axis=1)
    want = c[keep].copy()
    moved = zyx[keep] + parts["off"][slot[keep]]
    want["slot"] = parts["parent"][slot[keep]]
    want["z"], want["y"], want["x"] = moved[:, 0], moved[:, 1], moved[:, 2]
    return parts, c, want, kind, keep


def _canon(table):
    """The entries of a candidate table as rows of bytes, sorted: the fold keeps no order."""
    rows = np.ascontiguousarray(table).view(np.uint8).reshape(len(table), -1)
    return rows[np.lexsort(rows.T[::-1])]


def test_fold_case_covers_the_core_faces():
    """(CPU) the hand-made table holds kept voxels on first and last core layers and dropped ones just outside."""
    parts, c, want, kind, keep = _fold_case(203, 1)
    ok = (c["slot"] >= 0) & (c["slot"] < 3)
    assert keep[(kind == 0) & ok].all() and keep[(kind == 1) & ok].all()
    # (one layer outside the core: dropped -- where the box has such a layer at all, the voxel exists)
    assert not keep[(kind == 2) & ok].any() and not keep[(kind == 3) & ok].any()
    assert (~ok).sum() >= 3 and 60 < keep.sum() < 190
    assert set(want["slot"]) == {0, 1} and len(want) == keep.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [203, 9001], ids=["203", "9001-three-chunks"])
def test_fold_parts_alone(gpu, n):
    """``mmx_fold_parts`` through ctypes: the kept set, the remapped fields, every other field untouched, the count; then
    the same table with ``*d_count > cap``: table and count are left alone."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    L = nat.lib()
    parts, c, want, _, _ = _fold_case(n, n)
    stream = torch.cuda.current_stream().cuda_stream
    d_parts = torch.from_numpy(parts.view(np.uint8).reshape(-1).copy()).to(gpu)
    cap = n + 7
    pad = np.zeros(cap - n, dtype=nat.CAND_DTYPE)
    pad["slot"] = 1
    pad["z"], pad["y"], pad["x"] = 3, 10, 3              # (inside a core: must NOT be taken -- they lie beyond the count)
    full = np.concatenate([c, pad])
    d_tab = torch.from_numpy(full.view(np.uint8).reshape(-1).copy()).to(gpu)
    d_count = torch.tensor([n, 12345], dtype=torch.int32, device=gpu)
    nat.check(L.mmx_fold_parts(d_tab.data_ptr(), cap, d_count.data_ptr(), d_parts.data_ptr(), 3, stream), "mmx_fold_parts")
    torch.cuda.synchronize()
    count = d_count.cpu().numpy()
    got = d_tab.cpu().numpy().view(nat.CAND_DTYPE)
    assert count[0] == len(want) and count[1] == 12345
    np.testing.assert_array_equal(_canon(got[:len(want)]), _canon(want))
    np.testing.assert_array_equal(_canon(got[n:]), _canon(pad))
    # an overflowed table: the count stays above the capacity, nothing is touched
    small = n - 50
    d_tab = torch.from_numpy(c[:small].view(np.uint8).reshape(-1).copy()).to(gpu)
    d_count = torch.tensor([n, 7], dtype=torch.int32, device=gpu)
    nat.check(L.mmx_fold_parts(d_tab.data_ptr(), small, d_count.data_ptr(), d_parts.data_ptr(), 3, stream), "mmx_fold_parts")
    torch.cuda.synchronize()
    assert d_count.cpu().numpy().tolist() == [n, 7]
    np.testing.assert_array_equal(d_tab.cpu().numpy(), c[:small].view(np.uint8).reshape(-1))
    # bad arguments are refused before any launch
    assert L.mmx_fold_parts(None, cap, d_count.data_ptr(), d_parts.data_ptr(), 3, stream) == 1
    assert L.mmx_fold_parts(d_tab.data_ptr(), small, d_count.data_ptr(), d_parts.data_ptr(), 0, stream) == 1


# ---------------------------------------------------------------- 2. one block, cut 2 x 2 x 2 and 1 x 1 x 3
BLOCK = (40, 48, 52)
#: (limit, min_sigma, max_sigma): five scales of radius <= 8 whose halo (largest radius + 1) makes the fewest-parts grid
#: of the 40 x 48 x 52 block the one named -- rows are padded to 32 elements, so a cut across x only pays when a part's
#: row drops to 32: with halo 6 the halves of 52 do (2 x 2 x 2), with halo 7 only the thirds do (1 x 1 x 3)
CUT_CASES = {"2x2x2": (30000, 0.9, 1.3, (2, 2, 2)), "1x1x3": (70000, 1.0, 1.5, (1, 1, 3))}
THRESHOLD, OVERLAP = 0.02, 0.5


def _stamp(vol, centre, amp, width):
    """A Gaussian blob of integer voxels, cut off four voxels from its centre (so that what lies further away does not
    see it) -- the larger of it and what is there."""
    lo = [max(0, c - 4) for c in centre]
    hi = [min(n, c + 5) for c, n in zip(centre, vol.shape)]
    zz, yy, xx = np.meshgrid(*(np.arange(a, b) for a, b in zip(lo, hi)), indexing="ij")
    d2 = (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2
    blob = np.where(d2 <= 16, amp * np.exp(-d2 / (2.0 * width * width)), 0).astype(np.uint16)
    sl = tuple(slice(a, b) for a, b in zip(lo, hi))
    vol[sl] = np.maximum(vol[sl], blob)


_CUT = {}


def _cut_case(name):
    """The block of one cut case, built from the splitter's own cut planes, and its oracle result (once)."""
    if name in _CUT:
        return _CUT[name]
    from magellanmapper_amd import blob_log as bl, kernels1d as k1
    from oracle import blob_log_oracle as blo
    limit, s_lo, s_hi, grid = CUT_CASES[name]
    sigmas, _ = k1.sigma_ladder(s_lo, s_hi, 5)
    radii = [k1.kernel_radius(s) for s in sigmas]
    assert len(radii) == 5 and max(radii) <= 8
    sp = bl.split_oversized(BLOCK, limit, max(radii) + 1)
    assert sp.grid == grid
    planes = [(ax, int(c)) for ax in range(3) for c in sp.cuts[ax][1:-1]]
    vol = np.full(BLOCK, 200, dtype=np.uint16)
    placed = []

    def spot(centre, need):
        """``centre`` with its None coordinates taken from a lattice, the first choice that keeps ``need`` voxels
        (largest coordinate difference) from every blob placed so far."""
        lattice = [[6, 18, 30] if n < 44 else [6, 18, 30, 42] for n in BLOCK]
        free = [ax for ax in range(3) if centre[ax] is None]
        for pick in np.ndindex(*(len(lattice[ax]) for ax in free)):
            cen = list(centre)
            for ax, j in zip(free, pick):
                cen[ax] = lattice[ax][j]
            if all(max(abs(u - v) for u, v in zip(cen, other)) >= need for other in placed):
                placed.append(tuple(cen))
                return placed[-1]
        raise AssertionError("no room left for a blob at %r" % (centre,))

    # two equal blobs mirrored across the last x cut, nothing else within reach of either (a stamp's 4 voxels + the
    # largest radius): their peaks tie exactly
    cx = int(sp.cuts[2][-2])
    tie = spot((None, None, cx - 3), 0)
    placed.append((tie[0], tie[1], cx + 2))
    # a real corner at either end, and where the cut planes of all cut axes meet (an edge of eight parts for 2 x 2 x 2)
    spot((0, 0, 0), 12)
    spot(tuple(n - 1 for n in BLOCK), 12)
    if min(sp.grid) > 1:
        spot(tuple(int(sp.cuts[ax][1]) for ax in range(3)), 12)
    # on every cut plane, and one voxel either side of it
    for ax, c in planes:
        for off in ((-1, 0, 1) if len(planes) > 2 else (-1, 0, 1, -1, 0)):
            cen = [None, None, None]
            cen[ax] = c + off
            spot(tuple(cen), 12)
    for i, cen in enumerate(placed):
        tied = i < 2
        _stamp(vol, cen, 30000 if tied else 20000 + 1700 * i, 1.2 if tied else 1.0 + 0.1 * (i % 4))
    res, st = blo.blob_log(vol, s_lo, s_hi, 5, THRESHOLD, OVERLAP, return_stages=True)
    _CUT[name] = dict(vol=vol, split=sp, planes=planes, res=res, peaks=st["peaks"].reshape(-1, 4),
                      values=st["peak_values"].astype(np.float64), limit=limit, sigmas=(s_lo, s_hi))
    return _CUT[name]


@pytest.mark.parametrize("name", sorted(CUT_CASES))
def test_cut_case_proves_something(name):
    """(CPU) the condition on the input: at least 6 oracle peaks lie within one voxel of a cut plane, some in each half
    of it, and two peaks tie exactly across a cut."""
    case = _cut_case(name)
    peaks, values = case["peaks"], case["values"]
    near = np.zeros(len(peaks), dtype=bool)
    sides = set()
    for ax, c in case["planes"]:
        for side, v in ((0, c - 1), (1, c)):            # the two voxel layers that touch the plane
            hit = peaks[:, ax] == v
            near |= hit
            if hit.any():
                sides.add((ax, c, side))
    assert near.sum() >= 6, (near.sum(), peaks)
    assert len(sides) >= len(case["planes"]) + 1, sides
    uniq, counts = np.unique(values, return_counts=True)
    tied = uniq[counts > 1]
    assert len(tied) >= 1
    a, b = peaks[values == tied[-1]][:2]
    cuts = [c for ax, c in case["planes"] if a[ax] < c <= b[ax] or b[ax] < c <= a[ax]]
    assert cuts, (a, b)                                 # the tied peaks lie on either side of a cut
    assert len(case["res"]) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CUT_CASES))
def test_one_block_in_parts_equals_the_oracle_and_the_whole_block(gpu, monkeypatch, name):
    from magellanmapper_amd import blob_log as bl
    case = _cut_case(name)
    vol, (s_lo, s_hi) = case["vol"], case["sigmas"]
    dvol = bl.DeviceVolume(vol)
    seen = []
    real = bl._enqueue_detect
    monkeypatch.setattr(bl, "_enqueue_detect", lambda *a, **k: seen.append(k.get("split")) or real(*a, **k))
    whole_stats = bl.BatchStats()
    whole, whole_peaks = bl.blob_log_blocks(dvol, 0, [(0, 0, 0)], [BLOCK], s_lo, s_hi, 5, THRESHOLD, OVERLAP,
                                            stats=whole_stats, return_peaks=True)
    assert seen == [None] and whole_stats.n_part_voxels == whole_stats.n_voxels == vol.size
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", case["limit"], raising=True)
    stats = bl.BatchStats()
    got, peaks = bl.blob_log_blocks(dvol, 0, [(0, 0, 0)], [BLOCK], s_lo, s_hi, 5, THRESHOLD, OVERLAP, stats=stats,
                                    return_peaks=True)
    assert len(seen) == 2 and seen[1] is not None and seen[1].grid == CUT_CASES[name][3]
    assert stats.n_blocks == 1 and stats.n_voxels == vol.size
    assert stats.n_part_voxels == int(case["split"].box_shapes.prod(axis=1).sum()) > vol.size
    # the oracle, run on the CPU
    np.testing.assert_array_equal(peaks[0][0], case["peaks"])
    np.testing.assert_array_equal(peaks[0][1], case["values"])
    np.testing.assert_array_equal(got[0], case["res"])
    # the same call with the default limit, row for row, raw peaks included
    np.testing.assert_array_equal(peaks[0][0], whole_peaks[0][0])
    np.testing.assert_array_equal(peaks[0][1], whole_peaks[0][1])
    np.testing.assert_array_equal(got[0], whole[0])
    assert stats.n_peaks == whole_stats.n_peaks == len(case["peaks"])


@pytest.mark.gpu
def test_overflowed_table_of_a_block_in_parts_is_nominated_again(gpu, monkeypatch):
    """The fold leaves an overflowed table alone and its count above the capacity: the caller's retry fires, with all
    the parts again."""
    from magellanmapper_amd import blob_log as bl
    case = _cut_case("2x2x2")
    s_lo, s_hi = case["sigmas"]
    real = bl._enqueue_detect
    calls = []

    def tiny_first(*args, **kwargs):
        if not calls:
            kwargs["cap"] = 8
        calls.append((kwargs.get("cap"), kwargs.get("split")))
        return real(*args, **kwargs)

    monkeypatch.setattr(bl, "_enqueue_detect", tiny_first)
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", case["limit"], raising=True)
    got = bl.blob_log_blocks(bl.DeviceVolume(case["vol"]), 0, [(0, 0, 0)], [BLOCK], s_lo, s_hi, 5, THRESHOLD, OVERLAP)
    assert len(calls) >= 2 and calls[0][0] == 8 and calls[-1][0] > 8 and all(c[1] is not None for c in calls)
    np.testing.assert_array_equal(got[0], case["res"])


# ---------------------------------------------------------------- 3. wide radii
WIDE_SHAPE, WIDE_R = (70, 72, 80), 30
_WIDE = {}


def _wide_case():
    from magellanmapper_amd import synth
    from oracle import blob_log_oracle as blo
    if not _WIDE:
        vol = synth.make_volume(29, WIDE_SHAPE, 9, blob_sigma=7.0)
        sigma = (WIDE_R + 0.2) / 4.0
        _WIDE.update(vol=vol, sigma=sigma, res=blo.blob_log(vol, sigma, sigma, 1, 0.02, 0.5))
    return _WIDE


@pytest.mark.gpu
def test_wide_radius_block_in_parts(gpu, monkeypatch):
    """One scale of radius 30 through the wide passes by name, the block cut 1 x 2 x 2 (a grid the search never picks
    here -- the halves of a row of 80 are as wide as the row once padded -- so it is forced)."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    case = _wide_case()
    assert len(case["res"]) >= 3
    monkeypatch.setattr(bl, "ZX_MODE", nat.MMX_ZX_WIDE)
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", 460000, raising=True)
    monkeypatch.setattr(bl, "FORCED_PART_GRID", (1, 2, 2), raising=True)
    seen = []
    real = bl._enqueue_detect
    monkeypatch.setattr(bl, "_enqueue_detect", lambda *a, **k: seen.append(k.get("split")) or real(*a, **k))
    stats = bl.BatchStats()
    got = bl.blob_log_blocks(bl.DeviceVolume(case["vol"]), 0, [(0, 0, 0)], [WIDE_SHAPE], case["sigma"], case["sigma"], 1,
                             0.02, 0.5, stats=stats)
    assert len(seen) == 1 and seen[0].grid == (1, 2, 2) and seen[0].halo == WIDE_R + 1
    assert bl.LAST_ZX_PATH == nat.MMX_ZX_WIDE
    assert stats.n_part_voxels > stats.n_voxels == int(np.prod(WIDE_SHAPE))
    np.testing.assert_array_equal(got[0], case["res"])


# ---------------------------------------------------------------- 4. the real scikit-image's tables
GOLDEN_BLOBLOG = sorted(os.path.basename(p)[len("bloblog_"):-4] for p in
                        glob.glob(os.path.join(GOLDEN, "bloblog_u16_*.npz"))) + ["u8_3sigma"]
#: its ladder's halo of 21 voxels covers the whole 20 x 24 x 28 block from any core: such a block cannot be cut
UNSPLITTABLE = {"u16_empty"}


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLDEN_BLOBLOG)
def test_golden_blob_log_in_parts(gpu, monkeypatch, case):
    """Every uint16 fixture and the uint8 one with the limit at the fixture's own slot size: cut, and identical to what
    the real scikit-image stored.  The one fixture no grid can cut is refused with the reason."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    g = load_golden("bloblog_%s.npz" % case)
    shape = g["volume"].shape
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", int(bl._slot_elems(shape)), raising=True)
    args = (float(g["min_sigma"]), float(g["max_sigma"]), int(g["num_sigma"]), float(g["threshold"]), float(g["overlap"]))
    dvol = bl.DeviceVolume(g["volume"])
    if case in UNSPLITTABLE:
        with pytest.raises(nat.MmxError, match="cannot be cut into parts"):
            bl.blob_log_blocks(dvol, 0, [(0, 0, 0)], [shape], *args)
        return
    stats = bl.BatchStats()
    res, peaks = bl.blob_log_blocks(dvol, 0, [(0, 0, 0)], [shape], *args, stats=stats, return_peaks=True)
    assert stats.n_part_voxels > stats.n_voxels
    np.testing.assert_array_equal(peaks[0][0], g["peaks"].reshape(-1, 4))
    assert res[0].shape == g["pruned"].shape
    np.testing.assert_array_equal(res[0], g["pruned"])


# ---------------------------------------------------------------- 5., 6. stacks: stock preprocessing, raw voxels
@pytest.fixture
def golden_preproc_env(monkeypatch):
    """The environment the preprocessing fixtures were made in (as in test_gpu_parity.py)."""
    from magellanmapper_amd import config, preprocess
    w = load_golden("preproc.npz")["gauss8_weights"]
    monkeypatch.setattr(preprocess, "RGB_GUESS", True)
    monkeypatch.setattr(preprocess, "GAUSS_WEIGHTS_OVERRIDE", np.ascontiguousarray(w[32:]))
    yield
    config.near_max = [-1.0]


def _setup_stack(g):
    from magellanmapper_amd import config, stack_detect
    config.setup_roi_profiles(None)
    config.roi_profile["denoise_size"] = None
    config.roi_profile.update(ast.literal_eval(str(g["overrides"])))
    config.near_max = list(g["near_max"]) if "near_max" in g else [-1.0]
    config.resolutions = g["resolutions"]
    config.filename = "golden"
    return stack_detect.setup_blocks(config.roi_profile, g["roi"].shape)


#: 45 x 45 x 45 blocks (slot 129 600) and a ladder of radius 20: under this limit they are cut 2 x 2 x 1, along two axes
STACK_LIMIT = 125000


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["denoise", "u16_2x3x3"])
def test_golden_stack_with_blocks_in_parts(gpu, case, tmp_path, monkeypatch, golden_preproc_env):
    """``detect_blobs_blocks`` of a stored stack -- with the profile's preprocessing on, and on raw voxels -- with every
    full-size block cut along two axes: per-block, merged and final tables identical to the stored ones."""
    from magellanmapper_amd import blob_log as bl, chunking, config, stack_detect
    monkeypatch.chdir(tmp_path)
    g = load_golden("stack_%s.npz" % case)
    blocks = _setup_stack(g)
    roi = g["roi"]
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", STACK_LIMIT, raising=True)
    seen = []
    real = bl._enqueue_detect
    monkeypatch.setattr(bl, "_enqueue_detect", lambda *a, **k: seen.append(k.get("split")) or real(*a, **k))
    seg = stack_detect.StackDetector.detect_blobs_sub_rois(
        None, roi, blocks.sub_roi_slices, blocks.sub_rois_offsets, blocks.denoise_max_shape, blocks.exclude_border,
        False, [0])
    cut = [sp for sp in seen if sp is not None]
    assert cut and all(sorted(sp.grid) == [1, 2, 2] for sp in cut) and len(cut) < len(seen)
    assert (blocks.denoise_max_shape is not None) == (case == "denoise")
    assert seg.shape == tuple(g["grid"])
    for c in np.ndindex(*seg.shape):
        want = g["block_%d_%d_%d" % c]
        if want.shape[0] == 0:
            assert seg[c] is None
        else:
            np.testing.assert_array_equal(seg[c], want)
    np.testing.assert_array_equal(chunking.merge_blobs(seg), g["merged"])
    del seen[:]
    _, _, blobs = stack_detect.detect_blobs_blocks("golden", stack_detect.Image5d(roi[None]), None, None, None, False,
                                                   False, True, False)
    assert any(sp is not None for sp in seen)
    st = stack_detect.StackDetector.last_stats
    assert st.n_part_voxels > st.n_voxels
    np.testing.assert_array_equal(blobs.blobs, g["final"])
    assert list(blobs.cols) == list(g["final_cols"])


@pytest.mark.gpu
def test_dense_stack_blocks_cannot_be_cut(gpu, tmp_path, monkeypatch, golden_preproc_env):
    """``stack_denoise_dense.npz``: blocks of 41 voxels a side and a ladder of radius 20 -- a halo of 21 voxels reaches
    across the block from any core, so no grid of parts is smaller than the block.  With the limit at the block's own slot
    the detection raises the library's error with that reason; with the default limit the stack gives its stored table."""
    from magellanmapper_amd import _native as nat, blob_log as bl, stack_detect
    monkeypatch.chdir(tmp_path)
    g = load_golden("stack_denoise_dense.npz")
    _setup_stack(g)
    img = stack_detect.Image5d(g["roi"][None])
    _, _, blobs = stack_detect.detect_blobs_blocks("golden", img, None, None, None, False, False, True, False)
    np.testing.assert_array_equal(blobs.blobs, g["final"])
    assert stack_detect.StackDetector.last_stats.n_part_voxels == stack_detect.StackDetector.last_stats.n_voxels
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", int(bl._slot_elems((41, 41, 41))), raising=True)
    with pytest.raises(nat.MmxError, match="halo of 21 voxels.*segment_size"):
        stack_detect.detect_blobs_blocks("golden", img, None, None, None, False, False, True, False)


# ---------------------------------------------------------------- 7. what a block in parts does not take
@pytest.mark.gpu
def test_coloc_and_isotropic_on_a_block_in_parts_raise(gpu, tmp_path, monkeypatch):
    from magellanmapper_amd import blob_log as bl, config, stack_detect
    monkeypatch.chdir(tmp_path)
    g = load_golden("stack_coloc_2ch.npz")
    roi = g["roi"]
    _setup_stack(g)
    img = stack_detect.Image5d(roi[None])
    monkeypatch.setattr(bl, "MAX_SLOT_ELEMS", 1000, raising=True)
    with pytest.raises(NotImplementedError, match="coloc=True"):
        stack_detect.detect_blobs_blocks("golden", img, None, None, None, False, False, True, True)
    config.roi_profile["isotropic"] = (1.0, 1.0, 1.0)
    try:
        with pytest.raises(NotImplementedError, match="isotropic rescale"):
            stack_detect.detect_blobs_blocks("golden", img, None, None, None, False, False, True, False)
    finally:
        config.roi_profile["isotropic"] = None
    config.roi_profile.spectral_unmixing = {1: {0: 0.5}}
    try:
        with pytest.raises(NotImplementedError, match="spectral unmixing"):
            stack_detect.detect_blobs_blocks("golden", img, None, None, None, False, False, True, False)
    finally:
        config.roi_profile.spectral_unmixing = None


@pytest.mark.gpu
def test_no_batch_reports_parts_under_the_default_limit(gpu, tmp_path, monkeypatch):
    from magellanmapper_amd import blob_log as bl, stack_detect
    monkeypatch.chdir(tmp_path)
    g = load_golden("stack_u16_2x3x3.npz")
    _setup_stack(g)
    seen = []
    real = bl._enqueue_detect
    monkeypatch.setattr(bl, "_enqueue_detect", lambda *a, **k: seen.append(k.get("split")) or real(*a, **k))
    _, _, blobs = stack_detect.detect_blobs_blocks("golden", stack_detect.Image5d(g["roi"][None]), None, None, None,
                                                   False, False, True, False)
    assert seen and all(sp is None for sp in seen)
    st = stack_detect.StackDetector.last_stats
    assert st.n_part_voxels == st.n_voxels > 0
    np.testing.assert_array_equal(blobs.blobs, g["final"])
