"""The steps of the Z+X kernel's march outside its steady loop (``mmx_fused4.hip``): the X-only head steps, the edge
output tiles at both faces of a block, the drain.  For 16-bit tiles of integer voxels at kernel radius 9..24 they run
in a form of their own -- the edge tiles' Z fragments in LDS, the steady step's memory instructions in every step, head
stores dropped through the buffer range -- unless a depth of the batch has more edge tiles than the LDS holds, or
``MMX_ZX_EDGE_GLOBAL`` asks for the form that reads the global table.  Needs a real MI355X (``-m gpu``).

As in ``test_gpu_zx_two_kstep.py``: voxels uniform random over the full range of their type, every comparison against
the float64 restatement (``oracle.blob_log_oracle.log_cube``) within ``mmx_tiled_q16_error_bound`` x the value range,
blocks R + 4 rows high and 40 columns wide (three column tiles: a pair and an odd tile).  uint16 and uint8 voxels run
the same kernels (the copy widens uint8): the pair kernel at radius 9..16, the split-tile kernel at 17..24; float voxels
run the one-tile kernels, which keep the global-table form.
"""
import ctypes

import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIGMA_OF = {9: 2.25, 12: 3.0, 16: 4.0, 17: 4.25, 20: 5.0, 24: 6.0}
MAX_NZ = 192
NX = 40
NY_MAX = 24 + 4
FLOAT_RANGE = 2.0
PATTERN = 0x5A5AC3C3


# ---------------------------------------------------------------------------------------------- the march's geometry
def _march(nz, R):
    """(steady steps, edge output tiles, z tiles) of a block nz deep, as zx4_kernel lays its march out: a ring of two z
    tiles in flight, one output tile LA steps behind, steady steps in whole rings (radius <= 16) or turns of four."""
    LA = 1 if R <= 16 else 2
    group = 2 if LA == 1 else 4
    ntz = (nz + 15) // 16
    u_lo, u_hi = (R + 15) // 16, (nz - 16 - R) // 16           # (floor division: u_hi may be negative)
    tA = -(-(u_lo + LA) // 2) * 2
    nB = min(u_hi + LA + 1, ntz) - tA
    nB = nB // group * group if nB > 0 else 0
    hi0 = max(u_hi + 1, u_lo)
    return nB, u_lo + max(ntz - hi0, 0), ntz


def _fits(nz, R):
    """The block's edge tables fit the kernel's LDS (``zx4_edges_fit``): three tiles at radius <= 16, four above."""
    return _march(nz, R)[1] <= (3 if R <= 16 else 4)


def _depths(R):
    """nz = R + 1; the largest depth with no steady step; the least depths with exactly one ring or turn of steady
    steps and with two; last z tiles of 1, 5, 15 and 16 real planes."""
    group = 2 if R <= 16 else 4
    steady = {nz: _march(nz, R)[0] for nz in range(R + 1, MAX_NZ + 1)}
    out = [R + 1, max(nz for nz, n in steady.items() if n == 0)]
    out += [min(nz for nz, n in steady.items() if n == k * group) for k in (1, 2)]
    out += [64 + 1, 64 + 5, 64 + 15, 64 + 16]
    return sorted(set(out))


def test_depths_cover_the_march():
    """(no GPU work) the sweep's depths are what the docstring of _depths says, for every radius tested."""
    for R in SIGMA_OF:
        d = _depths(R)
        group = 2 if R <= 16 else 4
        assert R + 1 in d and {_march(nz, R)[0] for nz in d} >= {0, group, 2 * group}
        assert {(nz - 1) % 16 + 1 for nz in d} >= {1, 5, 15, 16}
        assert max(d) <= MAX_NZ
        if R <= 16:
            assert all(_fits(nz, R) for nz in d)
    # radius 18 .. 24: a third high edge tile where nz mod 16 is in [1, R - 16); no interior tile among five z tiles
    assert not _fits(65, 20) and not _fits(81, 24) and not _fits(66, 24) and _fits(69, 20) and _fits(261, 20)


# ------------------------------------------------------------------------------------------------------- the runs
class _Volumes:
    def __init__(self):
        from magellanmapper_amd import blob_log as bl
        rng = np.random.default_rng(1404)
        shape = (MAX_NZ, NY_MAX, NX)
        self.host = {
            "u16": rng.integers(0, 65536, shape, dtype=np.uint16),
            "u8": rng.integers(0, 256, shape, dtype=np.uint8),
            "f32": (rng.random(shape) * FLOAT_RANGE).astype(np.float32),
        }
        self.dev = {k: bl.DeviceVolume(v) for k, v in self.host.items()}
        self.refs = {}
        self.runs = {}

    def ref(self, kind, R, shape):
        from oracle import blob_log_oracle as blo
        key = (kind, R, tuple(shape))
        if key not in self.refs:
            sub = self.host[kind][:shape[0], :shape[1], :shape[2]]
            img = sub.astype(np.float64) if kind == "f32" else blo.img_as_float(sub)
            self.refs[key] = blo.log_cube(img, np.array([[SIGMA_OF[R]] * 3]))[..., 0]
        return self.refs[key]

    def run(self, kind, R, depths, flags, fresh=False):
        key = (kind, R, tuple(depths), flags)
        if fresh or key not in self.runs:
            out = _run(self, kind, R, depths, flags)
            if fresh:
                return out
            self.runs[key] = out
        return self.runs[key]


@pytest.fixture(scope="module")
def vols(gpu):
    return _Volumes()


def _space(R):
    from magellanmapper_amd import blob_log as bl
    space = bl.ScaleSpace.make(SIGMA_OF[R], SIGMA_OF[R], 1)
    assert space.radii[0] == R
    return space


def _tol(kind, R):
    from magellanmapper_amd import _native as nat
    space = _space(R)
    bound = nat.lib().mmx_tiled_q16_error_bound(nat.as_double_ptr(space.w0[0]), nat.as_double_ptr(space.w2[0]), R,
                                                float(space.norms[0]))
    return bound * (FLOAT_RANGE if kind == "f32" else 1.0)


def _run(vols, kind, R, depths, flags):
    """One batch of blocks (nz, R + 4, NX) through ``mmx_log_batch_f32`` on 16-bit tiles, over a workspace pre-filled with
    PATTERN: ``(LoG arrays, tile dwords of the real voxels per block, the tile half of the workspace, tile stride)``."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    L = nat.lib()
    dvol = vols.dev[kind]
    dvol.wait_all()
    dev = dvol.tensor.device
    space = _space(R)
    shapes = [(nz, R + 4, NX) for nz in depths]
    blocks, slot = bl._make_blocks(dvol, 0, [(0, 0, 0)] * len(shapes), shapes)
    nb = len(blocks)
    ws = torch.full((5 * nb * slot,), PATTERN, dtype=torch.int32, device=dev)
    d_blocks = bl._to_device_bytes(blocks, dev)
    v32 = dvol.view(0, True)
    if kind == "f32":
        v32.value_range = FLOAT_RANGE
    path = ctypes.c_int(0)
    log_base = ws.data_ptr() + 4 * nb * slot * 4
    nat.check(L.mmx_log_batch_f32(ctypes.byref(v32), d_blocks.data_ptr(), blocks.ctypes.data, nb, slot,
                                  nat.as_double_ptr(space.w0[0]), nat.as_double_ptr(space.w2[0]), R, float(space.norms[0]),
                                  log_base, ws.data_ptr(), None, 0.0, 0.0, None, nat.MMX_ZX_TILED_Q16 | flags,
                                  ctypes.byref(path), torch.cuda.current_stream().cuda_stream), "mmx_log_batch_f32")
    torch.cuda.synchronize()
    assert path.value == nat.MMX_ZX_TILED_Q16, (kind, R, depths, path.value)
    host = ws.cpu().numpy().view(np.uint32)
    logs = host[4 * nb * slot:].view(np.float32).reshape(nb, slot)
    ntx = (NX + 15) // 16
    stride = max(ntx * ((nz + 15) // 16) * ny * 256 for nz, ny, _ in shapes)       # (mmx_zx6_plan_make: tile_stride)
    cubes, tiles = [], []
    for i, (nz, ny, nx) in enumerate(shapes):
        px = int(blocks["px"][i])
        cubes.append(logs[i, :nz * ny * px].reshape(nz, ny, px)[..., :nx].copy())
        ntz = (nz + 15) // 16
        # tile (y, c, U) at ((y ntx + c) ntz + U) x 256 dwords, 16 planes x 16 columns row-major
        t = host[i * stride:i * stride + ny * ntx * ntz * 256].reshape(ny, ntx, ntz, 16, 16)
        tiles.append(t.transpose(2, 3, 0, 1, 4).reshape(ntz * 16, ny, ntx * 16)[:nz, :, :nx].copy())
    return cubes, tiles, host[:2 * nb * stride].copy(), stride


def _batches(R, depths):
    """The depths whose edge tables fit in one batch (a batch takes the LDS form only when all of its depths fit), the
    others in a second."""
    fit = [d for d in depths if _fits(d, R)]
    rest = [d for d in depths if not _fits(d, R)]
    return [b for b in (fit, rest) if b]


CASES = [(R, k) for R in (9, 12, 16) for k in ("u16", "u8", "f32")] + [(R, "u16") for R in (17, 20, 24)] + [(20, "u8")]


@pytest.mark.parametrize("R,kind", CASES)
def test_depth_sweep_matches_oracle(gpu, vols, R, kind):
    """Every depth of _depths(R), both edge forms, against the float64 oracle."""
    from magellanmapper_amd import _native as nat
    tol = _tol(kind, R)
    worst = 0.0
    for batch in _batches(R, _depths(R)):
        for flags in (0, nat.MMX_ZX_EDGE_GLOBAL):
            cubes = vols.run(kind, R, batch, flags)[0]
            for nz, got in zip(batch, cubes):
                want = vols.ref(kind, R, (nz, R + 4, NX))
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                assert got.shape == want.shape and err < tol, (kind, R, nz, flags, err, tol)
    print("R %d %s depths %s: largest error %.3g of %.3g" % (R, kind, _depths(R), worst, tol))


@pytest.mark.parametrize("R,kind", CASES)
def test_edge_forms_are_bit_identical(gpu, vols, R, kind):
    """Every stored tile dword of a real voxel is the same from the LDS form and from the global-table form, and from two
    runs of the same form; so is every LoG value."""
    from magellanmapper_amd import _native as nat
    for batch in _batches(R, _depths(R)):
        lds = vols.run(kind, R, batch, 0)
        glob = vols.run(kind, R, batch, nat.MMX_ZX_EDGE_GLOBAL)
        again = vols.run(kind, R, batch, 0, fresh=True)
        for nz, a, b, c in zip(batch, lds[1], glob[1], again[1]):
            assert not (a == PATTERN).all(), (kind, R, nz)
            np.testing.assert_array_equal(a, b, err_msg="LDS form against global-table form, nz %d" % nz)
            np.testing.assert_array_equal(a, c, err_msg="two runs of the LDS form, nz %d" % nz)
        for a, b, c in zip(lds[0], glob[0], again[0]):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
            np.testing.assert_array_equal(a.view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("R,depths", [(12, (13, 69, 133)), (20, (21, 69, 133)), (24, (40, 66, 104))])
def test_mixed_depths_in_one_batch(gpu, vols, R, depths):
    """Three depths in one batch (three depth classes, three sets of edge tables): every block right against its own
    oracle cube and bit-identical to the same block run alone.  (24: 66 planes do not fit -- the batch takes the
    global-table form, the blocks alone the form each admits.)"""
    tol = _tol("u16", R)
    cubes, tiles, _, _ = vols.run("u16", R, depths, 0)
    for nz, got, t in zip(depths, cubes, tiles):
        want = vols.ref("u16", R, (nz, R + 4, NX))
        err = float(np.abs(got - want).max())
        assert err < tol, (R, nz, err, tol)
        alone = vols.run("u16", R, (nz,), 0)
        np.testing.assert_array_equal(got.view(np.uint32), alone[0][0].view(np.uint32))
        np.testing.assert_array_equal(t, alone[1][0])


@pytest.mark.parametrize("R,nz", [(20, 65), (20, 81), (24, 66), (24, 71)])
def test_depths_beyond_the_lds_budget_fall_back(gpu, vols, R, nz):
    """Depths with five edge output tiles -- a third high one, or no interior tile among five -- exceed the four tables
    the split-tile kernel keeps: such a batch runs the global-table form and is right against the oracle."""
    assert not _fits(nz, R) and _march(nz, R)[1] == 5
    tol = _tol("u16", R)
    got = vols.run("u16", R, (nz,), 0)[0][0]
    err = float(np.abs(got - vols.ref("u16", R, (nz, R + 4, NX))).max())
    assert err < tol, (R, nz, err, tol)


@pytest.mark.parametrize("R", [12, 20])
def test_nothing_outside_the_tile_columns_changes(gpu, vols, R):
    """Over a workspace pre-filled with a pattern, the Z+X kernel writes the planes 0 .. nz - 1 of every tile column of
    its blocks and nothing else in the tile half of the workspace: not the rows past the block in the last z tile, not
    the rest of a shallower block's stride, not the next block, not the unused Q half -- the stores the head steps drop
    and the tail's last tiles included."""
    from magellanmapper_amd import _native as nat
    depths = [d for d in _depths(R) if _fits(d, R)]
    ntx = (NX + 15) // 16
    for flags in (0, nat.MMX_ZX_EDGE_GLOBAL):
        _, _, half, stride = vols.run("u16", R, depths, flags)
        untouched = np.ones(half.shape, dtype=bool)
        for i, nz in enumerate(depths):
            ny, ntz = R + 4, (nz + 15) // 16
            own = untouched[i * stride:i * stride + ny * ntx * ntz * 256].reshape(ny * ntx, ntz * 16, 16)
            own[:, :nz, :] = False
        bad = np.flatnonzero(untouched & (half != PATTERN))
        assert bad.size == 0, (R, flags, bad[:8], stride)
        # ... and what it does write is written: no real plane of a tile column keeps the pattern throughout
        for i, nz in enumerate(depths):
            ny, ntz = R + 4, (nz + 15) // 16
            own = half[i * stride:i * stride + ny * ntx * ntz * 256].reshape(ny * ntx, ntz * 16, 16)[:, :nz, :]
            assert not (own == PATTERN).all(axis=2).any(), (R, flags, nz)
