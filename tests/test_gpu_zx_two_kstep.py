"""The Z+X kernel class of kernel radius 17..24 (``zx4_kernel<2, 2, ...>``) takes its Z pass in two k-steps: a split
tile -- per lane the lower half of z tile U + 2 or the upper half of z tile U - 2 -- and z tiles U - 1, U, U + 1
(``mmx_fused4.hip``: ``cls4``).  These are the shapes at which that map can go wrong: blocks with no steady step, last
z tiles of 1, 7, 8, 9 and 16 real planes, reflections that reach into the split tile at both faces, whole turns of the
steady loop.  Needs a real MI355X (``-m gpu``).

Every comparison is against the float64 restatement (``oracle.blob_log_oracle.log_cube``) within the tolerance the
parity tests use: ``mmx_tiled_q16_error_bound`` x the value range for 16-bit tiles, 1e-6 x the value range for float32
tiles (``test_every_kernel_radius_matches_oracle``).  Voxels are uniform random over the full range of their type, so
the low bytes count.

The tiled path takes a batch whose blocks have ny >= R + 4, nz >= R + 1 and nx >= R (``mmx_fused_accepts``), so the
blocks here are R + 4 rows high -- the least it admits -- and the depth nz = R of every sweep runs in a batch of its own,
which the library sends through the separate passes: compared all the same, but not asserted to be the tiled path.
"""
import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIGMA_OF = {17: 4.25, 18: 4.5, 20: 5.0, 22: 5.5, 24: 6.0, 4: 1.0, 8: 2.0}
MAX_NZ = 128 + 15
NY_MAX, NX_MAX = 24 + 4, 40
FLOAT_RANGE = 2.0
F32_TILE_TOL = 1e-6
# (the float32 separate passes, which take the blocks of depth R: test_block_shape_and_dtype_sweep_matches_oracle)
SEPARATE_TOL = 5e-6


class _Volumes:
    """One random volume per voxel type, its device copy, and the float64 references of its blocks (each computed
    once: every block starts at the volume's origin, so (type, R, shape) names it)."""

    def __init__(self):
        from magellanmapper_amd import blob_log as bl
        rng = np.random.default_rng(1710)
        shape = (MAX_NZ, NY_MAX, NX_MAX)
        self.host = {
            "u16": rng.integers(0, 65536, shape, dtype=np.uint16),
            "u8": rng.integers(0, 256, shape, dtype=np.uint8),
            "f32": (rng.random(shape) * FLOAT_RANGE).astype(np.float32),
        }
        self.dev = {k: bl.DeviceVolume(v) for k, v in self.host.items()}
        self.refs = {}

    def ref(self, kind, R, shape):
        from oracle import blob_log_oracle as blo
        key = (kind, R, tuple(shape))
        if key not in self.refs:
            sub = self.host[kind][:shape[0], :shape[1], :shape[2]]
            img = sub.astype(np.float64) if kind == "f32" else blo.img_as_float(sub)
            self.refs[key] = blo.log_cube(img, np.array([[SIGMA_OF[R]] * 3]))[..., 0]
        return self.refs[key]


@pytest.fixture(scope="module")
def vols(gpu):
    return _Volumes()


def _space(R):
    from magellanmapper_amd import blob_log as bl
    space = bl.ScaleSpace.make(SIGMA_OF[R], SIGMA_OF[R], 1)
    assert space.radii[0] == R
    return space


def _q16_bound(space, R):
    from magellanmapper_amd import _native as nat
    return nat.lib().mmx_tiled_q16_error_bound(nat.as_double_ptr(space.w0[0]), nat.as_double_ptr(space.w2[0]), R,
                                               float(space.norms[0]))


def _sweep_depths(R, span):
    """nz = R .. R + span (every residue mod 16 at one to four z tiles) and 128 + {1, 8, 15} (whole turns of the steady
    loop)."""
    return list(range(R, R + span + 1)) + [128 + 1, 128 + 8, 128 + 15]


def _batches(R, depths):
    """At most eight distinct depths per batch (MMX_ZX4_MAXCLS), shallow and deep blocks mixed in each; nz = R alone."""
    tiled = [d for d in depths if d > R]
    n = -(-len(tiled) // 8)
    return [[R]] * (R in depths) + [tiled[i::n] for i in range(n)]


def _run(vols, kind, R, nx, depths, mode, value_range=0.0):
    """The LoG arrays of one batch of blocks (nz, R + 4, nx) under zx_mode `mode`, and the path that ran."""
    from magellanmapper_amd import blob_log as bl
    shapes = [(nz, R + 4, nx) for nz in depths]
    default, bl.ZX_MODE = bl.ZX_MODE, mode
    try:
        cubes = bl.log_cube_blocks(vols.dev[kind], 0, [(0, 0, 0)] * len(shapes), shapes, _space(R), value_range=value_range)
    finally:
        bl.ZX_MODE = default
    return shapes, [c[..., 0] for c in cubes], bl.LAST_ZX_PATH


def _check_sweep(vols, kind, R, span, modes_tol, value_range=0.0, depths=None):
    worst = {}
    for nx in (R, NX_MAX):
        for batch in _batches(R, depths or _sweep_depths(R, span)):
            for mode, tol in modes_tol:
                shapes, cubes, path = _run(vols, kind, R, nx, batch, mode, value_range)
                if min(batch) > R:
                    assert path == mode, (kind, R, nx, batch, path)
                elif mode == 6:
                    tol = SEPARATE_TOL * (value_range or 1.0)
                for shp, got in zip(shapes, cubes):
                    want = vols.ref(kind, R, shp)
                    err = float(np.abs(got - want).max())
                    worst[mode] = max(worst.get(mode, 0.0), err)
                    assert got.shape == want.shape and err < tol, (kind, R, shp, mode, err, tol)
    print("R %d %s: largest error %s" % (R, kind, {m: "%.3g of %.3g" % (worst[m], t) for m, t in modes_tol}))


@pytest.mark.parametrize("kind", ["u16", "u8"])
@pytest.mark.parametrize("R", [17, 18, 20, 22, 24])
def test_depth_sweep_16_bit_tiles(gpu, vols, R, kind):
    """Every block depth from R to R + 48 and 129, 136, 143, at two and three column tiles, uint16 and uint8 voxels."""
    from magellanmapper_amd import _native as nat
    _check_sweep(vols, kind, R, 48, [(nat.MMX_ZX_TILED_Q16, _q16_bound(_space(R), R))])


VARIANT_DEPTHS = [20, 33, 48, 49, 137]


def test_float_voxels_and_float32_tiles(gpu, vols):
    """The other instantiations of the class at R = 20: float voxels of a stated range on 16-bit and on float32 tiles,
    uint16 voxels on float32 tiles (zx_mode 6)."""
    from magellanmapper_amd import _native as nat
    R = 20
    q16 = _q16_bound(_space(R), R)
    _check_sweep(vols, "f32", R, 0, [(nat.MMX_ZX_TILED_Q16, q16 * FLOAT_RANGE), (nat.MMX_ZX_TILED, F32_TILE_TOL * FLOAT_RANGE)],
                 value_range=FLOAT_RANGE, depths=VARIANT_DEPTHS)
    _check_sweep(vols, "u16", R, 0, [(nat.MMX_ZX_TILED, F32_TILE_TOL)], depths=VARIANT_DEPTHS)


@pytest.mark.parametrize("R", [17, 18, 20, 22, 24])
def test_two_runs_are_bit_identical(gpu, vols, R, monkeypatch):
    """One batch of the sweep per R, twice: the same LoG arrays and the same candidates, values included, bit for bit
    (a register written behind the compiler's back showed as run-dependent values in this class before)."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    batch = _batches(R, _sweep_depths(R, 48))[1]
    runs = [_run(vols, "u16", R, NX_MAX, batch, nat.MMX_ZX_TILED_Q16) for _ in range(2)]
    assert runs[0][2] == runs[1][2] == nat.MMX_ZX_TILED_Q16
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    monkeypatch.setattr(bl, "ZX_MODE", nat.MMX_ZX_TILED_Q16)
    shapes = runs[0][0]
    found = []
    for _ in range(2):
        st = bl.BatchStats()
        res, peaks = bl.blob_log_blocks(vols.dev["u16"], 0, [(0, 0, 0)] * len(shapes), shapes, SIGMA_OF[R], SIGMA_OF[R], 1,
                                        0.002, 0.5, stats=st, return_peaks=True, exact_values=False)
        assert bl.LAST_ZX_PATH == nat.MMX_ZX_TILED_Q16
        found.append((res, peaks, st))
    assert found[0][2].n_candidates > 0
    assert found[0][2].n_candidates == found[1][2].n_candidates
    assert found[0][2].max_f32_error == found[1][2].max_f32_error
    for (ca, va), (cb, vb) in zip(found[0][1], found[1][1]):
        np.testing.assert_array_equal(ca, cb)
        np.testing.assert_array_equal(va.view(np.uint64), vb.view(np.uint64))
    for a, b in zip(found[0][0], found[1][0]):
        np.testing.assert_array_equal(a, b)
