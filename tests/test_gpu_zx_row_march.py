"""The row march of the Z+X kernel (``mmx_fused4.hip``): a wave of the pair kernel (16-bit tiles of integer voxels, radius
9..16, LDS edge form) keeps its column pair and marches through several rows of its block in one go -- one table fill,
one set of X fragments, one X-only head and one clamped tail per run of rows.  ``MMX_ZX_ROWS(n)`` forces n rows per wave
in every block; 0 leaves the choice to the launch (``zx4_rows_rule``).  Needs a real MI355X (``-m gpu``).

The cases, their shapes and the driver are stated in ``tests/golden/make_zx_row_march_digests.py`` (which also says why
the row counts start at R + 4 and not at 1), together with the digests recorded from the parent commit's library.
Voxels are uniform random over the full range of their type; the float64 restatement is
``oracle.blob_log_oracle.log_cube``, the tolerance ``mmx_tiled_q16_error_bound``.  The split-tile kernel (radius 17..24)
and the depths that do not fit the LDS keep the one-row march under every value of the field.
"""
import json
import os
import sys

import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_zx_row_march_digests as zr  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


class _Runs(zr.Volumes):
    """Each (voxel type, radius, blocks, rows per wave) runs once.  The arrays are kept for 0 (the launch's own choice)
    and 1 row per wave; every other form is compared with the one-row arrays as it comes in and leaves a record: the two
    digests, the first difference from the one-row form, what was written outside the tile columns, what was not written
    inside them."""

    def __init__(self):
        super().__init__()
        self.refs, self.recs = {}, {}
        with open(zr.FIXTURE) as f:
            self.golden = json.load(f)["cases"]

    def ref(self, kind, R, shape):
        from oracle import blob_log_oracle as blo
        key = (kind, R, tuple(shape))
        if key not in self.refs:
            sub = self.host[kind][:shape[0], :shape[1], :shape[2]]
            self.refs[key] = blo.log_cube(blo.img_as_float(sub), np.array([[zr.SIGMA_OF[R]] * 3]))[..., 0]
        return self.refs[key]

    def _record(self, kind, R, shp, n):
        from magellanmapper_amd import _native as nat
        cubes, tiles, half, stride = zr.run(self, kind, R, shp, nat.MMX_ZX_ROWS(n))
        rec = dict(tiles_sha=zr.digest(tiles), log_sha=zr.digest(cubes), differs=None)
        untouched = np.ones(half.shape, dtype=bool)
        unwritten = []
        for i, (nz, ny, nx) in enumerate(shp):
            ntx, ntz = -(-nx // 16), -(-nz // 16)
            lo, hi = i * stride, i * stride + ny * ntx * ntz * 256
            untouched[lo:hi].reshape(ny * ntx, ntz * 16, 16)[:, :nz, :] = False
            # ... and what it does write is written: no real plane of a tile column keeps the pattern throughout
            if (half[lo:hi].reshape(ny * ntx, ntz * 16, 16)[:, :nz, :] == zr.PATTERN).all(axis=2).any():
                unwritten.append((nz, ny, nx))
        rec["outside"] = np.flatnonzero(untouched & (half != zr.PATTERN))[:8].tolist()
        rec["unwritten"] = unwritten
        if n in (0, 1):
            rec["cubes"], rec["tiles"] = cubes, tiles
        if n != 1:
            one = self.rec(kind, R, shp, 1)
            for s, a, b, ca, cb in zip(shp, one["tiles"], tiles, one["cubes"], cubes):
                if not np.array_equal(a, b) or not np.array_equal(ca.view(np.uint32), cb.view(np.uint32)):
                    z, y, x = (np.argwhere(a != b)[0] if not np.array_equal(a, b) else np.argwhere(ca != cb)[0])
                    rec["differs"] = "block %s at (z %d, y %d, x %d)" % (s, z, y, x)
                    break
        return rec

    def rec(self, kind, R, shp, n, fresh=False):
        key = (kind, R, tuple(shp), n)
        if fresh:
            return self._record(kind, R, shp, n)
        if key not in self.recs:
            self.recs[key] = self._record(kind, R, shp, n)
        return self.recs[key]


@pytest.fixture(scope="module")
def runs(gpu):
    return _Runs()


def _forced(R):
    return zr.FORCED + ((15,) if R == 9 else ())


def _tol(R):
    from magellanmapper_amd import _native as nat
    sp = zr.space(R)
    return nat.lib().mmx_tiled_q16_error_bound(nat.as_double_ptr(sp.w0[0]), nat.as_double_ptr(sp.w2[0]), R, float(sp.norms[0]))


def test_cases_cover_the_march():
    """(no GPU work) the shapes are what the fixture's docstring says, for every radius tested."""
    for R in zr.SIGMA_OF:
        group = 2 if R <= 16 else 4
        d = zr.depths(R)
        assert R + 1 in d and {zr.march(nz, R)[0] for nz in d} >= {0, group}
        assert {zr.march(nz, R)[2] & 1 for nz in d} == {0, 1}
        assert {(nz - 1) % 16 + 1 for nz in d} >= {1, 5, 16} and max(d) <= zr.MAX_NZ
        if R <= 16:
            assert all(zr.fits(nz, R) for nz in d) and len(zr.batches(R)) == 1
        ny = zr.rows(R)
        assert min(ny) == R + 4 and max(ny) <= zr.NY_MAX
        for n in (2, 4, 8):             # whole runs, one row more, a short last run of more than one row
            assert {y % n for y in ny} >= {0, 1}, (R, n)
        assert any(y % 3 == 0 for y in ny) and any(y % 3 == 1 for y in ny)
        assert all(nx >= R for nx in zr.widths(R))
        for b in zr.batches(R):
            s = zr.shapes(R, b)
            assert {ny_ for _, ny_, _ in s} == set(ny) and {nx for _, _, nx in s} == set(zr.widths(R))
    assert not zr.fits(65, 20) and [65] in zr.batches(20)
    assert min(zr.rows(9)) < 15


@pytest.mark.parametrize("R,kind", zr.CASES)
def test_forms_are_bit_identical(gpu, runs, R, kind):
    """Every stored tile dword of a real voxel and every LoG value is the same with 1 row per wave and with 2, 3, 4 and 8
    (radius 9: 15, more than a block has), under the launch's own choice, and from two runs of one form."""
    for batch in zr.batches(R):
        shp = zr.shapes(R, batch)
        one = runs.rec(kind, R, shp, 1)
        assert all(not (t == zr.PATTERN).all() for t in one["tiles"])
        for n in (0,) + _forced(R)[1:]:
            got = runs.rec(kind, R, shp, n)
            assert got["differs"] is None, "%d rows per wave against 1: %s" % (n, got["differs"])
            assert (got["tiles_sha"], got["log_sha"]) == (one["tiles_sha"], one["log_sha"]), n
        n = _forced(R)[-1]
        again = runs.rec(kind, R, shp, n, fresh=True)
        assert again["differs"] is None and again["tiles_sha"] == one["tiles_sha"], "two runs with %d rows per wave" % n


@pytest.mark.parametrize("R,kind", zr.CASES)
def test_matches_oracle(gpu, runs, R, kind):
    """Every value agrees with the float64 restatement within the stated bound of the 16-bit tiles: under the launch's own
    choice and with one row per wave by value, with the most rows per wave through its digest."""
    tol = _tol(R)
    worst = 0.0
    for batch in zr.batches(R):
        shp = zr.shapes(R, batch)
        for n in (0, 1):
            for s, got in zip(shp, runs.rec(kind, R, shp, n)["cubes"]):
                want = runs.ref(kind, R, s)
                err = float(np.abs(got - want).max())
                worst = max(worst, err)
                assert got.shape == want.shape and err < tol, (kind, R, s, n, err, tol)
        assert runs.rec(kind, R, shp, _forced(R)[-1])["log_sha"] == runs.rec(kind, R, shp, 1)["log_sha"]
    print("R %d %s: largest error %.3g of %.3g" % (R, kind, worst, tol))


@pytest.mark.parametrize("R,kind", zr.CASES)
def test_reproduces_the_parent(gpu, runs, R, kind):
    """The digests recorded from the parent commit's library, in the automatic mode and in every forced one."""
    for i, batch in enumerate(zr.batches(R)):
        want = runs.golden[zr.case_name(R, kind, i)]
        shp = zr.shapes(R, batch)
        for n in (0,) + _forced(R):
            got = runs.rec(kind, R, shp, n)
            assert got["tiles_sha"] == want["tiles"], (R, kind, i, n)
            assert got["log_sha"] == want["log"], (R, kind, i, n)


@pytest.mark.parametrize("R", [12, 20])
def test_nothing_outside_the_tile_columns_changes(gpu, runs, R):
    """Over a workspace pre-filled with a pattern, the kernel writes the planes 0 .. nz - 1 of every tile column of its
    blocks and nothing else in the tile half of the workspace -- not the rows past the block in a row's last z tile, which
    a wave now passes on its way to the next row, not the next block, not the unused Q half."""
    for batch in zr.batches(R):
        shp = zr.shapes(R, batch)
        for n in (0,) + _forced(R):
            got = runs.rec("u16", R, shp, n)
            assert got["outside"] == [], (R, n, got["outside"])
            assert got["unwritten"] == [], (R, n, got["unwritten"])


def test_mixed_batch_under_the_automatic_rule(gpu, runs):
    """720 small blocks -- two depth classes, two widths, three row counts -- are enough wave-rows for the rule to taper:
    the first blocks get two rows per wave, the last ones one.  The result is the one-row
    march's and the parent's, bit for bit, and right against the oracle."""
    import ctypes
    from magellanmapper_amd import _native as nat
    R, shp = zr.TAPER_R, zr.TAPER_SHAPES
    f = ctypes.CDLL(nat.LIB_PATH).mmx_zx_rows_schedule
    i32p = ctypes.POINTER(ctypes.c_int32)
    f.argtypes = [ctypes.c_int, i32p, i32p, ctypes.c_int, ctypes.c_int, i32p, i32p]
    rows = np.array([ny for _, ny, _ in shp], dtype=np.int32)
    wpr = np.array([(-(-nx // 16) + 1) // 2 for _, _, nx in shp], dtype=np.int32)
    nr = np.zeros(len(shp), dtype=np.int32)
    # (slots -1: the library asks the runtime for the resident waves of the row kernel on this device, as the launch does)
    assert f(len(shp), rows.ctypes.data_as(i32p), wpr.ctypes.data_as(i32p), -1, 0, nr.ctypes.data_as(i32p), None) > 0
    values, first = np.unique(nr, return_index=True)
    print("rows per wave -> first block:", dict(zip(values.tolist(), first.tolist())), "of", len(shp), "blocks")
    assert set(values.tolist()) == {1, 2} and nr[0] == 2 and nr[-1] == 1 and (np.diff(nr) <= 0).all()
    auto = runs.rec("u16", R, shp, 0)
    assert auto["differs"] is None, auto["differs"]
    assert auto["outside"] == [] and auto["unwritten"] == []
    want = runs.golden["taper"]
    assert (auto["tiles_sha"], auto["log_sha"]) == (want["tiles"], want["log"])
    tol = _tol(R)
    for s, got in list(zip(shp, auto["cubes"]))[:3] + list(zip(shp, auto["cubes"]))[-3:]:
        assert float(np.abs(got - runs.ref("u16", R, s)).max()) < tol, s
