"""The k-block loop of the matrix-core Y pass (``ym_kernel``, csrc/mmx_ymfma.hip) at the shapes where its structure can go
wrong: both parities of the number of k-blocks for each class of block offsets (NB = 3, 4, 5), the last block, partial
row tiles, partial z quarters and column tiles, tiles with nothing above the threshold between tiles that hold something,
with and without entries.

Two references.  The bytes: the loop was restructured without touching the arithmetic -- every accumulator takes the same
six products per k-block in the same order from the same start value -- so every LoG array and every entry must be what
the library wrote before, recorded as SHA-1 in tests/golden/y_kblock_digests.json by tests/golden/make_y_kblock_digests.py
(which also states the cases).  And one that does not rest on an earlier build: ``y6_kernel`` (``MMX_ZX_Y_VALU``) on the
same 16-bit tiles, within the 1e-5 of test_gpu_parity.py::test_y_pass_on_the_matrix_cores_agrees_with_the_valu_kernel."""
import importlib.util
import json
import os

import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_y_kblock_digests", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_y_kblock_digests.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)

_RUNS = {}


def _run(case, y_valu=False):
    """``cases.run_case``, once per module: the results are shared and left unchanged."""
    key = (case, y_valu)
    if key not in _RUNS:
        _RUNS[key] = cases.run_case(case, y_valu)
    return _RUNS[key]


def test_cases_cover_both_parities_of_the_k_block_count():
    """(the arithmetic of the shapes: no GPU work) ``ym_kernel`` runs ``(tiles + NB - 3) // 2 + 1`` k-blocks per column."""
    tiles = sorted({-(-ny // 16) for _, ny, _ in cases.SHAPES})
    assert tiles == [2, 3, 4, 5]
    assert {ny % 16 for _, ny, _ in cases.SHAPES} >= {0, 1, 13}
    for nb in (3, 4, 5):
        assert {((t + nb - 3) // 2 + 1) % 2 for t in tiles} == {0, 1}
    assert {nz % 4 for nz, _, _ in cases.SHAPES} == {1, 2} and all(nx % 16 for _, _, nx in cases.SHAPES)


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_bytes_are_those_of_the_recorded_library(gpu, case):
    with open(cases.FIXTURE) as f:
        want = json.load(f)
    assert len(want["commit"]) >= 7
    _, arrays = _run(case)
    got = cases.digests(arrays)
    assert sorted(got) == sorted(want["cases"][case])
    differ = [k for k in sorted(got) if got[k] != want["cases"][case][k]]
    assert not differ, "%s: %s differ from the library of commit %s" % (case, differ, want["commit"])


@pytest.mark.parametrize("case", sorted(cases.CASES))
def test_agrees_with_the_valu_kernel(gpu, case):
    """Where both kernels wrote a row of 64 values: within 1e-5.  A row only one of them wrote holds nothing above the
    other's threshold test, so its values are at most 1e-5 above the threshold.  Without entries every voxel is written."""
    vol, _, entries = cases.CASES[case]
    thr, eps, _ = cases.VOLUMES[vol]
    bm, am = _run(case)
    bv, av = _run(case, True)
    compared = 0
    for s in range(bm.ns):
        lm, lv = bm.cubes(am["log%d" % s]), bv.cubes(av["log%d" % s])
        if not entries:
            for i, (cm, cv) in enumerate(zip(lm, lv)):
                err = float(np.max(np.abs(cm - cv)))
                print(case, "scale", s, "block", i, "max |ym - y6| = %.3g" % err)
                assert err < 1e-5
                compared += cm.size
            continue
        om, ov = cases.rows_above(bm, am["ent%d" % s]), cases.rows_above(bv, av["ent%d" % s])
        for i, (nz, ny, nx) in enumerate(bm.shapes):
            vox = [np.moveaxis(np.repeat(np.repeat(o[i], 4, axis=1), 16, axis=2)[:, :nz, :nx], 0, 1) for o in (om, ov)]
            cm, cv = lm[i][:, :, :nx], lv[i][:, :, :nx]
            both, one = vox[0] & vox[1], vox[0] ^ vox[1]
            if both.any():
                err = float(np.max(np.abs(cm[both] - cv[both])))
                print(case, "scale", s, "block", i, "rows written by both: %d voxels, max |ym - y6| = %.3g; by one: %d"
                      % (both.sum(), err, one.sum()))
                assert err < 1e-5
                compared += int(both.sum())
            if one.any():
                assert float(np.max(np.maximum(cm[one], cv[one]))) <= thr - eps + 1e-5
            assert not cm[~vox[0]].any() and not cv[~vox[1]].any()       # (the zeroed workspace shows through)
    assert compared > 1000


@pytest.mark.parametrize("lad", sorted(cases.LADDERS))
def test_sparse_volume_has_quiet_tiles_between_tiles_with_rows(gpu, lad):
    """From the entries: in some column, a whole tile of 16 rows x 64 columns without a row above the threshold lies
    between two tiles that have one (the pending row before it is closed without a successor, the row after it starts
    without a predecessor) -- and the synthetic volume has tiles of both kinds too."""
    for vol in ("sparse", "synth"):
        b, arrays = _run("%s_%s" % (vol, lad))
        for s in range(b.ns):
            between = quiet = loud = 0
            for on, (nz, ny, nx) in zip(cases.rows_above(b, arrays["ent%d" % s]), b.shapes):
                nt = -(-ny // 16)
                tile_on = np.stack([on[16 * t:16 * t + 16].any(axis=0) for t in range(nt)])      # [tile][z quad][column tile]
                full = [t for t in range(nt) if 16 * t + 16 <= ny]
                quiet += int(sum((~tile_on[t]).sum() for t in full))
                loud += int(sum(tile_on[t].sum() for t in full))
                for t in full:
                    if 0 < t < nt - 1:
                        between += int((tile_on[t - 1] & ~tile_on[t] & tile_on[t + 1]).sum())
            print(vol, lad, "scale", s, "full tiles quiet %d, with rows %d, quiet between two with rows %d" % (quiet, loud, between))
            assert quiet > 0 and loud > 0
            if vol == "sparse":
                assert between > 0
