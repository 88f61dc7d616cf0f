"""GPU tests of the kernel-path rules (``csrc/mmx_route.h``): what ``mmx_log_scales_f32`` / ``mmx_detect_batch`` report for
a ladder, which kernel families they launch and that the re-scored candidates are those nominated from the full cube of
the same kernels by name; and single ``mmx_log_batch_f32`` calls by name against the rows of
``tests/golden/route_by_name.txt``, which ``tools/route_check.cpp`` holds the pure routing function to.  One block per
test, by ``ladder_run`` of gpu_support.py.  Needs a real MI355X (``-m gpu``)."""
import ctypes
import os

import numpy as np
import pytest

from gpu_support import gpu, ladder_run  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_by_name.txt")
FAMILIES = ("zpass", "ypass", "xpass", "generic", "zxpass", "y2pass", "zxpack", "widepass")


@pytest.fixture(scope="module")
def volume():
    """One uint16 volume with blobs of the ladders' sizes; the blocks are cut from it at an odd x origin."""
    from magellanmapper_amd import synth
    return synth.make_volume(19, (48, 40, 80), 30, blob_sigma=2.5)


def _voxels(vol16, kind):
    return vol16 if kind == "u16" else (vol16 / 65535.0).astype(np.float32)


def _families(kinds):
    from magellanmapper_amd.rawbatch import families
    return families(kinds, FAMILIES)


def _check_ladder(vol, origin, shape, sigmas, value_range, want_radii, want_info, by_name, want_families):
    """The report, the candidates against the by-name reference, and the launches of one extra, timed run (the ladder
    runs twice in it: ``mmx_log_scales_f32``, then ``mmx_detect_batch``)."""
    from magellanmapper_amd.rawbatch import timed
    info, cands, space = ladder_run(vol, origin, shape, *sigmas, value_range=value_range)
    assert [int(r) for r in space.radii] == want_radii
    zx_path, layout, rounds, bounded = want_info
    print("info: path %d layout %d rounds %d q16_bound %g" % (info.zx_path, info.mask_layout, info.n_pass_rounds, info.q16_bound))
    assert (info.zx_path, info.mask_layout, info.n_pass_rounds) == (zx_path, layout, rounds)
    # (the bound of the worst scale in value units -- the range is 1 here -- or 0 when the last scale ran no 16-bit tiles)
    assert info.q16_bound == (space.q16_bound() if bounded else 0.0)
    _, dense, _ = ladder_run(vol, origin, shape, *sigmas, value_range=value_range, by_name=by_name)
    assert len(dense) > 0 and len(cands) == len(dense)
    for f in ("slot", "s", "z", "y", "x", "v", "v64"):
        np.testing.assert_array_equal(cands[f], dense[f], err_msg=f)
    _, kinds = timed(lambda: ladder_run(vol, origin, shape, *sigmas, value_range=value_range))
    print("families:", _families(kinds))
    assert _families(kinds) == {k: 2 * n for k, n in want_families.items()}


# ---------------------------------------------------------------- A. a ladder whose scales disagree
def test_a_mixed_ladder_launches_its_final_configuration_only(gpu, volume):
    """Radii 6 and 18 on a uint16 block of 40 x 20 x 40: radius 18 needs 22 rows for the fused path and has 20, so it
    takes the separate passes (Z and X on the register-ring kernels, Y generic) and writes no entries, radius 6 takes the
    16-bit tiles and would write quads -- the rules settle on no entries, the second configuration they go through.
    The report and the candidates are the parent's; only that configuration is launched (the parent launched both: 4 of
    each family below instead of 2)."""
    from magellanmapper_amd import _native as nat
    _check_ladder(volume, (3, 7, 5), (40, 20, 40), (1.5, 4.5, 2), 0.0, [6, 18],
                  (nat.MMX_ZX_SEPARATE, 0, 2, False), [nat.MMX_ZX_TILED_Q16, nat.MMX_ZX_SEPARATE],
                  dict(zxpack=1, zxpass=1, y2pass=1, zpass=1, generic=1, xpass=1))


# ---------------------------------------------------------------- B. ladders whose scales agree at once
@pytest.mark.parametrize("kind,value_range,path,layout,bounded,families", [
    ("u16", 0.0, "MMX_ZX_TILED_Q16", "MMX_MASK_QUADS", True, dict(zxpack=1, zxpass=3, y2pass=3)),
    ("f32", 0.0, "MMX_ZX_PACKED", "MMX_MASK_ROWS", False, dict(zxpass=3, y2pass=3)),
    # (blob_log's band for voxels in [0, 1] covers the 16-bit tiles' error fourfold: ranged float voxels take them too)
    ("f32", 1.0, "MMX_ZX_TILED_Q16", "MMX_MASK_QUADS", True, dict(zxpack=1, zxpass=3, y2pass=3)),
], ids=["u16", "f32-no-range", "f32-ranged"])
def test_a_ladder_of_one_path_is_one_round(gpu, volume, kind, value_range, path, layout, bounded, families):
    """Radii 4, 8, 12 (one per Z+X geometry class up to 16) on a block of 48 x 40 x 64: one round, one voxel copy for the
    tiled ladders, the candidates of the by-name reference."""
    from magellanmapper_amd import _native as nat
    _check_ladder(_voxels(volume, kind), (0, 0, 5), (48, 40, 64), (1.0, 3.0, 3), value_range, [4, 8, 12],
                  (getattr(nat, path), getattr(nat, layout), 1, bounded), [getattr(nat, path)] * 3, families)


# ---------------------------------------------------------------- C. single calls by name
def _golden_rows():
    rows = []
    with open(GOLDEN) as f:
        for line in f:
            if line.startswith("#") or not line.strip():
                continue
            ins, outs = line.split("|")
            dtype, vrange, mode, y_valu, prepacked, entries, band = ins.split()
            rows.append((int(dtype), float(vrange), int(mode), int(y_valu), int(prepacked), int(entries), float(band),
                         tuple(int(v) for v in outs.split())))
    return rows


def test_calls_by_name_run_the_route_the_table_states(gpu, volume):
    """Every mode of ``mmx_zx_mode`` with and without its flags and entries (``tests/golden/route_by_name.txt``): the
    reported path, the reported entry layout and the kernel families that ran are the route of that row."""
    from magellanmapper_amd import _native as nat
    from magellanmapper_amd.rawbatch import RawBatch, timed
    rows = _golden_rows()
    assert len(rows) >= 30 and {r[2] for r in rows} == {-1, 0, 2, 6, 7, 8}
    origin, shape, R = (0, 0, 5), (48, 40, 64), 8
    held = {}
    for dtype, vrange, mode, y_valu, prepacked, entries, band, want in rows:
        kind = {nat.MMX_U16: "u16", nat.MMX_F32: "f32"}[dtype]
        if kind not in held:
            held[kind] = RawBatch(_voxels(volume, kind), [origin], [shape], (2.0, 2.0, 1), 0.05, 0.0, 0)
            assert held[kind].space.radii[0] == R
        b = held[kind]
        b.ws = torch.empty_like(b.ws)           # (a workspace of its own per row)
        assert b.v32.dtype == dtype
        b.v32.value_range = vrange
        if prepacked:
            nat.check(b.L.mmx_zx_pack(ctypes.byref(b.v32), b.d_blocks.data_ptr(), b.blocks.ctypes.data, 1, b.slot,
                                      b.ws.data_ptr(), b.stream), "mmx_zx_pack")
        zx_mode = mode | (nat.MMX_ZX_Y_VALU if y_valu else 0) | (nat.MMX_ZX_PREPACKED if prepacked else 0)
        ran, kinds = timed(lambda: b.log_batch(0, zx_mode, 0.05 - band, band, entries=bool(entries)))
        path, written = ran if entries else (ran, 0)
        family, q16, copy, y, rings, layout, zx_path = want
        if family == 0:
            ring = [bool(rings & 1), bool(rings & 2), bool(rings & 4)]
            fams = dict(zpass=int(ring[0]), ypass=int(ring[1]), xpass=int(ring[2]), generic=3 - sum(ring))
        elif family == 1:
            fams = dict(widepass=3)
        else:
            fams = dict(zxpack=copy, zxpass=1, y2pass=1)
        got = (path, written, _families(kinds))
        row = (kind, vrange, mode, y_valu, prepacked, entries, band)
        print(row, "->", got)
        assert got == (zx_path, layout, {k: n for k, n in fams.items() if n}), row
