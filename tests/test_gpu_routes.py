"""GPU tests of the kernel-path rules (``csrc/mmx_route.h``): what ``mmx_log_scales_f32`` / ``mmx_detect_batch`` report for
a ladder, which kernel families they launch and that the re-scored candidates are those nominated from the full cube of
the same kernels by name; and single ``mmx_log_batch_f32`` calls by name against the rows of
``tests/golden/route_by_name.txt``, which ``tools/route_check.cpp`` holds the pure routing function to.  One block per
test, in the idiom of ``_ladder_run`` of test_gpu_wide_radius.py.  Needs a real MI355X (``-m gpu``)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "route_by_name.txt")
FAMILIES = ("zpass", "ypass", "xpass", "generic", "zxpass", "y2pass", "zxpack", "widepass")


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from magellanmapper_amd import _native
    assert os.path.exists(_native.LIB_PATH), "libmmx_hip.so must be built in-tree"
    assert _native.lib().mmx_device_count() >= 1, "no gfx950 device visible to libmmx_hip.so"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def volume():
    """One uint16 volume with blobs of the ladders' sizes; the blocks are cut from it at an odd x origin."""
    from magellanmapper_amd import synth
    return synth.make_volume(19, (48, 40, 80), 30, blob_sigma=2.5)


def _voxels(vol16, kind):
    return vol16 if kind == "u16" else (vol16 / 65535.0).astype(np.float32)


def _candidates(table, n):
    t = table[:n]
    t = t[(t["flags"] & 4) == 0]                             # MMX_CAND_PROBE
    order = np.lexsort(tuple(t[k] for k in ("x", "y", "z", "s", "slot")))
    return t[order]


def _families(kinds):
    return {k: int(kinds[k][1]) for k in FAMILIES if kinds[k][1]}


def _ladder_run(bl, nat, vol, origin, shape, lo_sigma, hi_sigma, ns, value_range=0.0, by_name=None):
    """One block through ``mmx_log_scales_f32`` (the report) and ``mmx_detect_batch`` (the table); with ``by_name``
    instead every scale by ``mmx_log_batch_f32`` in the given mode WITHOUT entries, then the dense NMS, the probes and
    the re-score: the same float32 cube, nominated from every voxel."""
    L = nat.lib()
    dvol = bl.DeviceVolume(vol)
    dev = dvol.tensor.device
    lane = bl.Lane(0, lo_sigma, hi_sigma, ns, 0.05, 0.5)
    lane.bind(dvol, 1)
    space = lane.space
    blocks, slot = bl._make_blocks(dvol, 0, [origin], [shape])
    d_blocks = bl._to_device_bytes(blocks, dev)
    v32, vex = dvol.view(0, True), dvol.view(0, False)
    v32.value_range = value_range
    ws = torch.empty(-(-int(L.mmx_workspace_bytes(1, slot, ns, 1)) // 4), dtype=torch.float32, device=dev)
    cap = 65536
    table = torch.zeros(cap * nat.CAND_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    a = nat.DetectArgs()
    a.vol32, a.vol_exact = ctypes.pointer(v32), ctypes.pointer(vex)
    a.d_blocks, a.h_blocks, a.n_blocks, a.n_sigma, a.slot_elems = d_blocks.data_ptr(), blocks.ctypes.data, 1, ns, slot
    a.h_w0, a.h_w2 = space.w0_tab.ctypes.data, space.w2_tab.ctypes.data
    a.d_w0, a.d_w2 = lane.d_w0.data_ptr(), lane.d_w2.data_ptr()
    a.h_radius, a.h_norm = space.radii.ctypes.data, space.norms.ctypes.data
    a.d_work, a.work_bytes, a.thr, a.eps = ws.data_ptr(), ws.numel() * 4, lane.threshold, lane.eps
    a.d_cands, a.cap, a.d_count = table.data_ptr(), cap, count.data_ptr()
    a.zx_mode, a.zx_flags, a.store_f32, a.exact, a.expand = nat.MMX_ZX_AUTO, 0, 0, 1, 1
    a.stream = a.tail_stream = a.pack_stream = stream
    info = nat.DetectInfo()
    if by_name is None:
        half = nat.DetectInfo()
        nat.check(L.mmx_log_scales_f32(ctypes.byref(a), ctypes.byref(half)), "mmx_log_scales_f32")
        nat.check(L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info)), "mmx_detect_batch")
        torch.cuda.synchronize()
        assert ((half.zx_path, half.mask_layout, half.n_pass_rounds, half.q16_bound) ==
                (info.zx_path, info.mask_layout, info.n_pass_rounds, info.q16_bound))
    else:
        log_base = ws.data_ptr() + 4 * slot * 4
        for s in range(ns):
            path = ctypes.c_int(-1)
            nat.check(L.mmx_log_batch_f32(ctypes.byref(v32), d_blocks.data_ptr(), blocks.ctypes.data, 1, slot,
                                          nat.as_double_ptr(space.w0[s]), nat.as_double_ptr(space.w2[s]),
                                          int(space.radii[s]), float(space.norms[s]), log_base + s * slot * 4,
                                          ws.data_ptr(), None, 0.0, 0.0, None, by_name[s], ctypes.byref(path),
                                          stream), "mmx_log_batch_f32")
            assert path.value == by_name[s]
        nat.check(L.mmx_peaks_batch(log_base, None, 0, ns, d_blocks.data_ptr(), blocks.ctypes.data, 1, slot,
                                    lane.threshold, lane.eps, table.data_ptr(), cap, count.data_ptr(), stream),
                  "mmx_peaks_batch")
        nat.check(L.mmx_expand_probes(table.data_ptr(), cap, count.data_ptr(), count.data_ptr() + 4,
                                      d_blocks.data_ptr(), 1, ns, stream), "mmx_expand_probes")
        nat.check(L.mmx_rescore_f64(ctypes.byref(vex), d_blocks.data_ptr(), 1, table.data_ptr(), cap, count.data_ptr(),
                                    lane.d_w0.data_ptr(), lane.d_w2.data_ptr(), nat.as_int32_ptr(space.radii),
                                    nat.as_double_ptr(space.norms), ns, 0, stream), "mmx_rescore_f64")
        torch.cuda.synchronize()
    n_all = int(count.cpu().numpy().view(np.uint32)[0])
    assert 0 < n_all <= cap
    return info, _candidates(table.cpu().numpy().view(nat.CAND_DTYPE), n_all), space


def _check_ladder(bl, nat, vol, origin, shape, sigmas, value_range, want_radii, want_info, by_name, want_families):
    """The report, the candidates against the by-name reference, and the launches of one extra, timed run (the ladder
    runs twice in it: ``mmx_log_scales_f32``, then ``mmx_detect_batch``)."""
    info, cands, space = _ladder_run(bl, nat, vol, origin, shape, *sigmas, value_range=value_range)
    assert [int(r) for r in space.radii] == want_radii
    zx_path, layout, rounds, bounded = want_info
    print("info: path %d layout %d rounds %d q16_bound %g" % (info.zx_path, info.mask_layout, info.n_pass_rounds, info.q16_bound))
    assert (info.zx_path, info.mask_layout, info.n_pass_rounds) == (zx_path, layout, rounds)
    # (the bound of the worst scale in value units -- the range is 1 here -- or 0 when the last scale ran no 16-bit tiles)
    assert info.q16_bound == (space.q16_bound() if bounded else 0.0)
    _, dense, _ = _ladder_run(bl, nat, vol, origin, shape, *sigmas, value_range=value_range, by_name=by_name)
    assert len(dense) > 0 and len(cands) == len(dense)
    for f in ("slot", "s", "z", "y", "x", "v", "v64"):
        np.testing.assert_array_equal(cands[f], dense[f], err_msg=f)
    nat.timing_enable(True)
    try:
        nat.timing_read()
        _ladder_run(bl, nat, vol, origin, shape, *sigmas, value_range=value_range)
        kinds = nat.timing_read()
    finally:
        nat.timing_enable(False)
    print("families:", _families(kinds))
    assert _families(kinds) == {k: 2 * n for k, n in want_families.items()}


# ---------------------------------------------------------------- A. a ladder whose scales disagree
def test_a_mixed_ladder_launches_its_final_configuration_only(gpu, volume):
    """Radii 6 and 18 on a uint16 block of 40 x 20 x 40: radius 18 needs 22 rows for the fused path and has 20, so it
    takes the separate passes (Z and X on the register-ring kernels, Y generic) and writes no entries, radius 6 takes the
    16-bit tiles and would write quads -- the rules settle on no entries, the second configuration they go through.
    The report and the candidates are the parent's; only that configuration is launched (the parent launched both: 4 of
    each family below instead of 2)."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    _check_ladder(bl, nat, volume, (3, 7, 5), (40, 20, 40), (1.5, 4.5, 2), 0.0, [6, 18],
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
    from magellanmapper_amd import _native as nat, blob_log as bl
    _check_ladder(bl, nat, _voxels(volume, kind), (0, 0, 5), (48, 40, 64), (1.0, 3.0, 3), value_range, [4, 8, 12],
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
    from magellanmapper_amd import _native as nat, blob_log as bl
    L = nat.lib()
    rows = _golden_rows()
    assert len(rows) >= 30 and {r[2] for r in rows} == {-1, 0, 2, 6, 7, 8}
    origin, shape, R = (0, 0, 5), (48, 40, 64), 8
    space = bl.ScaleSpace.make(2.0, 2.0, 1)
    assert space.radii[0] == R
    stream = torch.cuda.current_stream().cuda_stream
    held = {}
    for dtype, vrange, mode, y_valu, prepacked, entries, band, want in rows:
        kind = {nat.MMX_U16: "u16", nat.MMX_F32: "f32"}[dtype]
        if kind not in held:
            dvol = bl.DeviceVolume(_voxels(volume, kind))
            blocks, slot = bl._make_blocks(dvol, 0, [origin], [shape])
            held[kind] = (dvol, blocks, slot, bl._to_device_bytes(blocks, dvol.tensor.device))
        dvol, blocks, slot, d_blocks = held[kind]
        ws = torch.empty(-(-int(L.mmx_workspace_bytes(1, slot, 1, 1)) // 4), dtype=torch.float32, device=dvol.tensor.device)
        mask_base = (ws.data_ptr() + 5 * slot * 4 + 15) & ~15
        v32 = dvol.view(0, True)
        assert v32.dtype == dtype
        v32.value_range = vrange
        if prepacked:
            nat.check(L.mmx_zx_pack(ctypes.byref(v32), d_blocks.data_ptr(), blocks.ctypes.data, 1, slot, ws.data_ptr(),
                                    stream), "mmx_zx_pack")
        zx_mode = mode | (nat.MMX_ZX_Y_VALU if y_valu else 0) | (nat.MMX_ZX_PREPACKED if prepacked else 0)
        written, path = ctypes.c_int(-1), ctypes.c_int(-1)
        nat.timing_enable(True)
        try:
            nat.timing_read()
            nat.check(L.mmx_log_batch_f32(ctypes.byref(v32), d_blocks.data_ptr(), blocks.ctypes.data, 1, slot,
                                          nat.as_double_ptr(space.w0[0]), nat.as_double_ptr(space.w2[0]), R,
                                          float(space.norms[0]), ws.data_ptr() + 4 * slot * 4, ws.data_ptr(),
                                          mask_base if entries else None, 0.05 - band, band,
                                          ctypes.byref(written) if entries else None, zx_mode, ctypes.byref(path), stream),
                      "mmx_log_batch_f32")
            kinds = nat.timing_read()
        finally:
            nat.timing_enable(False)
        family, q16, copy, y, rings, layout, zx_path = want
        if family == 0:
            ring = [bool(rings & 1), bool(rings & 2), bool(rings & 4)]
            fams = dict(zpass=int(ring[0]), ypass=int(ring[1]), xpass=int(ring[2]), generic=3 - sum(ring))
        elif family == 1:
            fams = dict(widepass=3)
        else:
            fams = dict(zxpack=copy, zxpass=1, y2pass=1)
        got = (path.value, written.value if entries else 0, _families(kinds))
        row = (kind, vrange, mode, y_valu, prepacked, entries, band)
        print(row, "->", got)
        assert got == (zx_path, layout, {k: n for k, n in fams.items() if n}), row
