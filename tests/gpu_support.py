"""What the GPU test files share, stated once: the ``gpu`` fixture, the voxel-type, timing and candidate-key helpers and
the one-block ladder run of test_gpu_routes.py / test_gpu_wide_radius.py.  A helper whose bodies differ between files
stays in those files.  A plain module (pytest does not rewrite its assertions): every ``assert`` here carries its values
in a message."""
import ctypes
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    from magellanmapper_amd import _native
    assert os.path.exists(_native.LIB_PATH), "libmmx_hip.so must be built in-tree: no %s" % _native.LIB_PATH
    n = _native.lib().mmx_device_count()
    assert n >= 1, "no gfx950 device visible to libmmx_hip.so (mmx_device_count() = %d)" % n
    return torch.device("cuda", 0)


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def as_dtype(vol16, dtype):
    """One uint16 volume in each of the four voxel types the ABI takes."""
    if dtype == np.uint16:
        return vol16
    if dtype == np.uint8:
        return (vol16 >> 8).astype(np.uint8)
    return (vol16 / 65535.0).astype(dtype)


def cand_key(rows):
    """``(slot, s, z, y, x)`` of candidate records as an ``(n, 5)`` int64 array."""
    return np.stack([rows[f].astype(np.int64) for f in ("slot", "s", "z", "y", "x")], axis=1)


def rescore_strip(rmax):
    """Columns the re-score stages at once for a batch whose largest radius is ``rmax`` (mmx_rescore.hip, whose LDS
    budget is 60 KiB)."""
    n = 2 * rmax + 1
    return min(n, (60 * 1024 - 32 * n - 16) // (16 * n))


def timed_cubes(dvol, origins, shapes, space, generic=False):
    """``log_cube_blocks`` with the per-kernel events on: ``(cubes, kinds)``."""
    from magellanmapper_amd import blob_log as bl
    from magellanmapper_amd.rawbatch import timed
    return timed(lambda: bl.log_cube_blocks(dvol, 0, origins, shapes, space, generic=generic))


def ladder_run(vol, origin, shape, lo_sigma, hi_sigma, ns, value_range=None, by_name=None):
    """One block through ``mmx_log_scales_f32`` (the report) and ``mmx_detect_batch`` (the table); with ``by_name``
    instead every scale by ``mmx_log_batch_f32`` in the given mode WITHOUT entries, then the dense NMS, the probes and
    the re-score: the same float32 cube, nominated from every voxel.  ``(info, candidates, scale space)``."""
    import torch
    from magellanmapper_amd import _native as nat, blob_log as bl
    from magellanmapper_amd.rawbatch import RawBatch
    L = nat.lib()
    dvol = bl.DeviceVolume(vol)
    lane = bl.Lane(0, lo_sigma, hi_sigma, ns, 0.05, 0.5)
    lane.bind(dvol, 1)
    b = RawBatch(dvol, [origin], [shape], lane.space, lane.threshold, lane.eps, 65536, value_range=value_range)
    info = nat.DetectInfo()
    if by_name is None:
        half = b.log_scales()
        info = b.detect()
        torch.cuda.synchronize()
        reports = [(i.zx_path, i.mask_layout, i.n_pass_rounds, i.q16_bound) for i in (half, info)]
        assert reports[0] == reports[1], "mmx_log_scales_f32 reports %s, mmx_detect_batch %s" % tuple(reports)
    else:
        table, count, d_blocks = b.tables[0].data_ptr(), b.counts_dev[0].data_ptr(), b.d_blocks.data_ptr()
        for s in range(ns):
            path = b.log_batch(s, by_name[s])
            assert path == by_name[s], "scale %d asked for mode %d ran path %d" % (s, by_name[s], path)
        nat.check(L.mmx_peaks_batch(b.log_base, None, 0, ns, d_blocks, b.blocks.ctypes.data, 1, b.slot, b.thr, b.eps,
                                    table, b.cap, count, b.stream), "mmx_peaks_batch")
        nat.check(L.mmx_expand_probes(table, b.cap, count, count + 4, d_blocks, 1, ns, b.stream), "mmx_expand_probes")
        nat.check(L.mmx_rescore_f64(ctypes.byref(b.vex), d_blocks, 1, table, b.cap, count, b.d_w0.data_ptr(),
                                    b.d_w2.data_ptr(), nat.as_int32_ptr(b.space.radii), nat.as_double_ptr(b.space.norms),
                                    ns, 0, b.stream), "mmx_rescore_f64")
        torch.cuda.synchronize()
    n_all = b.counts()[0]
    assert 0 < n_all <= b.cap, "%d entries in a table of %d" % (n_all, b.cap)
    return info, b.candidates(), b.space
