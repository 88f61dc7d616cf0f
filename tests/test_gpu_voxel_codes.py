"""GPU test of argument checking: every ``extern "C"`` entry that takes an ``mmx_volume`` refuses a dtype code that names
no voxel type (-1 and 5) with the status stated here, and writes nothing.

One block of 4 x 6 x 16 voxels.  Every other argument of every call is valid, so the dtype alone decides; the volume's
buffer is 8 bytes a voxel, the widest type, and every output is sized for the call as if it ran -- a build that launched
after all would read and write inside its buffers, and fail the sentinel check rather than fault.  The outputs and the
workspaces are filled with a sentinel byte and compared whole after the call.

The statuses (mmx_voxel.h: the refusal each entry hands the dispatcher, or its own check of the accepted set):
MMX_ERR_ARG from mmx_rescore_f64, mmx_order_stats and mmx_extract_patches; MMX_ERR_UNSUPPORTED everywhere else.
mmx_detect_batch is called with the bad code in ``vol32``, which its LoG passes refuse ahead of the first launch (a bad
``vol_exact`` alone is refused by the re-score behind the passes, after they have written: not a case here)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MMX_ERR_ARG, MMX_ERR_UNSUPPORTED = 1, 5
SENTINEL = 0xA5
NZ, NY, NX, PX = 4, 6, 16, 32
SLOT = NZ * NY * PX
TAB = 256               # MMX_MAX_RADIUS_GENERIC + 1: the pitch of a scale's weights in mmx_detect_args


class _Call:
    """The buffers of one call: sentinel-filled outputs, and the inputs kept alive until the check."""

    def __init__(self, gpu, code):
        from magellanmapper_amd import _native as nat
        self.nat, self.gpu, self.outs, self.keep = nat, gpu, [], []
        self.lib = nat.lib()
        self.stream = torch.cuda.current_stream().cuda_stream
        data = self.dev(np.zeros(NZ * NY * NX, dtype=np.float64))
        self.vol = nat.Volume(data, code, 0.0, NY * NX, NX, 1)
        blocks = np.zeros(1, dtype=nat.BLOCK_DTYPE)
        blocks[0] = (0, NZ, NY, NX, 0, PX, 0)
        self.h_blocks = self.host(blocks)
        self.d_blocks = self.dev(blocks)

    def host(self, arr):
        self.keep.append(arr)
        return arr.ctypes.data

    def dev(self, arr):
        t = torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).to(self.gpu)
        self.keep.append(t)
        return t.data_ptr()

    def out(self, nbytes):
        t = torch.full((int(nbytes),), SENTINEL, dtype=torch.uint8, device=self.gpu)
        self.outs.append(t)
        return t.data_ptr()

    def check(self, status, want):
        torch.cuda.synchronize()
        assert status == want
        assert self.outs, "a call without outputs checks nothing"
        for t in self.outs:
            assert bool((t == SENTINEL).all()), "a refused call wrote to an output"


def _doubles(*values):
    return (ctypes.c_double * len(values))(*values)


def _log_batch(c):
    work = c.out(c.lib.mmx_workspace_bytes(1, SLOT, 1, 1))
    return c.lib.mmx_log_batch_f32(ctypes.byref(c.vol), c.d_blocks, c.h_blocks, 1, SLOT, _doubles(0.5, 0.25), _doubles(-0.5, 0.25),
                                   1, 1.0, c.out(SLOT * 4), work, None, 0.0, 0.0, None, c.nat.MMX_ZX_AUTO, None, c.stream)


def _log_batch_generic(c):
    return c.lib.mmx_log_batch_f32_generic(ctypes.byref(c.vol), c.d_blocks, c.h_blocks, 1, SLOT, _doubles(0.5, 0.25),
                                           _doubles(-0.5, 0.25), 1, 1.0, c.out(SLOT * 4), c.out(4 * SLOT * 4), c.stream)


def _zx_pack(c):
    return c.lib.mmx_zx_pack(ctypes.byref(c.vol), c.d_blocks, c.h_blocks, 1, SLOT, c.out(4 * SLOT * 4), c.stream)


def _detect_args(c):
    nat = c.nat
    w0, w2 = np.zeros(TAB), np.zeros(TAB)
    w0[:2], w2[:2] = (0.5, 0.25), (-0.5, 0.25)
    radius, norm = np.array([1], dtype=np.int32), np.array([1.0])
    a = nat.DetectArgs()                # (filled by hand on purpose: every output is a sentinel-tracked buffer of `c`)
    c.keep.append(c.vol)
    a.vol32 = a.vol_exact = ctypes.pointer(c.vol)
    a.d_blocks, a.h_blocks, a.n_blocks, a.n_sigma, a.slot_elems = c.d_blocks, c.h_blocks, 1, 1, SLOT
    a.h_w0, a.h_w2, a.d_w0, a.d_w2 = c.host(w0), c.host(w2), c.dev(w0), c.dev(w2)
    a.h_radius, a.h_norm = c.host(radius), c.host(norm)
    a.work_bytes = c.lib.mmx_workspace_bytes(1, SLOT, 1, 1)
    a.d_work = c.out(a.work_bytes)
    a.thr, a.eps = 0.1, 1e-5
    a.d_cands, a.cap, a.d_count = c.out(16 * nat.CAND_DTYPE.itemsize), 16, c.out(8)
    a.zx_mode, a.exact, a.expand, a.stream = nat.MMX_ZX_AUTO, 1, 1, c.stream
    return a


def _log_scales(c):
    return c.lib.mmx_log_scales_f32(ctypes.byref(_detect_args(c)), ctypes.byref(c.nat.DetectInfo()))


def _detect_batch(c):
    return c.lib.mmx_detect_batch(ctypes.byref(_detect_args(c)), ctypes.byref(c.nat.DetectInfo()))


def _rescore(c):
    w = np.zeros(TAB)
    return c.lib.mmx_rescore_f64(ctypes.byref(c.vol), c.d_blocks, 1, c.out(4 * c.nat.CAND_DTYPE.itemsize), 4,
                                 c.dev(np.array([4, 4], dtype=np.uint32)), c.dev(w), c.dev(w),
                                 (ctypes.c_int32 * 1)(1), _doubles(1.0), 1, 0, c.stream)


def _preprocess(which):
    def run(c):
        nat = c.nat
        subs = np.zeros(1, dtype=nat.SUBBLOCK_DTYPE)
        subs[0] = (0, 0, 0, NZ, NY, NX, 0)
        qc = np.zeros(1, dtype=nat.QCLASS_DTYPE)
        n = NZ * NY * NX
        qc[0] = (0, 1, n - 2, n - 1, 0.5, 0.5)
        params = nat.PreprocParams(0.0, 1.0, 0.0, 0.3, 0.0, 32, 0, 0.0, 0.0)
        head = (ctypes.byref(c.vol), c.dev(subs), c.host(subs), 1, c.dev(qc), 1, ctypes.byref(params), c.dev(np.zeros(33)),
                PX, NY * PX, c.out(SLOT * 4), c.out(SLOT * 8), c.out(nat.SUBINFO_DTYPE.itemsize))
        if which == "batch":
            return c.lib.mmx_preprocess_batch(*head, c.stream)
        if which == "mode":
            work = int(c.lib.mmx_preprocess_work_bytes(c.host(subs), 1))
            return c.lib.mmx_preprocess_batch_mode(*head, 0, 0, c.out(max(work, 256)), max(work, 256), c.stream)
        return c.lib.mmx_preprocess_batch_generic(*head, c.out(7 * n * 8), 7 * n, c.stream)
    return run


def _coloc(voxels):
    def run(c):
        blobs, offsets = np.array([[0, 2, 3, 8, 0]], dtype=np.int32), np.array([0, 1], dtype=np.int32)
        args = (ctypes.byref(c.vol), c.d_blocks, 1, c.dev(blobs), c.dev(offsets), 1, c.out(8), c.out(4))
        if voxels:
            return c.lib.mmx_coloc_voxels(*args, c.out(c.nat.MMX_COLOC_BALL * 8), c.stream)
        return c.lib.mmx_coloc_means(*args, c.stream)
    return run


def _unmix(c):
    sub = c.nat.Volume(c.vol.d_data, c.vol.dtype, 0.0, NY * NX, NX, 1)
    return c.lib.mmx_unmix_batch(ctypes.byref(c.vol), ctypes.byref(sub), _doubles(0.5), 1, c.d_blocks, c.h_blocks, 1,
                                 SLOT, PX, NY * PX, c.out(SLOT * 4), c.out(SLOT * 8), c.stream)


def _minmax(c):
    return c.lib.mmx_minmax_batch(ctypes.byref(c.vol), c.d_blocks, c.h_blocks, 1, c.out(16), c.stream)


def _gauss_axis(c):
    return c.lib.mmx_gauss_axis_batch(ctypes.byref(c.vol), c.d_blocks, c.h_blocks, 1, 2, c.dev(np.array([0.5, 0.25])),
                                      c.dev(np.array([1], dtype=np.int32)), 2, 0, SLOT, PX, NY * PX, c.out(SLOT * 8), c.stream)


def _resize(out_code):
    def run(c):
        nat = c.nat
        rb = np.zeros(1, dtype=nat.RESIZE_DTYPE)
        rb[0] = (0, NZ, NY, NX, NZ, NY, NX, 0, 0, NZ, NZ + NY)
        n_tab = NZ + NY + NX
        index = np.zeros((n_tab, 2), dtype=np.int32)
        weight = np.tile(np.array([1.0, 0.0]), (n_tab, 1))
        head = (ctypes.byref(c.vol), c.dev(rb), c.host(rb), 1, c.dev(index), c.dev(weight), c.dev(np.array([0.0, 1.0])),
                SLOT, PX, NY * PX)
        if out_code is None:
            return c.lib.mmx_resize_batch(*head, c.out(SLOT * 8), c.out(SLOT * 4), c.stream)
        return c.lib.mmx_resize_batch_as(*head, out_code, c.out(SLOT * 8), c.out(SLOT * 4), c.stream)
    return run


def _order_stats(c):
    groups = np.zeros(1, dtype=c.nat.RANK_GROUP_DTYPE)
    groups[0] = (0, NZ, (0, 1, 2, 3))
    work = int(c.lib.mmx_order_stats_workspace(1))
    return c.lib.mmx_order_stats(ctypes.byref(c.vol), NZ, NY, NX, c.dev(groups), c.host(groups), 1, c.out(4 * 8), c.out(4),
                                 c.out(work), work, c.stream)


def _patches(c):
    zyx = np.array([[2, 3, 8]], dtype=np.int32)
    return c.lib.mmx_extract_patches(ctypes.byref(c.vol), c.dev(zyx), 1, 4, c.out(16 * 8), c.out(16 * 4), c.stream)


ENTRIES = [
    ("mmx_log_batch_f32", _log_batch, MMX_ERR_UNSUPPORTED),
    ("mmx_log_batch_f32_generic", _log_batch_generic, MMX_ERR_UNSUPPORTED),
    ("mmx_zx_pack", _zx_pack, MMX_ERR_UNSUPPORTED),
    ("mmx_log_scales_f32", _log_scales, MMX_ERR_UNSUPPORTED),
    ("mmx_detect_batch", _detect_batch, MMX_ERR_UNSUPPORTED),
    ("mmx_rescore_f64", _rescore, MMX_ERR_ARG),
    ("mmx_preprocess_batch", _preprocess("batch"), MMX_ERR_UNSUPPORTED),
    ("mmx_preprocess_batch_mode", _preprocess("mode"), MMX_ERR_UNSUPPORTED),
    ("mmx_preprocess_batch_generic", _preprocess("generic"), MMX_ERR_UNSUPPORTED),
    ("mmx_coloc_means", _coloc(False), MMX_ERR_UNSUPPORTED),
    ("mmx_coloc_voxels", _coloc(True), MMX_ERR_UNSUPPORTED),
    ("mmx_unmix_batch", _unmix, MMX_ERR_UNSUPPORTED),
    ("mmx_minmax_batch", _minmax, MMX_ERR_UNSUPPORTED),
    ("mmx_gauss_axis_batch", _gauss_axis, MMX_ERR_UNSUPPORTED),
    ("mmx_resize_batch", _resize(None), MMX_ERR_UNSUPPORTED),
    ("mmx_resize_batch_as", _resize(0), MMX_ERR_UNSUPPORTED),
    ("mmx_order_stats", _order_stats, MMX_ERR_ARG),
    ("mmx_extract_patches", _patches, MMX_ERR_ARG),
]


def test_every_entry_that_takes_a_volume_is_listed():
    """The header's entries with an mmx_volume argument (mmx_detect_args carries two) are the ones called here."""
    import os
    import re
    from conftest import ROOT
    header = open(os.path.join(ROOT, "include", "mmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    takes = set(re.findall(r"\b(mmx_\w+)\s*\([^;{]*?\bmmx_(?:volume|detect_args)\s*\*", header))
    takes -= {"mmx_detect_batch_capture"}       # (mmx_detect_batch under a stream capture: the same checks, no second case)
    assert takes == {name for name, _, _ in ENTRIES}


@pytest.mark.parametrize("code", [-1, 5])
def test_a_code_that_names_no_voxel_type_is_refused_and_nothing_is_written(code):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    gpu = torch.device("cuda", 0)
    for name, run, want in ENTRIES:
        c = _Call(gpu, code)
        try:
            c.check(run(c), want)
        except AssertionError as exc:
            raise AssertionError(f"{name}, dtype code {code}: {exc}") from exc
