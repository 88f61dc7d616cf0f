"""One batch of blocks driven through the C ABI from raw pointers: what the GPU tests and the A/B tools under ``tools/``
build ``mmx_detect_batch`` / ``mmx_log_scales_f32`` / ``mmx_log_batch_f32`` calls from.  The second, independent
statement of how a caller fills ``mmx_detect_args`` -- the product's is ``blob_log._detect_args``, which does not use
this module and is cross-checked by the tests that do.

The workspace layout is stated here for tests and tools (``test_gpu_parity.py::_abi_batch`` alone keeps a layout of its
own on purpose, with the entries in a buffer of their own).  Its source is ``mmx_workspace_bytes`` in
``include/mmx.h``: ``[d_work | d_log x n_sigma | pad to 16 | entries]``, in floats of ``n = n_blocks * slot_elems``:
four intermediate arrays ``[0, 4 n)``, the LoG array of scale ``s`` at ``(4 + s) n`` with block ``b`` at ``b * slot_elems``
as ``[nz][ny][px]``, and behind the last one, 16-byte aligned, the NMS entries of 16 bytes each (word 0: candidates,
word 1: above the threshold), block ``b`` starting ``(b * slot_elems) >> 5`` entries in."""
import ctypes

import numpy as np
import torch

from . import _native as nat
from . import blob_log as bl


def timed(fn):
    """``fn()`` with the per-kernel events on: ``(result, kinds)``, ``kinds`` as ``nat.timing_read`` gives them."""
    nat.timing_enable(True)
    try:
        nat.timing_read()
        out = fn()
        kinds = nat.timing_read()
    finally:
        nat.timing_enable(False)
    return out, kinds


def families(kinds, names):
    """Launches per kernel family of ``names``, the families that did not run left out."""
    return {k: int(kinds[k][1]) for k in names if kinds[k][1]}


def _space_of(scales):
    return scales if isinstance(scales, bl.ScaleSpace) else bl.ScaleSpace.make(*scales)


class RawBatch:
    """Channel 0 of ``volume`` (host array, device tensor or ``DeviceVolume``) cut into the blocks ``origins`` /
    ``shapes``, with everything one call needs kept alive: block records, volume views, weight tables, workspace,
    ``n_tables`` candidate tables of ``cap`` entries with their counters (initially ``count_fill``) and, on request,
    a pinned table of ``host_entries`` entries with pinned counters and an event.  ``scales``: a ``ScaleSpace`` or
    ``(min_sigma, max_sigma, num_sigma)``.  ``slot`` / ``value_range``: ``slot_elems`` and the float32 view's range where
    they are not what ``_make_blocks`` / the volume report.  The remaining keywords are the fields of
    ``mmx_detect_args`` of the same names."""

    def __init__(self, volume, origins, shapes, scales, threshold, eps, cap, *, slot=None, value_range=None, store_f32=0,
                 zx_mode=nat.MMX_ZX_AUTO, zx_flags=0, exact=1, expand=1, host_entries=None, event=False, count_fill=0,
                 n_tables=1):
        self.L = nat.lib()
        self.dvol = volume if isinstance(volume, bl.DeviceVolume) else bl.DeviceVolume(volume)
        self.dev = dev = self.dvol.tensor.device
        self.space = _space_of(scales)
        self.d_w0, self.d_w2 = self.space.device_tables(dev)
        self.origins, self.shapes = list(origins), list(shapes)
        self.blocks, self.blocks_slot = bl._make_blocks(self.dvol, 0, self.origins, self.shapes)
        self.d_blocks = bl._to_device_bytes(self.blocks, dev)
        self.slot = self.blocks_slot if slot is None else slot
        self.nb, self.ns = len(self.blocks), len(self.space.sigmas)
        self.v32, self.vex = self.dvol.view(0, True), self.dvol.view(0, False)
        if value_range is not None:
            self.v32.value_range = value_range
        self.ws = torch.empty(-(-int(self.L.mmx_workspace_bytes(self.nb, self.slot, self.ns, 1)) // 4), dtype=torch.float32,
                              device=dev)
        self.thr, self.eps, self.cap = threshold, eps, cap
        item = nat.CAND_DTYPE.itemsize
        self.tables = [torch.zeros(cap * item, dtype=torch.uint8, device=dev) for _ in range(n_tables)]
        self.counts_dev = [torch.full((2,), count_fill, dtype=torch.int32, device=dev) for _ in range(n_tables)]
        self.h_count = self.h_table = self.event = None
        self.host_entries = host_entries
        if host_entries is not None:
            self.h_count = torch.full((2,), count_fill, dtype=torch.int32).pin_memory()
            self.h_table = torch.zeros(host_entries * item, dtype=torch.uint8).pin_memory()
        if event:
            self.event = bl._NativeEvent()
        self.stream = bl._stream_ptr()
        self.mode = dict(zx_mode=int(zx_mode), zx_flags=int(zx_flags), store_f32=int(store_f32), exact=int(exact),
                         expand=int(expand))

    def set_scales(self, scales):
        """Another ladder of the same number of scales on the same blocks, workspace and tables."""
        space = _space_of(scales)
        if len(space.sigmas) != self.ns:
            raise ValueError("the workspace is sized for %d scales" % self.ns)
        self.space = space
        self.d_w0, self.d_w2 = space.device_tables(self.dev)

    # ------------------------------------------------------------------------------------------------- the calls
    def args(self, **overrides):
        """A fresh ``mmx_detect_args`` on the first table; ``overrides``: fields set last."""
        a, space = nat.DetectArgs(), self.space
        a.vol32, a.vol_exact = ctypes.pointer(self.v32), ctypes.pointer(self.vex)
        a.d_blocks, a.h_blocks = self.d_blocks.data_ptr(), self.blocks.ctypes.data
        a.n_blocks, a.n_sigma, a.slot_elems = self.nb, self.ns, self.slot
        a.h_w0, a.h_w2, a.d_w0, a.d_w2 = (space.w0_tab.ctypes.data, space.w2_tab.ctypes.data, self.d_w0.data_ptr(),
                                          self.d_w2.data_ptr())
        a.h_radius, a.h_norm = space.radii.ctypes.data, space.norms.ctypes.data
        a.d_work, a.work_bytes, a.thr, a.eps = self.ws.data_ptr(), self.ws.numel() * 4, self.thr, self.eps
        a.d_cands, a.cap, a.d_count = self.tables[0].data_ptr(), self.cap, self.counts_dev[0].data_ptr()
        if self.h_table is not None:
            a.h_count, a.h_cands, a.h_prefix = self.h_count.data_ptr(), self.h_table.data_ptr(), self.host_entries
        a.stream = a.tail_stream = a.pack_stream = self.stream
        if self.event is not None:
            a.ev_done = self.event.handle
        for k, v in dict(self.mode, **overrides).items():
            setattr(a, k, v)
        return a

    def log_scales(self, a=None):
        """``mmx_log_scales_f32``: its report."""
        info = nat.DetectInfo()
        nat.check(self.L.mmx_log_scales_f32(ctypes.byref(self.args() if a is None else a), ctypes.byref(info)),
                  "mmx_log_scales_f32")
        return info

    def detect(self, a=None):
        """``mmx_detect_batch`` (enqueued: the caller synchronises): its report."""
        info = nat.DetectInfo()
        rc = self.L.mmx_detect_batch(ctypes.byref(self.args() if a is None else a), ctypes.byref(info))
        nat.check(rc, "mmx_detect_batch [%s]" % self.L.mmx_detect_last_error().decode())
        return info

    def log_batch(self, s, mode, lo=0.0, band=0.0, entries=False):
        """``mmx_log_batch_f32`` of scale ``s`` in ``mode`` with ``nms_lo = lo`` and ``nms_eps = band`` into that scale's
        LoG array: the path.  With ``entries`` the NMS entries are asked for too: then ``(path, entry layout written)``."""
        space, path, written = self.space, ctypes.c_int(-1), ctypes.c_int(-1)
        nat.check(self.L.mmx_log_batch_f32(ctypes.byref(self.v32), self.d_blocks.data_ptr(), self.blocks.ctypes.data,
                                           self.nb, self.slot, nat.as_double_ptr(space.w0[s]),
                                           nat.as_double_ptr(space.w2[s]), int(space.radii[s]), float(space.norms[s]),
                                           self.log_base + s * self.nb * self.slot * 4, self.ws.data_ptr(),
                                           self.entries_base if entries else None, lo, band,
                                           ctypes.byref(written) if entries else None, mode, ctypes.byref(path),
                                           self.stream), "mmx_log_batch_f32")
        return (path.value, written.value) if entries else path.value

    # -------------------------------------------------------------------------------------- the workspace layout
    @property
    def log_base(self):
        """Device address of the first LoG array."""
        return self.ws.data_ptr() + 4 * self.nb * self.slot * 4

    @property
    def entries_base(self):
        """Device address of the NMS entries."""
        return (self.log_base + self.ns * self.nb * self.slot * 4 + 15) & ~15

    def log_arrays(self):
        """The LoG arrays on the host, ``[n_sigma][n_blocks * slot_elems]``."""
        n = self.nb * self.slot
        return self.ws[4 * n:(4 + self.ns) * n].cpu().numpy().reshape(self.ns, n)

    def cubes(self, flat):
        """One LoG array as per-block ``[nz][ny][px]`` views."""
        out = []
        for i, s in enumerate(self.shapes):
            px = int(self.blocks["px"][i])
            out.append(flat[i * self.slot:i * self.slot + s[0] * s[1] * px].reshape(s[0], s[1], px))
        return out

    def quads_written(self):
        """``MMX_MASK_QUADS`` entries of the first scale decoded: per block, ``[z][y][x]``, whether the voxel's entry
        has a bit above the threshold.  Entry ``y nwords + (z >> 2) ntx + (x >> 4)`` of a block holds 4 planes x 16
        columns of row ``y``; the Y pass writes those 64 values when any of them is above."""
        off = self.entries_base - self.ws.data_ptr()
        if off % 4:
            raise AssertionError("entries at byte %d of the workspace" % off)
        n = self.nb * self.slot
        words = self.ws[off // 4:off // 4 + (n >> 5) * 4].cpu().numpy().view(np.uint64).reshape(-1, 2)
        written = []
        for i, (nz, ny, nx) in enumerate(self.shapes):
            ntx, nzq = -(-nx // 16), -(-nz // 4)
            ent = words[(i * self.slot) >> 5:][:ny * nzq * ntx].reshape(ny, nzq, ntx, 2)
            on = ent[..., 1] != 0                                            # [y][z quad][column tile]
            vox = np.repeat(np.repeat(on, 4, axis=1), 16, axis=2)[:, :nz, :nx]
            written.append(np.moveaxis(vox, 0, 1))                           # [z][y][x]
        return written

    # ------------------------------------------------------------------------------------------------ the tables
    def counts(self, i=0, host=False):
        """``(n_all, n_cands)`` of table ``i``, or what the batch copied to the pinned counters."""
        words = self.h_count.numpy() if host else self.counts_dev[i].cpu().numpy()
        return tuple(int(v) for v in words.view(np.uint32))

    def table(self, i=0, host=False):
        """Table ``i`` (or the pinned copy of its head) as ``CAND_DTYPE`` records."""
        return (self.h_table.numpy() if host else self.tables[i].cpu().numpy()).view(nat.CAND_DTYPE)

    def candidates(self, i=0):
        """The entries of table ``i`` that are no probes, sorted by ``(slot, s, z, y, x)``."""
        t = self.table(i)[:self.counts(i)[0]]
        t = t[(t["flags"] & nat.MMX_CAND_PROBE) == 0]
        return t[np.lexsort(tuple(t[k] for k in ("x", "y", "z", "s", "slot")))]
