"""Device ``blob_log``: Laplacian-of-Gaussian scale-space blob detection on MI355X.

Drop-in for the one third-party call on the reference's hot path,
``skimage.feature.blob_log`` as ``magmap.cv.detector.detect_blobs`` uses it
(reference magmap/cv/detector.py:931-933), for batches of blocks of one volume:

=====  ==========================================  ================================
row    reference step                              here
=====  ==========================================  ================================
A0     ``img_as_float`` (skimage dtype.py:310-328)  folded into the Z-pass weights
A1     sigma ladder (skimage blob.py:473-497)       :func:`kernels1d.sigma_ladder`
A2,A3  ``-gaussian_laplace * sigma**2`` per scale   ``mmx_log_batch_f32`` (HIP)
A4     ``peak_local_max`` 3^4 NMS (peak.py)         the tail of ``mmx_detect_batch`` (HIP:
                                                    NMS, probes, exact re-score)
                                                    + tie resolution below
A5     ``_prune_blobs`` (blob.py:146-187)           ``mmx_overlap_pairs`` (HIP) +
                                                    the sequential rule below
=====  ==========================================  ================================

Exactness.  The float32 passes only *nominate* candidates (within ``eps`` of being a
maximum / of the threshold).  Wherever a decision of the reference could depend on more
than float32 resolves -- a candidate within ``eps`` of the threshold or of a neighbour, two
candidates of a block within ``eps`` of each other (their order) -- the float64 cube values
are recomputed on the device with SciPy's exact operation order (contested candidates also
get their 80 neighbours' exact values); by default every candidate is re-scored.  Peak
membership, the descending-response order and therefore the integer blob coordinates are
decided as the reference's float64 values decide them.  Nothing here falls back to a CPU implementation: without the HIP library and a
GPU the calls raise.
"""
from __future__ import annotations

import ctypes
import os
import time
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from . import kernels1d as k1

try:  # torch is the device-memory / stream plumbing
    import torch
except Exception as exc:  # pragma: no cover
    raise ImportError("magellanmapper_amd needs PyTorch-ROCm for device memory") from exc
#: half-width of the float32 "contested" band, relative to the input's value scale
EPS_REL = float(os.environ.get("MMX_EPS_REL", 2e-5))
#: the band for raw integer volumes, whose default kernels hand the Z+X results to the Y pass as 16-bit fixed point
#: (``MMX_ZX_TILED_Q16``: error <= 3.0e-5 of the value range from radius 4 on, ``mmx_tiled_q16_error_bound``); 0 keeps
#: float32 intermediates
EPS_REL_Q16 = float(os.environ.get("MMX_EPS_REL_Q16", 2.5e-4))
#: the rounding error of the 16-bit intermediates, relative to the value range, for kernel radii >= 4 (sigma >= 0.875;
#: largest at radius 5: 2.97e-5 -- swept over sigma in tests/test_host_logic.py; rounds 3-5 carried 5.3e-5: Q was
#: quantised over twice the range it can take, see ``mmx_q16_bounds`` in csrc/mmx_route.h).  Per call the library states the
#: bound of the sigmas at hand (``mmx_tiled_q16_error_bound``); the kernels of radius 1..3 carry up to 5.4e-5.
Q16_BOUND_ANY_SIGMA = 3.0e-5
#: ``MMX_LOG_ABS_TOL`` of include/mmx.h: the LoG contract in value units (BASELINE.json: "LoG response within 1e-4")
LOG_ABS_TOL = 1e-4
if 0.0 < EPS_REL_Q16 < 4.0 * Q16_BOUND_ANY_SIGMA:
    # exactness rests on the band covering the error fourfold: an environment variable may widen it or switch the
    # 16-bit intermediates off (0), not narrow it below what the bound needs
    raise ValueError(f"MMX_EPS_REL_Q16={EPS_REL_Q16:g} is narrower than 4 x the 16-bit intermediates' error bound "
                     f"({4.0 * Q16_BOUND_ANY_SIGMA:g}); use 0 to keep float32 intermediates")
#: EVERY batch is enqueued by one ``mmx_detect_batch`` call (voxel copy, the passes of every scale, NMS, probes, exact
#: re-score, copies).  This switch only says whether small raw batches on the native host path may be captured as a
#: hipGraph and replayed (``GRAPH_BLOCKS``); ``False``: plain ``mmx_detect_batch`` calls, never a graph
NATIVE_BATCH = True
#: batches of at most this many blocks that come back with the very same arguments (a small volume detected step
#: after step) are captured as a hipGraph and replayed with one launch (0: never)
GRAPH_BLOCKS = 8
#: with the per-kernel timing on: (before, after) event pairs around the LoG stream's wait for a batch's preprocessing
PRE_WAITS: list = []
#: batches replayed from a captured graph so far (bench.py reports the count of its timed region)
GRAPH_REPLAYS = 0
#: bound of the 16-bit intermediates of the most recent batch that used them (value units), else 0: bench.py prints it
LAST_Q16_BOUND = 0.0
#: nomination band (value units) of that batch
LAST_NMS_BAND = 0.0
#: host clock (time.perf_counter) at which the most recent batch's last kernel was seen complete
LAST_BATCH_DONE_T = 0.0
#: host clock at which the first batch of the most recent ``blob_log_blocks`` call had been handed to the GPU (the
#: "start" of a step: block lists, plans, tables -> first launch), and the batch sizes of that call (bench.py --share)
FIRST_ENQUEUED_T = 0.0
LAST_BATCH_SIZES: list = []
#: ``mmx_zx_mode`` passed with every ``mmx_log_batch_f32`` call (``MMX_FUSE`` in the environment overrides the
#: default for kernel experiments; tests set it to cross-check the kernels against each other)
ZX_MODE = int(os.environ.get("MMX_FUSE", nat.MMX_ZX_AUTO))
#: flags or-ed into the mode of the tiled calls: ``nat.MMX_ZX_Y_VALU`` runs the Y pass of the 16-bit tiles on the VALU
#: (``y6_kernel``) instead of the matrix cores (``ym_kernel``) -- cross-checks and A/B timing
ZX_FLAGS = 0
#: the ``mmx_zx_mode`` the most recent ``mmx_log_batch_f32`` call of this process actually ran
LAST_ZX_PATH = None
#: of the most recent batch (``mmx_detect_info``): how many times its scales were computed (1, or more when they had
#: to be computed again on another path) and the NMS entry layout its peaks were nominated from (0: the full cube)
LAST_PASS_ROUNDS = None
LAST_MASK_LAYOUT = None
#: who takes the per-batch decisions on the re-scored candidates: "native" (``mmx_host_resolve_peaks`` /
#: ``mmx_host_overlap_prune``: threaded, outside the GIL, no second device round trip) or "numpy" (the same rules as
#: array expressions; kept as a cross-check -- tests run both -- and for ``exact_values=False``)
HOST_PATH = os.environ.get("MMX_HOST_PATH", "native")
#: value scales (largest |voxel|, at least 1) up to which float voxels take the tiled matrix-core path: its float16
#: pieces overflow at 65504 (faint images are no problem: the nomination band never shrinks below EPS_REL x 1)
FLOAT_TILED_RANGE = (0.0, 2.0 ** 12)
#: per-block preprocessing on a stream of its own (beside the previous batch's LoG kernels)
PRE_STREAM = True
#: (the NMS / re-score tail of a PREPROCESSED batch stays on the main stream: DESIGN.md, "Host side of a step")
#: ... and this many batches ahead of the one the host is finishing (``preprocess.N_BUFFER_SETS`` - 1 buffer sets allow
#: it): the first batch is then the only one whose LoG passes wait for their preprocessing
PRE_AHEAD = 2
#: ... and this many BATCHES (x the number of lanes) when the preprocessed blocks are retained per block
PRE_AHEAD_RETAINED = 2
#: raw volumes: everything after a batch's last LoG kernel -- NMS, probe expansion, exact re-score, the copies of the
#: results to the host -- on a stream of its own, beside the LoG kernels of the next batch, which then work in a second
#: workspace (``_Buffers.workspace(n, 1)``: +16 GiB with the default budget).  Measured on the benchmark volume,
#: alternating runs on one box: 115.2 / 113.5 ms per volume without, 110.2 / 109.4 with (the NMS takes 8.3 instead of
#: 4.5 ms and the Z+X kernel 59 instead of 53 when they run beside each other; the re-score alone on the side stream,
#: one workspace: -2.8 ms)
RESCORE_STREAM = True

from . import batch_plan as _bp   # noqa: E402
from .batch_plan import (LIB_MAX_SLOT_ELEMS, MAX_PARTS, BatchPlan, PartSplit, PlannedBatch, _isolate_parents,   # noqa: F401,E402
                         _row_elems, _slot_elems, block_records, slot_limit, slot_refusal, split_oversized)
from .volume import (DeviceVolume, _SlabUpload, _img_as_float_host, _require_gpu, _stream_ptr,   # noqa: F401,E402
                     _NP_TO_MMX, _TORCH_DTYPES)
from .buffers import (_Buffers, _NativeEvent, _UploadRing, _buffers_for, _stream_wait, _to_device_bytes,   # noqa: F401,E402
                      release_buffers, to_device, _PREFIX_ENTRIES)
from .host_resolve import (OVERLAP_BAND, PeakBatch, VERIFIED_SCIPY, _BandTooNarrow, _apply_pairs,   # noqa: F401,E402
                           _check_f32_error, _exact_overlap, _prune_batch, _prune_batch_native,
                           _reference_pair_order, _resolve_peaks, _resolve_peaks_native)


@dataclass
class ScaleSpace:
    """Per-call filter parameters (never cached across calls: the reference re-reads its
    profile on every call and the grid search mutates it)."""
    sigmas: np.ndarray
    norms: np.ndarray
    radii: np.ndarray
    w0: List[np.ndarray]
    w2: List[np.ndarray]
    w0_tab: np.ndarray = field(default=None)
    w2_tab: np.ndarray = field(default=None)
    _dev: Optional[dict] = field(default=None, repr=False)
    _q16: Optional[float] = field(default=None, repr=False)

    @classmethod
    def make(cls, min_sigma: float, max_sigma: float, num_sigma: int) -> "ScaleSpace":
        """The filter parameters of ``blob_log(min_sigma, max_sigma, num_sigma)``: a pure function of the three
        numbers, so the last few are kept (the PROFILE is re-read at every call; what its numbers imply is not)."""
        if np.isscalar(min_sigma) and np.isscalar(max_sigma):
            key = (float(min_sigma), float(max_sigma), int(num_sigma))
            hit = _SPACES.get(key)
            if hit is None:
                if len(_SPACES) > 64:
                    _SPACES.clear()
                hit = _SPACES[key] = cls._make(min_sigma, max_sigma, num_sigma)
            return hit
        return cls._make(min_sigma, max_sigma, num_sigma)

    def device_tables(self, dev):
        """``(w0, w2)`` half-kernel tables on ``dev`` (for the exact re-score), uploaded once per device."""
        key = str(dev)
        if self._dev is None:
            self._dev = {}
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.w0_tab).to(dev), torch.from_numpy(self.w2_tab).to(dev))
        return self._dev[key]

    def q16_bound(self) -> float:
        """``mmx_tiled_q16_error_bound`` of the worst scale, relative to the value range (cached: the scale space is)."""
        if self._q16 is None:
            L = nat.lib()
            b = [float(L.mmx_tiled_q16_error_bound(nat.as_double_ptr(self.w0[s]), nat.as_double_ptr(self.w2[s]),
                                                   int(self.radii[s]), float(self.norms[s]))) for s in range(len(self.sigmas))]
            self._q16 = float("inf") if (not b or min(b) < 0) else max(b)
        return self._q16

    @classmethod
    def _make(cls, min_sigma: float, max_sigma: float, num_sigma: int) -> "ScaleSpace":
        if not (np.isscalar(min_sigma) and np.isscalar(max_sigma)):
            raise NotImplementedError("per-axis sigmas are not on the reference's path "
                                      "(detector.py:926-927 passes scalars)")
        sigmas, norms = k1.sigma_ladder(float(min_sigma), float(max_sigma), int(num_sigma))
        radii = np.array([k1.kernel_radius(s) for s in sigmas], dtype=np.int32)
        if radii.max(initial=0) > nat.MMX_MAX_RADIUS_GENERIC:
            raise nat.MmxError("sigma too large for the device kernels (radius > 255)")
        w0, w2 = [], []
        tab0 = np.zeros((len(sigmas), nat.MMX_MAX_RADIUS_GENERIC + 1))
        tab2 = np.zeros_like(tab0)
        for i, (s, r) in enumerate(zip(sigmas, radii)):
            if s <= 1e-15:
                raise NotImplementedError("sigma = 0 is not supported on the device path")
            a = k1.gaussian_half_kernel(float(s), 0, int(r))
            b = k1.gaussian_half_kernel(float(s), 2, int(r))
            w0.append(a)
            w2.append(b)
            tab0[i, :r + 1] = a
            tab2[i, :r + 1] = b
        return cls(sigmas, norms, radii, w0, w2, tab0, tab2)


_SPACES: Dict[tuple, ScaleSpace] = {}


@dataclass
class BatchStats:
    """Counters of one :func:`blob_log_blocks` call (also feeds bench.py)."""
    n_blocks: int = 0
    n_voxels: int = 0
    n_part_voxels: int = 0      # voxels the kernels processed: n_voxels, plus the halos of blocks detected in parts
    n_candidates: int = 0
    n_contested: int = 0
    n_probes: int = 0
    n_rescored: int = 0         # candidates re-scored in float64 because a decision needed it
    n_peaks: int = 0
    n_blobs: int = 0
    n_overlap_pairs: int = 0
    n_order_fallbacks: int = 0
    n_band_retries: int = 0       # batches nominated again because float32 strayed too far from float64
    max_f32_error: float = 0.0


#: debugging aid: cap on the blocks of one batch (``MMX_MAX_BATCH``; bisecting a batch-size dependent failure)
_MAX_BATCH = 1 << 30
_INTEGER_DTYPES = nat.voxel_dtypes(integer=True)      # raw voxels whose value range is the type's
#: the tail of the block list is re-split into batches that shrink by this factor (nothing hides the host work of the
#: last batches), the first batch into a ramp that starts at this many blocks (nothing hides its GPU time from the host)
TAPER = 4
RAMP = 16
#: blocks shorter than the largest kernel radius + ``MMX_COL_PREFETCH`` along an axis (a ragged stack's remainders) leave
#: the batches of the others -- one of them takes its whole batch off the fast kernels -- when the others hold more than
#: this many voxels (the taper's measure of real work); below it the plan is the one of all blocks together (a one-batch
#: stack keeps its single native call and its captured graph).  Tests set it to 0
THIN_SPLIT_MIN_VOXELS = 64 << 20
#: experiments only: cut the block list into batches of exactly these sizes (when they add up to the number of blocks)
FORCED_BATCH_SIZES: list = []
#: a block whose workspace slot (:func:`_slot_elems`) reaches this many elements is detected as several overlapping parts
#: (:func:`split_oversized`).  The library refuses such a slot itself, so a value above
#: ``LIB_MAX_SLOT_ELEMS`` counts as that; tests lower it
MAX_SLOT_ELEMS = 1 << 29
#: experiments and tests only: cut every oversized block into this ``(gz, gy, gx)`` grid instead of the smallest one (a
#: grid the search would never pick -- a cut that saves no padded row -- or the cost of a split on blocks that need none,
#: tools/partsbench.py); its boxes must still stay below the limit
FORCED_PART_GRID: Optional[Tuple[int, int, int]] = None


def _slot_limit() -> int:
    return slot_limit(MAX_SLOT_ELEMS)


def plan_batches(shapes: Sequence[Tuple[int, int, int]], num_sigma: int,
                 budget_bytes: int, extra_bytes_per_voxel: int = 0, *, thin_below: int = 0,
                 never_thin: Sequence[int] = ()) -> List[List[int]]:
    """:func:`batch_plan.plan_batches` with this module's settings: block indices grouped into batches whose workspace
    fits ``budget_bytes``, the blocks with an extent below ``thin_below`` in batches of their own behind the others."""
    return _bp.plan_batches(shapes, num_sigma, budget_bytes, extra_bytes_per_voxel, taper=TAPER, ramp=RAMP,
                            max_batch=_MAX_BATCH, forced_sizes=FORCED_BATCH_SIZES, thin_below=thin_below,
                            thin_min_voxels=THIN_SPLIT_MIN_VOXELS, never_thin=never_thin)


def _thin_below(lanes) -> int:
    """The extent below which a block is thin for this call: the largest kernel radius over the lanes +
    ``MMX_COL_PREFETCH`` (what the register-ring column kernels need).  0 -- no block is -- unless the mode is
    ``MMX_ZX_AUTO``: a mode asked for by name is passed as it is."""
    if ZX_MODE != nat.MMX_ZX_AUTO:
        return 0
    return max(int(lane.space.radii.max(initial=0)) for lane in lanes) + nat.col_prefetch()


def _split_blocks(lanes, shapes, limit: int) -> Dict[int, PartSplit]:
    """The splits of the blocks whose slot reaches ``limit``, by block index.  One split serves every lane: its halo is
    that of the widest ladder.  What a block in parts cannot go through raises ``NotImplementedError`` here."""
    big = np.nonzero(_slot_elems(np.asarray(shapes, dtype=np.int64).reshape(-1, 3)) >= limit)[0]
    if not len(big):
        return {}
    align = (1, 1, 1)
    for lane in lanes:
        pre = lane.pre
        if pre is None:
            continue
        from . import preprocess
        if isinstance(pre, preprocess.Rescaler) or getattr(pre, "rescale", None) is not None:
            raise NotImplementedError("a block too large for one workspace slot is detected in parts, which the "
                                      "isotropic rescale does not take; detect with a smaller segment_size")
        if isinstance(pre, preprocess.Unmixer):
            raise NotImplementedError("a block too large for one workspace slot is detected in parts, which spectral "
                                      "unmixing does not take; detect with a smaller segment_size")
        if not isinstance(pre, preprocess.Preprocessor):
            raise NotImplementedError(f"a block detected in parts cannot take its voxels from a {type(pre).__name__}")
        if pre.retains(lane.channel):
            raise NotImplementedError("a block too large for one workspace slot is detected in parts, which the "
                                      "intensity co-localisation (coloc=True) does not take; detect with a smaller "
                                      "segment_size")
        # (the parent is preprocessed WHOLE, tile by tile as ever, and its parts are boxes of that result: their faces
        #  need not lie on tile planes, so no alignment -- which a halo of half a block would not survive)
    halo = max(int(lane.space.radii.max(initial=0)) for lane in lanes) + 1
    return {int(i): split_oversized(shapes[int(i)], limit, halo, align, FORCED_PART_GRID) for i in big}


def _workspace(bufs, n_floats: int, which: int, split: Optional[PartSplit]):
    """``bufs.workspace`` -- and for a block in parts, whose workspace holds all of them at once, an error that says what
    was needed and what to do about it."""
    try:
        return bufs.workspace(n_floats, which)
    except torch.cuda.OutOfMemoryError as exc:
        if split is None:
            raise
        raise nat.MmxError(f"a block of {split.shape[0]} x {split.shape[1]} x {split.shape[2]} voxels is detected as "
                           f"{len(split)} parts in one batch, whose workspace needs {4 * int(n_floats)} bytes of device "
                           "memory that could not be allocated; detect with a smaller segment_size") from exc


def _workspace_floats(nb: int, slot: int, ns: int) -> int:
    """float32 elements of the workspace of a batch of ``nb`` blocks in slots of ``slot`` elements, ``ns`` scales."""
    return -(-int(nat.lib().mmx_workspace_bytes(nb, slot, ns, 1)) // 4)


_SELF_TESTED = set()


def self_test(dev) -> None:
    """Known-answer check of the matrix-core kernels, once per process and device (~30 ms): a small block tall
    enough for their steady-state loop through ``MMX_ZX_TILED`` and ``MMX_ZX_TILED_Q16`` (integer and float voxels,
    one radius per kernel geometry class) against the library's generic one-thread-per-voxel kernels -- and, at the
    radius that is longer than its 12 rows, through ``MMX_ZX_THIN`` (the folded Y pass).

    Why it exists: the exactness machinery compares float32 with float64 values AT THE CANDIDATES a batch
    nominates -- a kernel that is wrong everywhere nominates nothing and the batch comes back empty without an
    error.  That happened during development (an inline-assembly instruction behind an MFMA that still read its
    destination register: zeros for radius <= 8); the parity tests caught it, and this makes a production process
    fail as loudly should a compiler or driver ever produce it again."""
    key = str(dev)
    if key in _SELF_TESTED:
        return
    L = nat.lib()
    rng = np.random.default_rng(1234)
    vol = rng.integers(0, 65536, (70, 12, 80)).astype(np.uint16)
    vol[20:50, 3:9, 30:60] //= 16
    shape = vol.shape
    for dtype in (np.uint16, np.float32):
        dv = DeviceVolume(vol if dtype == np.uint16 else (vol.astype(np.float32) / np.float32(65535.0)), dev)
        blocks, slot = _make_blocks(dv, 0, [(0, 0, 0)], [shape])
        d_blocks = _to_device_bytes(blocks, dev)
        v32 = dv.view(0, True)
        v32.value_range = 1.0 if dtype == np.float32 else 0.0
        ws = torch.zeros(6 * slot, dtype=torch.float32, device=dev)
        for sigma in (1.6, 3.2, 4.6):                      # radii 6, 13, 18: the three kernel geometry classes
            space = ScaleSpace.make(sigma, sigma, 1)
            args = (ctypes.byref(v32), d_blocks.data_ptr(), blocks.ctypes.data, 1, slot, nat.as_double_ptr(space.w0[0]),
                    nat.as_double_ptr(space.w2[0]), int(space.radii[0]), float(space.norms[0]))
            nat.check(L.mmx_log_batch_f32_generic(*args, ws.data_ptr() + 5 * slot * 4, ws.data_ptr(), _stream_ptr()),
                      "mmx_log_batch_f32_generic")
            want = ws[5 * slot:6 * slot].clone()
            for mode, tol in ((nat.MMX_ZX_TILED, 2e-6), (nat.MMX_ZX_TILED_Q16, 6e-5), (nat.MMX_ZX_THIN, 2e-6)):
                path = ctypes.c_int(0)
                nat.check(L.mmx_log_batch_f32(*args, ws.data_ptr() + 4 * slot * 4, ws.data_ptr(), None, 0.0, 0.0, None,
                                              mode, ctypes.byref(path), _stream_ptr()), "mmx_log_batch_f32")
                got = ws[4 * slot:5 * slot]
                n = shape[0] * shape[1] * int(blocks["px"][0])
                g = got[:n].view(shape[0], shape[1], -1)[..., :shape[2]]
                w = want[:n].view(shape[0], shape[1], -1)[..., :shape[2]]
                err = float((g - w).abs().max().item())
                if path.value == mode and not err < tol:
                    raise nat.MmxError(f"self-test of the device kernels failed (zx_mode {mode}, radius "
                                       f"{int(space.radii[0])}, {np.dtype(dtype).name} voxels: off by {err:.3g}); "
                                       "this build of libmmx_hip.so must not be used")
    _SELF_TESTED.add(key)


def log_cube_blocks(dvol: DeviceVolume, channel: int, origins, shapes, space: ScaleSpace,
                    generic: bool = False, value_range: float = 0.0) -> List[np.ndarray]:
    """Float32 ``(z, y, x, sigma)`` cubes of the given blocks (A0-A3 only; used by tests
    for the 1e-4 LoG tolerance and by the profiling scripts).  ``value_range``: what the caller knows about float
    voxels (``mmx_volume.value_range``: > 0 = values in [0, m], < 0 = |v| <= m, 0 = unknown), which decides whether
    they may take the tiled matrix-core kernels."""
    dvol.wait_all()
    dev = dvol.tensor.device
    L = nat.lib()
    blocks, slot = _make_blocks(dvol, channel, origins, shapes)
    nb, ns = len(blocks), len(space.sigmas)
    ws = torch.empty((4 + ns) * nb * slot, dtype=torch.float32, device=dev)
    d_blocks = _to_device_bytes(blocks, dev)
    vol32 = dvol.view(channel, True)
    if vol32.dtype == nat.MMX_F32:
        vol32.value_range = float(value_range)
    fn = L.mmx_log_batch_f32_generic if generic else L.mmx_log_batch_f32
    log_base = ws.data_ptr() + 4 * nb * slot * 4
    global LAST_ZX_PATH
    path = ctypes.c_int(0)
    for s in range(ns):
        nat.check(fn(ctypes.byref(vol32), d_blocks.data_ptr(), blocks.ctypes.data, nb, slot,
                     nat.as_double_ptr(space.w0[s]), nat.as_double_ptr(space.w2[s]),
                     int(space.radii[s]), float(space.norms[s]),
                     log_base + s * nb * slot * 4, ws.data_ptr(),
                     *(() if generic else (None, 0.0, 0.0, None, ZX_MODE | ZX_FLAGS if ZX_MODE >= 0 else ZX_MODE, ctypes.byref(path))),
                     _stream_ptr()), "mmx_log_batch_f32")
        LAST_ZX_PATH = None if generic else path.value
    torch.cuda.synchronize()
    logs = ws[4 * nb * slot:].view(ns, nb, slot).cpu().numpy()
    out = []
    for i, shp in enumerate(shapes):
        px = int(blocks["px"][i])
        n = int(shp[0]) * int(shp[1]) * px
        cube = logs[:, i, :n].reshape((ns, shp[0], shp[1], px))[..., :shp[2]]
        out.append(np.moveaxis(cube, 0, -1).copy())
    return out


def _make_blocks(dvol: DeviceVolume, channel: int, origins, shapes):
    """``mmx_block`` records of one batch (block i owns slot i) and the workspace slot size they need."""
    o = _held_origins(dvol, origins, shapes)
    return block_records(o @ np.asarray(dvol.tensor.stride()[:3], dtype=np.int64), shapes)


def _held_origins(dvol: DeviceVolume, origins, shapes) -> np.ndarray:
    """``origins`` as an ``(n, 3)`` array, once the blocks are known to lie in what ``dvol`` holds."""
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 3)
    shp = np.asarray(shapes, dtype=np.int64).reshape(-1, 3)
    if (o < 0).any() or (shp < 1).any() or (o + shp > np.asarray(dvol.shape[:3], dtype=np.int64)).any():
        raise ValueError("block outside the volume")
    held_lo = np.array([dvol.z_off, dvol.y_off, 0], dtype=np.int64)
    if (o < held_lo).any() or (o[:, :2] + shp[:, :2] > held_lo[:2] + np.asarray(dvol.tensor.shape[:2], dtype=np.int64)).any():
        raise ValueError("block outside the planes and rows this volume holds")
    return o


def blob_log_blocks(dvol: DeviceVolume, channel: int, origins: Sequence[Sequence[int]],
                    shapes: Sequence[Sequence[int]], min_sigma: float, max_sigma: float,
                    num_sigma: int, threshold: float, overlap: float, *,
                    budget_bytes: Optional[int] = None, stats: Optional[BatchStats] = None,
                    return_peaks: bool = False, on_batch=None, pre=None,
                    exact_values: Optional[bool] = None, sink=None, finisher=None, plan_num_sigma: Optional[int] = None):
    """``blob_log`` of every block -> list of ``(n, 4)`` float64 ``[z, y, x, sigma]`` arrays.

    ``exact_values`` (default True): re-score EVERY candidate in float64 in the batch's own kernel queue, so
    that the peak values are the reference's bit for bit.  ``False`` re-scores only the candidates whose
    decision needs it (see ``_resolve_peaks``) -- fewer points, but as a second, host-synchronous launch
    per batch: on the benchmark volume, whose blobs are all alike, 68 % of the candidates have a block mate
    within eps and the step is slower (243 vs 227 ms); it pays on images with a wide intensity range.

    Each block is an independent image exactly as each reference worker's sub-ROI is
    (reference magmap/cv/stack_detect.py:79): reflect boundaries at the block faces,
    coordinates relative to the block.  Blocks without blobs give ``np.empty((0, 3))`` like
    scikit-image does (blob.py:516-517).  Row order equals the reference's.
    ``on_batch(indices, results)`` is called as each batch finishes, while the GPU is busy
    with the next one.  ``pre`` (a ``preprocess.Preprocessor``) saturates + denoises every block
    on the device first (reference stack_detect.py:122-150); detection then runs on the
    float64 result exactly as the reference's ``blob_log`` does.
    ``sink(indices, peak_batch)`` (native host path only) takes each batch as a :class:`PeakBatch` -- rows, ``alive``
    flags, block offsets -- instead of per-block arrays; the call then returns ``None`` entries for those blocks.
    ``finisher(indices, cands, n_cands, blocks, space, thr, eps, overlap, stats) -> bool`` (native host path, only when
    ALL blocks are one batch): takes the batch's re-scored candidate table and does everything behind it itself
    (``stack_detect._StackFinisher``: one native call up to the stack's final table); ``False``: it left the batch to
    the usual steps.
    """
    lane = Lane(channel, min_sigma, max_sigma, num_sigma, threshold, overlap, stats=stats, on_batch=on_batch, pre=pre,
                exact_values=exact_values, sink=sink, finisher=finisher)
    out = blob_log_lanes(dvol, [lane], origins, shapes, budget_bytes=budget_bytes, return_peaks=return_peaks,
                         plan_num_sigma=plan_num_sigma)
    return (out[0][0], out[1][0]) if return_peaks else out[0]


class Lane:
    """One detection over the blocks of a volume -- a channel with its scales, threshold, preprocessing and the callbacks
    that take its batches (the arguments of :func:`blob_log_blocks`); :func:`blob_log_lanes` runs several of them over the
    same blocks in ONE pipeline."""

    def __init__(self, channel: int, min_sigma: float, max_sigma: float, num_sigma: int, threshold: float, overlap: float,
                 *, stats: Optional[BatchStats] = None, on_batch=None, pre=None, exact_values: Optional[bool] = None,
                 sink=None, finisher=None):
        self.channel, self.threshold, self.overlap = channel, float(threshold), float(overlap)
        from . import host_resolve as _hr
        if _hr.PEAK_ORDER == "0.19+" and self.threshold < 0:
            raise NotImplementedError("PEAK_ORDER '0.19+' pads the peak mask with 'nearest': identical to the zero padding "
                                      "of this path for thresholds >= 0 only")
        self.space = ScaleSpace.make(min_sigma, max_sigma, num_sigma)
        self.stats = stats if stats is not None else BatchStats()
        self.on_batch, self.pre, self.sink, self.finisher = on_batch, pre, sink, finisher
        self.exact = bool(True if exact_values is None else exact_values)
        self.results: list = []
        self.peaks_out: list = []

    def bind(self, dvol: DeviceVolume, n_blocks: int) -> None:
        """What follows from the volume: value scale, nomination band, value range, the weight tables on its device."""
        space, pre, channel = self.space, self.pre, self.channel
        self.results = [None] * n_blocks
        self.peaks_out = [None] * n_blocks
        self.vscale = float(dvol.value_scale() if pre is None else pre.value_scale([channel]))
        eps = EPS_REL * self.vscale
        # what is known about the voxels the passes will read: raw integer images [0, 1]; float images their measured
        # range; preprocessed / unmixed / rescaled blocks the bounds their arithmetic implies
        self.vrange = vrange = dvol.value_range(channel) if pre is None else pre.value_range([channel])
        integer_voxels = pre is None and dvol.np_dtype in _INTEGER_DTYPES
        # (raw int16: [-1, 1], which the tiled kernels carry as [0, 2] less a constant per scale -- a value SPAN of 2,
        #  twice the rounding error of the 16-bit intermediates; the wide band is taken only where it still covers that
        #  fourfold, as the library's own rule asks, else the batch keeps float32 tiles and the narrow band)
        signed_raw = integer_voxels and dvol.np_dtype.kind == "i"
        span = 2.0 if signed_raw else 1.0
        # volumes whose voxels are known to be non-negative and of ordinary magnitude take 16-bit intermediates: the
        # band must cover their rounding error fourfold
        # -- and their error in value units must stay inside the LoG contract (a profile whose unsharp / clip settings
        # stretch the preprocessed range past ~3.4 keeps float32 intermediates and the narrow band)
        if (vrange is not None and (vrange[0] >= 0.0 or signed_raw) and vrange[1] <= FLOAT_TILED_RANGE[1]
                and EPS_REL_Q16 > EPS_REL and ZX_MODE in (nat.MMX_ZX_AUTO, nat.MMX_ZX_TILED_Q16)
                and (ZX_MODE == nat.MMX_ZX_TILED_Q16 or space.q16_bound() * (vrange[1] if not integer_voxels else span)
                     <= LOG_ABS_TOL)
                and (not signed_raw or 4.0 * space.q16_bound() * span <= EPS_REL_Q16 * self.vscale)):
            eps = EPS_REL_Q16 * self.vscale
        self.eps = eps
        self.d_w0, self.d_w2 = space.device_tables(dvol.tensor.device)


#: workspace budget per batch of a call that does not say (``budget_bytes=None``); bench.py sets it from the free HBM
BUDGET_BYTES = 24 << 30
#: several channels of a stack in one pipeline, batch-major (both channels of a batch of blocks before the next batch):
#: "uploading" (default) = while the volume is still on its way to the device -- a host tile is then needed layer by
#: layer by all channels instead of whole by the first (one C5 tile from the host: 240 against 285 ms); True = always;
#: False = never: the channels one after the other, each through all its batches.  For a RESIDENT volume the two orders
#: cost the same on average (213-217 ms per C5 step) but batch-major scatters more (p95 / p50 1.08 against 1.02; as a
#: sub-record behind other workloads 232-254 against 223-225): profiles/r06_experiments.txt section 7
BATCH_MAJOR = "uploading"


class _BlockLists(NamedTuple):
    """The block lists of a call as given, their checked copies, content key and largest slot (``_Buffers.plan_lists``)."""
    given: tuple                # (origins, shapes) as passed -- kept alive: their ids stay theirs
    key: tuple
    origins: list
    shapes: list
    slot_max: int


def _block_lists(bufs: _Buffers, origins, shapes) -> _BlockLists:
    """The very same tuple objects step after step (stack_detect hands over its cached block lists): their checked copies
    and their content key are remembered -- converting and hashing 256 blocks is 0.3 ms before the first launch.
    (tuples only: a list could have been edited in place since)"""
    immutable = type(origins) is tuple and type(shapes) is tuple
    seen = bufs.plan_lists.get((id(origins), id(shapes))) if immutable else None
    if seen is not None and seen.given[0] is origins and seen.given[1] is shapes:
        return seen
    given = (origins, shapes)
    shapes = [tuple(int(v) for v in s) for s in shapes]
    origins = [tuple(int(v) for v in o) for o in origins]
    slot_max = int(_slot_elems(np.asarray(shapes, dtype=np.int64).reshape(-1, 3)).max()) if shapes else 0
    lists = _BlockLists(given, (tuple(origins), tuple(shapes)), origins, shapes, slot_max)
    if immutable:
        if len(bufs.plan_lists) >= 8:
            bufs.plan_lists.clear()
        bufs.plan_lists[(id(given[0]), id(given[1]))] = lists
    return lists


def _plan_for(dvol: DeviceVolume, lanes, lists: _BlockLists, bufs: _Buffers, ns: int, budget_bytes: int) -> BatchPlan:
    """The batches of the call, planned for ``ns`` scales.  Raw lanes with no block in parts: remembered in
    ``bufs.plans`` for the same block lists, volume layout and budget (a stack detected step after step) -- a
    millisecond of planning, record building and upload per step otherwise, before the first kernel can start."""
    pre = lanes[0].pre is not None
    # blocks too large for one workspace slot go through as several overlapping parts, each in a batch of its own
    # (DESIGN.md section 4f); without one -- nearly every call -- nothing takes another path
    splits = _split_blocks(lanes, lists.shapes, _slot_limit()) if lists.slot_max >= _slot_limit() else {}
    thin_below = _thin_below(lanes)
    key = None
    if not pre and not splits:
        t_ = dvol.tensor
        # (block records hold element offsets, not addresses: any volume of this layout can use them; the block lists
        #  are compared by content -- `lists.key` -- so that a caller who builds them afresh finds the same device
        #  tables, which is also what lets a small batch's captured graph be found again)
        key = (lists.key, tuple(t_.stride()), tuple(t_.shape), str(t_.dtype), ns, int(budget_bytes), _MAX_BATCH, RAMP, TAPER,
               thin_below, THIN_SPLIT_MIN_VOXELS)
        hit = bufs.plans.get(key)
        if hit is not None:
            return hit
    batches = plan_batches(lists.shapes, ns, budget_bytes,
                           0 if not pre else max(lane.pre.bytes_per_voxel() for lane in lanes), thin_below=thin_below,
                           never_thin=sorted(splits))
    if splits:
        batches = _isolate_parents(batches, splits)
    # (raw lanes: the records of every batch but a block in parts are made here, for `_upload_records`)
    if not pre:
        _held_origins(dvol, lists.origins, lists.shapes)
    plan = _bp.make_plan(lists.origins, lists.shapes, batches, splits, None if pre else dvol.tensor.stride()[:3],
                         thin_below)
    if key is not None:
        if len(bufs.plans) >= 8:
            bufs.plans.clear()
        bufs.plans[key] = plan
    return plan


def _upload_records(plan: BatchPlan, dev) -> None:
    """The block tables of every batch that has one go to the device BEFORE the first kernel (a pageable host -> device
    copy waits for everything queued on the stream before it), in ONE upload: fourteen small copies were 0.4 ms of idle
    GPU at the start of a step.  A plan that comes from ``bufs.plans`` has them already."""
    ready = [b for b in plan.batches if b.records is not None and b.d_records is None]
    if not ready:
        return
    table = _to_device_bytes(np.concatenate([b.records.view(np.uint8).reshape(-1) for b in ready]), dev)
    at = 0
    for b in ready:
        b.d_records = table[at:at + b.records.nbytes]
        at += b.records.nbytes


def _size_workspaces(bufs: _Buffers, plan: BatchPlan, ns: int, two: bool) -> None:
    """Raw lanes: the shared workspace has its final size before anything is queued on it -- workspace 0 for every
    batch, and with ``two`` workspace 1 for the batches that alternate (a block in parts works in workspace 0 alone)."""
    if not plan.batches:
        return
    need = [_workspace_floats(b.n_blocks, b.slot, ns) for b in plan.batches]
    _workspace(bufs, max(need), 0, max((b.split for b in plan.batches if b.split is not None), key=len, default=None))
    if two and not all(b.split is not None for b in plan.batches):
        bufs.workspace(max(n for n, b in zip(need, plan.batches) if b.split is None), 1)
    bufs.ws_free = [None, None]


def blob_log_lanes(dvol: DeviceVolume, lanes: Sequence[Lane], origins: Sequence[Sequence[int]],
                   shapes: Sequence[Sequence[int]], *, budget_bytes: Optional[int] = None, return_peaks: bool = False,
                   plan_num_sigma: Optional[int] = None):
    """:func:`blob_log_blocks` for several lanes (channels) over the SAME blocks in one pipeline, batch-major: the
    batches are planned once, and batch b goes through lane 0, lane 1, ... before batch b + 1 -- one queue of launches
    for the whole call (no drain between channels), a block's tables of every channel complete together (so that a stack's
    rows land, and its regions are pruned, from the first batches on), and a host tile still on its way up is needed
    layer by layer by ALL channels instead of whole by the first.  All lanes preprocess or none does.
    ``plan_num_sigma``: plan the batches as for this many scales (calls for the channels of one stack made one after
    the other cut the blocks into the SAME batches that way, whatever each channel's own number of scales).
    Returns ``[lane results]`` (and ``[lane peaks]`` with ``return_peaks``)."""
    _require_gpu()
    budget_bytes = int(BUDGET_BYTES if budget_bytes is None else budget_bytes)
    lanes = list(lanes)
    if not lanes:
        return ([], []) if return_peaks else []
    if len({lane.pre is None for lane in lanes}) > 1:
        raise ValueError("lanes of one pipeline either all preprocess their blocks or none does")
    any_pre = lanes[0].pre is not None
    bufs = _buffers_for(dvol.tensor.device)
    lists = _block_lists(bufs, origins, shapes)
    origins, shapes = lists.origins, lists.shapes
    for lane in lanes:
        lane.bind(dvol, len(shapes))
    ns_max = max([len(lane.space.sigmas) for lane in lanes] + [int(plan_num_sigma or 0)])
    plan = _plan_for(dvol, lanes, lists, bufs, ns_max, budget_bytes)
    n_l = len(lanes)
    items = [(b, l) for b in plan.batches for l in range(n_l)]       # batch-major
    n_items = len(items)
    # How far the GPU queue runs ahead of the host.  Raw volumes: EVERY batch is enqueued before the host looks at
    # the first result, so the GPU runs the batches back to back whatever the host is doing (measured: enqueueing
    # batch k + 1 only after the host work of batch k - 1 left the GPU idle ~4 ms per batch once the host work of
    # a batch outlasted the kernels of the next).  Each batch in flight owns a candidate table; the workspace is
    # shared (stream order).  With preprocessing the float64 tiles are double-buffered, so one batch ahead.
    ahead = n_items if not any_pre else PRE_AHEAD
    if any_pre and all(getattr(lane.pre, "retains", lambda c: False)(lane.channel) for lane in lanes):
        # every lane's preprocessed blocks have slots of their own (Preprocessor.retain: the co-localisation's): no buffer
        # set limits how far the queue may run ahead -- and with several lanes PRE_AHEAD items are less than PRE_AHEAD
        # batches
        ahead = max(ahead, min(n_items, PRE_AHEAD_RETAINED * n_l))
    bufs.slots(ahead + 1)
    if not any_pre:
        _upload_records(plan, dvol.tensor.device)
        _size_workspaces(bufs, plan, ns_max, bool(RESCORE_STREAM and n_items > 1))
    jobs: List[Optional[_Batch]] = [None] * n_items
    done_events: List = []
    enq = 0
    uploading = dvol._upload is not None
    for k, (_, l_k) in enumerate(items):
        while enq < min(n_items, k + 1 + ahead):       # item k itself and `ahead` items behind it
            planned, ln = items[enq][0], lanes[items[enq][1]]
            batch = planned.indices
            if uploading and enq > k and not dvol.upload_ready(
                    [(origins[i][0], origins[i][0] + shapes[i][0], origins[i][1], origins[i][1] + shapes[i][1]) for i in batch]):
                # a volume still on its way up: this batch's voxels have not been queued for copying yet.  Enqueueing it
                # would block the host until they are -- with finished batches waiting for their host work (all of it
                # then piled up behind the upload's last region: 30 ms at the end of a from-host step).  Item k first.
                break
            # (preprocessing: when the buffer set's previous holder is done; the first holders behind the main stream)
            pipe = _Pipelined(planned, enq & 1, None if enq < ahead + 1 else done_events[enq - (ahead + 1)])
            jobs[enq] = _enqueue_detect(dvol, ln, [origins[i] for i in batch], [shapes[i] for i in batch], bufs,
                                        enq % (ahead + 1), pipe=pipe, split=planned.split, zx_mode=planned.zx_mode)
            done_events.append(jobs[enq].done)
            jobs[enq].indices = batch
            if enq == 0:
                global FIRST_ENQUEUED_T, LAST_BATCH_SIZES
                FIRST_ENQUEUED_T, LAST_BATCH_SIZES = time.perf_counter(), [len(b_.indices) for b_ in plan.batches]
            enq += 1
        pending, jobs[k] = jobs[k], None
        ln = lanes[l_k]
        # host + side-stream work of item k, the GPU busy with the items behind it
        peaks = _finish_detect(pending, dvol, bufs, ln.finisher if n_items == 1 else None)
        if peaks is _FINISHED:
            continue
        if isinstance(peaks, PeakBatch):
            pb = _prune_batch_native(peaks, ln.space, ln.overlap, ln.stats)
            if ln.sink is not None:        # the caller builds its tables from the arrays (native, no per-block lists)
                with torch.cuda.stream(bufs.side):      # (whatever it launches -- co-localisation means -- beside the next batch)
                    ln.sink(pending.indices, pb)
                continue
            pruned = [pb.blobs(b) for b in range(len(pb))]
            peaks = [pb.block(b) for b in range(len(pb))] if return_peaks else [None] * len(pb)
        else:
            with torch.cuda.stream(bufs.side):
                pruned = _prune_batch(peaks, ln.space, ln.overlap, dvol.tensor.device, ln.stats)
        for i, pk, res in zip(pending.indices, peaks, pruned):
            ln.results[i] = res
            ln.peaks_out[i] = pk
        if ln.on_batch is not None:    # caller's per-block post-processing, still overlapped: whatever it launches
            with torch.cuda.stream(bufs.side):           # (co-localisation means) runs beside the next batch's kernels
                ln.on_batch(pending.indices, pruned)
    results = [ln.results for ln in lanes]
    return (results, [ln.peaks_out for ln in lanes]) if return_peaks else results


# --------------------------------------------------------------------------- A0-A4
@dataclass
class _Batch:
    """One batch in flight: what :func:`_enqueue_detect` hands to :func:`_finish_detect` (and to :func:`_redo`)."""
    lane: "Lane"
    origins: list
    shapes: list
    blocks: np.ndarray
    d_blocks: "torch.Tensor"
    nb: int
    ns: int
    n_vox: int
    cap: int
    which: int                  # the slot of `bufs` (candidate table, counters, events) it owns
    done: _NativeEvent
    store_f32: int
    vol_exact: object           # the `mmx_volume` record of the voxels the exact re-score reads
    eps: float
    exact: bool
    native: bool
    indices: Optional[list] = None      # its blocks' places in the call's block lists (the pipeline's)
    retries: int = 0                    # times it has been nominated again with a wider band
    # a block detected in parts (`origins` / `shapes` hold that one block, the PARENT; `blocks` / `nb` its parts): the
    # split, the parent table -- what everything behind the fold works on -- and the voxels of the parts
    split: Optional[PartSplit] = None
    parents: Optional[np.ndarray] = None
    d_parents: Optional["torch.Tensor"] = None
    d_parts: Optional["torch.Tensor"] = None
    n_part_vox: int = 0
    zx_mode: Optional[int] = None       # the mode its plan asks for (`PlannedBatch.zx_mode`)
    block_f32: object = None            # `_Voxels.block_f32`, alive until the batch is finished

    @property
    def table_blocks(self) -> np.ndarray:
        """The blocks the finished candidate table speaks of."""
        return self.blocks if self.split is None else self.parents

    @property
    def d_table_blocks(self):
        return self.d_blocks if self.split is None else self.d_parents


@dataclass
class _Pipelined:
    """What the pipeline of :func:`blob_log_lanes` tells :func:`_enqueue_detect` about a batch it enqueues ahead."""
    planned: PlannedBatch
    workspace: int              # which of the two workspaces a raw batch with a side tail works in
    pre_after: object = None    # preprocessing lanes: the event its buffer set is free at; None: behind the main stream


@dataclass
class _Voxels:
    """The voxels of a batch as the library reads them (:func:`_batch_voxels`)."""
    blocks: np.ndarray
    slot: int
    d_blocks: object            # the uploaded ``blocks``, or None: not uploaded yet
    parents: Optional[np.ndarray]       # a block in parts: its own record (``blocks`` are its parts)
    vol32: object               # the ``mmx_volume`` records the passes / the exact re-score read
    vol_exact: object
    store_f32: int
    block_f32: object = None    # preprocessed blocks of a float32 image: the device flag per block (1 = a float32 block)


def _preprocess(dvol, lane: "Lane", origins, shapes, bufs: _Buffers, which: int, boxes, pipe: Optional[_Pipelined]):
    """Enqueue P1-P3 of a batch -> ``(blocks, slot, vol32, vol_exact)``.  Pipelined with ``PRE_STREAM``: on a stream of
    its own, where it may start as soon as the batch that last used this buffer set is done (``pipe.pre_after``: that
    batch's completion event), i.e. while the batch before this one is still filtering.  (None: a buffer set no batch of
    this call has used yet -- behind whatever is queued on the main stream.  Letting the first batches' preprocessing
    start at once instead measured nothing on C3 --denoise 25 and +10 ms on C5, round 5.)"""
    if not (PRE_STREAM and pipe is not None):
        dvol.stream_wait(None, [torch.cuda.current_stream(), bufs.side], boxes)
        return lane.pre.run(dvol, lane.channel, origins, shapes, which)
    main = torch.cuda.current_stream()
    bufs.pre_stream.wait_stream(main) if pipe.pre_after is None else _stream_wait(bufs.pre_stream, pipe.pre_after)
    with torch.cuda.stream(bufs.pre_stream):
        dvol.stream_wait(None, [torch.cuda.current_stream(), bufs.side], boxes)     # (side: co-localisation means)
        out = lane.pre.run(dvol, lane.channel, origins, shapes, which)
        ready = torch.cuda.Event()
        ready.record()
    timed = bool(nat.lib().mmx_timing_is_enabled())
    if timed:       # how long the LoG stream waits for this batch's preprocessing (bench.py: pre_stream_wait_ms)
        before = torch.cuda.Event(enable_timing=True)
        before.record()
    main.wait_event(ready)
    if timed:
        after = torch.cuda.Event(enable_timing=True)
        after.record()
        PRE_WAITS.append((before, after))
    return out


def _batch_voxels(dvol, lane: "Lane", origins, shapes, bufs: _Buffers, which: int, split: Optional[PartSplit],
                  pipe: Optional[_Pipelined]) -> _Voxels:
    """The voxels of the batch, raw or preprocessed (enqueued here), as the parts of ``split`` where there is one."""
    channel, pre = lane.channel, lane.pre
    # a volume still on its way up (`DeviceVolume.stream_wait`): this batch waits for the slabs its blocks touch, on
    # every stream that reads voxels (the passes, the voxel copy of the tiled path, the exact re-score)
    boxes = ([(int(o[0]), int(o[0]) + int(s_[0]), int(o[1]), int(o[1]) + int(s_[1])) for o, s_ in zip(origins, shapes)]
             if dvol._upload is not None else None)
    d_blocks = None
    block_f32 = None
    if pre is None:
        if dvol._upload is not None:
            dvol.stream_wait(None, [torch.cuda.current_stream(), bufs.pack_stream, bufs.rescore_stream, bufs.side], boxes)
        if pipe is not None and pipe.planned.records is not None:
            blocks, slot, d_blocks = pipe.planned.records, pipe.planned.slot, pipe.planned.d_records
        else:
            blocks, slot = _make_blocks(dvol, channel, origins, shapes)
        vol32, vol_exact = dvol.view(channel, True), dvol.view(channel, False)
        store_f32 = 1 if dvol.np_dtype == np.float32 else 0
        strides = dvol.tensor.stride()[:3]
    else:
        blocks, slot, vol32, vol_exact = _preprocess(dvol, lane, origins, shapes, bufs, which, boxes, pipe)
        store_f32 = int(getattr(pre, "store_f32", 0))
        # a float32 image (preprocess.FLOAT32_RULES): float32 and float64 blocks in one batch, told apart on the device
        block_f32 = getattr(pre, "block_flags", None)
        # (a block in parts was preprocessed whole, tile by tile as ever: its parts are boxes of that slot -- same
        #  strides -- and the exact re-score reads the slot with the parent's extent)
        strides = (vol32.stride_z, vol32.stride_y, vol32.stride_x)
    parents = None
    if split is not None:
        parents = blocks
        blocks, slot = split.block_records(parents["src_off"][0], strides)
    return _Voxels(blocks, slot, d_blocks, parents, vol32, vol_exact, store_f32, block_f32)


def _detect_args(lane: "Lane", vox: _Voxels, bufs: _Buffers, which: int, ws, ws_i: int, cap: int, eps: float, exact: bool,
                 native: bool, side_tail: bool, zx_mode: Optional[int] = None) -> "nat.DetectArgs":
    """The ``mmx_detect_args`` of a batch whose voxels, workspace and table slot are settled.  ``zx_mode``: the mode
    the batch's plan asks for, which holds under ``MMX_ZX_AUTO`` only."""
    space, stream = lane.space, _stream_ptr()
    ev_read, ev_done = bufs.events(which)
    a = nat.DetectArgs()
    a.vol32, a.vol_exact = ctypes.pointer(vox.vol32), ctypes.pointer(vox.vol_exact)
    a.d_blocks, a.h_blocks = vox.d_blocks.data_ptr(), vox.blocks.ctypes.data
    a.n_blocks, a.n_sigma, a.slot_elems = len(vox.blocks), len(space.sigmas), vox.slot
    a.h_w0, a.h_w2 = space.w0_tab.ctypes.data, space.w2_tab.ctypes.data
    a.d_w0, a.d_w2 = lane.d_w0.data_ptr(), lane.d_w2.data_ptr()
    a.h_radius, a.h_norm = space.radii.ctypes.data, space.norms.ctypes.data
    a.d_work, a.work_bytes = ws.data_ptr(), ws.numel() * 4
    a.thr, a.eps = lane.threshold, eps
    a.d_cands, a.cap, a.d_count = bufs.cand_table(which, cap).data_ptr(), cap, bufs.counts[which].data_ptr()
    a.h_count = bufs.host_counts[which].data_ptr()
    if native:
        a.h_cands, a.h_prefix = bufs.host_table(which).data_ptr(), min(cap, _PREFIX_ENTRIES)
    a.zx_mode = ZX_MODE if (zx_mode is None or ZX_MODE != nat.MMX_ZX_AUTO) else zx_mode
    a.zx_flags, a.store_f32, a.exact, a.expand = ZX_FLAGS, vox.store_f32, int(exact), int(native)
    if vox.block_f32 is not None:
        a.d_block_f32 = vox.block_f32.data_ptr()
    a.stream = a.pack_stream = stream
    a.tail_stream = bufs.rescore_stream.cuda_stream if side_tail else stream      # (the library forks and joins it)
    # (the last reader of this workspace; also a batch that is nominated again, on the main stream: same workspace)
    a.ev_work_free = bufs.ws_free[ws_i].handle if bufs.ws_free[ws_i] is not None else None
    a.ev_work_read = ev_read.handle if side_tail else None
    a.ev_done = ev_done.handle
    return a


def _enqueue_detect(dvol, lane: "Lane", origins, shapes, bufs: _Buffers, which: int, *, cap: Optional[int] = None,
                    eps: Optional[float] = None, exact: Optional[bool] = None, split: Optional[PartSplit] = None,
                    pipe: Optional[_Pipelined] = None, zx_mode: Optional[int] = None) -> _Batch:
    """Enqueue (P1-P3,) A0-A4 of one batch of ``lane`` on the current stream: the preprocessing, then ONE
    ``mmx_detect_batch`` call (or the replay of its captured graph); nothing here waits for the GPU.
    ``eps`` / ``exact`` (default: the lane's): the nomination band, and whether every candidate is also re-scored in
    float64 (otherwise ``_resolve_peaks`` re-scores the few whose decision depends on it).
    ``split``: ``origins`` / ``shapes`` hold ONE block, which goes through the passes and the NMS as the parts of this
    split; the library folds their candidates back into it (``mmx_fold_parts``) and everything behind sees that block.
    ``zx_mode``: the mode the batch's plan asks for (``PlannedBatch.zx_mode``; every path below passes it on).
    ``pipe``: the batch's place in the pipeline of :func:`blob_log_lanes`.  Without it the block records are made here,
    the batch works in workspace 0 with no side tail, and its preprocessing runs on the main stream."""
    space, pre, vrange = lane.space, lane.pre, lane.vrange
    eps = lane.eps if eps is None else eps
    exact = lane.exact if exact is None else exact
    L = nat.lib()
    dev = dvol.tensor.device
    if split is not None and (len(shapes) != 1 or tuple(int(v) for v in shapes[0]) != split.shape):
        raise ValueError("a split belongs to the one block of its batch")
    vox = _batch_voxels(dvol, lane, origins, shapes, bufs, which, split, pipe)
    blocks, vol32 = vox.blocks, vox.vol32
    nb, ns = len(blocks), len(space.sigmas)
    if vox.slot >= _slot_limit():
        raise nat.MmxError(slot_refusal(_slot_limit()))
    # raw volumes: the pipeline's batches alternate between two workspaces, and everything after a batch's last LoG
    # kernel -- NMS, probe expansion, exact re-score, copies -- runs on a second stream beside the next batch's LoG
    # kernels (never a block in parts, whose records the pipeline does not hold)
    side_tail = bool(RESCORE_STREAM and exact and pre is None and pipe is not None and pipe.planned.records is not None)
    ws_i = pipe.workspace if (side_tail and bufs.ws2 is not None) else 0
    ws = _workspace(bufs, _workspace_floats(nb, vox.slot, ns), ws_i, split)
    if vox.d_blocks is None:
        vox.d_blocks = _to_device_bytes(blocks, dev)
    if vol32.dtype == nat.MMX_F32:
        # float voxels (float images, preprocessed blocks): the tiled path holds each as two float16 pieces, which
        # suits values of ordinary magnitude -- the range is known here, not in the library (mmx_volume.value_range)
        float_ok = vrange is not None and max(abs(vrange[0]), abs(vrange[1])) <= FLOAT_TILED_RANGE[1]
        vol32.value_range = 0.0 if not float_ok else (max(vrange[1], 1e-30) if vrange[0] >= 0.0
                                                      else -max(abs(vrange[0]), abs(vrange[1])))
    n_vox = int(sum(int(np.prod(s)) for s in shapes))
    n_part_vox = n_vox if split is None else int(split.box_shapes.prod(axis=1).sum())       # (what the NMS nominates from)
    if cap is None:
        cap = max(4096, min(n_part_vox * ns, n_part_vox // 2000 * ns + 65536))
    native = bool(exact and HOST_PATH == "native")
    if vox.block_f32 is not None and (not native or split is not None):
        # (the store type per block exists in mmx_detect_batch's exact re-score of every candidate alone)
        raise NotImplementedError("preprocessed blocks of a float32 image are detected with exact values and the native "
                                  "host path only (blob_log.HOST_PATH = \"native\"), and never in parts")
    a = _detect_args(lane, vox, bufs, which, ws, ws_i, cap, eps, exact, native, side_tail, zx_mode)
    ev_read, ev_done = bufs.events(which)
    d_parents = d_parts = None
    if split is not None:
        lo, hi = split.boxes[:, 0], split.boxes[:, 1]
        if (lo < 0).any() or (hi > np.asarray(split.shape)).any() or (split.cores[:, 0] < lo).any() or \
                (split.cores[:, 1] > hi).any():
            raise ValueError("a part outside its block")           # (the re-score reads the parent at folded coordinates)
        d_parents = _to_device_bytes(vox.parents, dev)
        d_parts = _to_device_bytes(split.records(0), dev)
        a.d_parts, a.n_parts = d_parts.data_ptr(), len(split)
        a.d_parents, a.h_parents, a.n_parents = d_parents.data_ptr(), vox.parents.ctypes.data, 1
    info = nat.DetectInfo()
    # a small raw batch that comes by again and again: captured once, then replayed (never a block in parts)
    if NATIVE_BATCH and pre is None and native and split is None:
        rc = _launch_batch(L, a, info, bufs, nb, blocks, space, vol32, vox.vol_exact, ev_read if side_tail else None)
    else:
        rc = L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
    if rc != 0:
        detail = L.mmx_detect_last_error().decode()
        nat.check(rc, "mmx_detect_batch" + (f" [{detail}]" if detail and rc == 2 else ""))
    global LAST_ZX_PATH, LAST_PASS_ROUNDS, LAST_MASK_LAYOUT, LAST_Q16_BOUND, LAST_NMS_BAND
    LAST_ZX_PATH = info.zx_path
    LAST_PASS_ROUNDS, LAST_MASK_LAYOUT = info.n_pass_rounds, info.mask_layout
    if info.zx_path == nat.MMX_ZX_TILED_Q16:
        LAST_Q16_BOUND, LAST_NMS_BAND = info.q16_bound, eps
    if side_tail:
        bufs.ws_free[ws_i] = ev_read
    return _Batch(lane=lane, origins=origins, shapes=shapes, blocks=blocks, d_blocks=vox.d_blocks, nb=nb, ns=ns, n_vox=n_vox,
                  cap=cap, which=which, done=ev_done, store_f32=vox.store_f32, vol_exact=vox.vol_exact, eps=eps, exact=exact,
                  native=native, split=split, parents=vox.parents, d_parents=d_parents, d_parts=d_parts,
                  n_part_vox=n_part_vox, zx_mode=zx_mode, block_f32=vox.block_f32)


def _launch_batch(L, a, info, bufs: _Buffers, nb: int, blocks, space, vol32, vol_exact, ev_read) -> int:
    """``mmx_detect_batch(a)`` -- or, for a small batch that has come by with the very same arguments before (a small
    volume detected step after step: same buffers, geometry, scales, band), the replay of its captured hipGraph: one
    launch instead of a dozen.  The second sighting of a key captures, later ones replay; a capture is refused while
    per-kernel timing is on (its events cannot live inside one) and the plain call is made instead."""
    if not (0 < nb <= GRAPH_BLOCKS) or a.ev_work_free:
        return L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
    if L.mmx_timing_is_enabled():                   # (a replay would hide the kernels from the per-kernel timing, and
        return L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))      # a capture cannot hold its events)
    caller = None
    if not a.stream:
        # the caller works on the default stream, which cannot be captured: the batch runs on a stream of this module's
        # instead, ordered after what the caller has queued and before what it queues next
        caller = torch.cuda.current_stream()
        if bufs.graph_stream is None:
            bufs.graph_stream = torch.cuda.Stream(device=bufs.dev)
        gs = bufs.graph_stream
        origin = a.stream
        for name in ("stream", "tail_stream", "pack_stream"):
            if getattr(a, name) == origin:
                setattr(a, name, gs.cuda_stream)
        gs.wait_stream(caller)
    rc = _launch_batch_graph(L, a, info, bufs, blocks, space, vol32, vol_exact, ev_read)
    if caller is not None:
        caller.wait_stream(bufs.graph_stream)
    return rc


def _launch_batch_graph(L, a, info, bufs: _Buffers, blocks, space, vol32, vol_exact, ev_read) -> int:
    # everything a node of the graph would freeze (the two volume records by content: their addresses change per call)
    key = (bytes(vol32), bytes(vol_exact), blocks.tobytes(), space.sigmas.tobytes(), a.d_blocks, a.slot_elems, a.d_w0,
           a.d_w2, a.d_work, a.work_bytes, a.thr, a.eps, a.d_cands, a.cap, a.h_prefix, a.d_count, a.h_count, a.h_cands,
           a.zx_mode, a.zx_flags, a.store_f32, a.stream, a.tail_stream, a.pack_stream)
    hit = bufs.graphs.get(key)
    if hit is None:                                 # first sighting: remember it, run it plainly
        if len(bufs.graphs) >= 16:
            bufs.drop_graphs()
        bufs.graphs[key] = ()
        return L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
    if hit == "plain":                              # a capture of this batch failed once: launched call by call
        return L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
    if not hit:
        # second sighting: capture (this only records the launches; the replay below runs them)
        graph = ctypes.c_void_p()
        rc = L.mmx_detect_batch_capture(ctypes.byref(a), ctypes.byref(info), ctypes.byref(graph))
        if rc != 0:
            # not capturable (the library says why in mmx_detect_last_error): never tried again for this key
            bufs.graphs[key] = "plain"
            return L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
        hit = bufs.graphs[key] = (graph.value, nat.DetectInfo.from_buffer_copy(info), (blocks, space))
    graph, saved, _ = hit
    global GRAPH_REPLAYS
    GRAPH_REPLAYS += 1
    ctypes.memmove(ctypes.byref(info), ctypes.byref(saved), ctypes.sizeof(info))
    rc = L.mmx_graph_launch(graph, a.stream, a.ev_done, None)
    if rc == 0 and ev_read is not None:
        # (the graph is ordered as a whole on `stream`: "the NMS has read the workspace" holds once it is through)
        ev_read.record(a.stream)
    return rc


_FINISHED = object()        # what `_finish_detect` returns when a finisher has taken the whole batch


def _redo(batch: _Batch, dvol, bufs: _Buffers, *, cap: Optional[int], eps: float, exact: bool):
    """Nominate ``batch`` again -- its candidate table overflowed, or its band proved too narrow -- and finish it.  The
    pipeline has reused the workspace, so the passes run again: the main stream is synchronised first, and the batch goes
    up outside the pipeline (no ``pipe``).  It keeps its slot ``which``, its ``indices`` and its count of ``retries``,
    and is never offered to a ``finisher``.  A block in parts is nominated again whole: all its parts, the same split."""
    torch.cuda.current_stream().synchronize()
    again = _enqueue_detect(dvol, batch.lane, batch.origins, batch.shapes, bufs, batch.which, cap=cap, eps=eps, exact=exact,
                            split=batch.split, zx_mode=batch.zx_mode)
    again.indices, again.retries = batch.indices, batch.retries
    return _finish_detect(again, dvol, bufs)


def _finish_detect(batch: _Batch, dvol, bufs: _Buffers, finisher=None):
    """Wait for one batch's candidates and turn them into ordered raw peaks
    ``(coords int64 (n, 4), values float64 (n,))`` per block."""
    batch.done.synchronize()
    global LAST_BATCH_DONE_T
    LAST_BATCH_DONE_T = time.perf_counter()      # (bench.py: what a step still does after its last kernel)
    lane, eps, which, cap, ns, native = batch.lane, batch.eps, batch.which, batch.cap, batch.ns, batch.native
    space, thr, stats = lane.space, lane.threshold, lane.stats
    words = bufs.host_counts[which].numpy().view(np.uint32)
    count = int(words[0])
    n_cands = int(words[1]) if native else count
    # (a block in parts: the count is that of the folded table -- at most the block's voxels -- unless the table
    #  overflowed before the fold, which then left the parts' count alone)
    cube = (batch.n_vox if (batch.split is None or n_cands <= cap) else batch.n_part_vox) * ns
    if native and n_cands >= cube:
        count = n_cands = 0                 # constant cubes (below)
    if count > cap:
        if count >= cube and not native:
            # every voxel of every block "equals its maximum": only possible for constant
            # cubes, which scikit-image treats as having no peaks (peak.py:41-43)
            count = 0
        else:
            # table overflow (rare): redo this batch with a table that fits
            return _redo(batch, dvol, bufs, cap=count + 1024, eps=eps, exact=batch.exact)
    with torch.cuda.stream(bufs.side):
        table = bufs.cands[which]
        try:
            if native:
                if count <= _PREFIX_ENTRIES:
                    cands = bufs.host_table(which).numpy()[:count * nat.CAND_DTYPE.itemsize].view(nat.CAND_DTYPE)
                else:
                    cands = table[:count * nat.CAND_DTYPE.itemsize].cpu().numpy().view(nat.CAND_DTYPE)
                # (mmx_host_finish_stack takes whole stacks of ordinary blocks: never a block in parts)
                if finisher is not None and batch.split is None and finisher(batch.indices, cands, n_cands, batch.blocks,
                                                                             space, thr, eps, lane.overlap, stats):
                    stats.n_blocks += batch.nb
                    stats.n_voxels += batch.n_vox
                    stats.n_part_voxels += batch.n_part_vox
                    stats.n_candidates += n_cands
                    return _FINISHED
                out = _resolve_peaks_native(cands, n_cands, batch.table_blocks, ns, thr, stats, eps)
            else:
                cands = (table[:count * nat.CAND_DTYPE.itemsize].cpu().numpy().view(nat.CAND_DTYPE)
                         if count else np.zeros(0, dtype=nat.CAND_DTYPE))
                out = _resolve_peaks(cands, batch.table_blocks, batch.shapes, ns, thr, dvol, batch.vol_exact,
                                     batch.d_table_blocks,
                                     lane.d_w0, lane.d_w2, space, batch.store_f32, stats, eps, batch.exact)
        except _BandTooNarrow as exc:
            out = None
            err = exc.err
        if out is not None:
            stats.n_blocks += len(batch.shapes)
            stats.n_voxels += batch.n_vox
            stats.n_part_voxels += batch.n_part_vox
            stats.n_candidates += n_cands
            return out
    # the float32 values were further from the exact ones than the band allows: nominate this batch again
    # with a band of 8 x the deviation found (the exact re-score then decides as always)
    if batch.retries >= 6:
        raise nat.MmxError(f"float32 LoG deviates from the exact values by {err:.3g}: no usable band")
    stats.n_band_retries += 1
    batch.retries += 1
    return _redo(batch, dvol, bufs, cap=None, eps=max(2.0 * eps, 8.0 * err), exact=True)


def blob_log(image, min_sigma=1, max_sigma=50, num_sigma=10, threshold=.2, overlap=.5):
    """``skimage.feature.blob_log`` signature for one 3-D image (host array or tensor)."""
    dvol = image if isinstance(image, DeviceVolume) else DeviceVolume(image)
    if dvol.multichannel:
        raise ValueError("blob_log takes a single-channel (z, y, x) image")
    return blob_log_blocks(dvol, 0, [(0, 0, 0)], [dvol.shape[:3]], min_sigma, max_sigma, num_sigma,
                           threshold, overlap)[0]
