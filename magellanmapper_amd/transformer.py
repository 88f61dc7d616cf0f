"""Whole-image down-sampling and plane transposition on the device (mirror of ``magmap.atlas.transformer``).

``mm <img> --proc transform`` (reference magmap/io/cli.py:1233 -> magmap/atlas/transformer.py:152 ``transpose_img``)
re-orients the stack and down-samples it for registration: the image is cut into chunks of 100 x 500 x 500 voxels
(``chunking.stack_splitter``), every chunk is resized ON ITS OWN through ``cv_nd.rescale_resize`` ->
``skimage.transform.rescale`` / ``resize`` in a process pool, and the resized chunks are merged into
``<base>_<modifier>_image5d.npy`` with its metadata.  Here the chunks of one layer of the plan are one batch of
``csrc/mmx_downsample.hip``:

* ``rescale=`` -- no anti-aliasing (``rescale``'s default from scikit-image 0.19 on): one kernel reads the raw voxels
  through the zoom's axis tables, converts them like ``img_as_float``, interpolates, clips to the chunk's converted range
  and writes the chunk's place in a device copy of the output volume;
* ``target_size=`` -- ``resize`` anti-aliases a chunk that shrinks: the three ``correlate1d`` passes of its Gaussian
  are evaluated only at the planes, rows and columns the zoom reads (:func:`compact_axis_table`) and written compacted,
  the zoom then reads the compact array through remapped tables.  Every value computed is the dense pass's sum in the
  dense pass's order, so the result is the dense result, bit for bit.

The arithmetic is the pinned release's (scikit-image >= 0.19, pinned 0.25.2; ``scipy.ndimage.zoom(order=1,
mode='mirror', grid_mode=True)``); every result is float64, or float32 for a float32 image.

Host images larger than the device go up one layer of chunks at a time (:data:`LAYER_BYTES`).  The next layer's upload
is started before the current layer's kernels and waited for only ahead of its own first kernel, so a streamed upload
(a large read-only memory map cut along z or y) runs beside them; the device then holds two layers, the passes'
intermediates and the output volume, which is copied out once.  Other sources go up synchronously, layer after layer.

``preprocess_img`` (reference transformer.py:353-393, ``--proc preprocess=saturate,denoise,remap,rotate``) runs the
whole-image tasks of :mod:`equalize` (``saturate``, ``denoise``, ``remap``) and ``rotate_img`` (:mod:`rotate`: the atlas
profile's chain of plane rotations, two streaming passes per rotation) in the order given and writes
``<base>_image5d.npy`` slab by slab; ``rotate`` is refused while no atlas profile is set, ``denoise`` for an integer
image that nothing ahead of it stretched to 0-1.  How an image goes up and a result comes down is :mod:`device_image`'s.
Setting up atlas profiles, ``order=0`` label images in ``transpose_img`` and registration stay in the reference.
"""
from __future__ import annotations

import ctypes
import time
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as nat
from . import chunking, config, equalize, importer, kernels1d
from . import device_image as dimg
from . import rotate as rot

#: chunk size of the reference's plan (transformer.py:227), in z, y, x
MAX_PIXELS = (100, 500, 500)
#: byte budget of a host image that stays resident for the whole call; a larger one goes up one layer of chunks at a
#: time.  ``None``: 60 % of the device memory free at the call
LAYER_BYTES: Optional[int] = None
#: file axes behind the (z, y, x) axes of each orientation: "xz" swaps z and y, "yz" then swaps the new z and x
#: (transformer.py:209-218)
_PLANE_AXES = {"xy": (0, 1, 2), "xz": (1, 0, 2), "yz": (2, 0, 1)}


class Downsampler(object):
    """``magmap.atlas.transformer.Downsampler``: the image shared by the chunks of one call."""
    img = None

    @classmethod
    def set_data(cls, img):
        cls.img = img

    @classmethod
    def rescale_sub_roi(cls, coord: Sequence[int], slices: Sequence[slice], target_size, multichannel: bool,
                        sub_roi: Optional[np.ndarray] = None) -> Tuple[Sequence[int], np.ndarray]:
        """``(coord, the rescaled or resized chunk)``: ``target_size`` a factor or a (z, y, x) shape."""
        from . import preprocess
        if sub_roi is None and cls.img is not None:
            sub_roi = cls.img[tuple(slices)]
        return coord, preprocess.rescale_resize(sub_roi, target_size, multichannel)


def make_modifier_plane(plane) -> str:
    return "plane{}".format(plane.upper())


def make_modifier_scale(scale) -> str:
    return "scale{}".format(scale).replace(".", "pt")


def make_modifier_resized(target_size) -> str:
    return "resized({},{},{})".format(*target_size)


def _insert_before_ext(name: str, insert: str, sep: str = "") -> str:
    """``libmag.insert_before_ext`` (reference libmag.py:247-269)."""
    import os
    name = str(name)
    if os.path.basename(name).find(".") == -1:
        return name + sep + insert
    return "{0}{2}{3}.{1}".format(*name.rsplit(".", 1), sep, insert)


def get_transposed_image_path(img_path: str, scale: Optional[float] = None,
                              target_size: Optional[Sequence[int]] = None) -> str:
    """``img_path`` with the modifier of the transposition; unchanged when both factors are ``None``."""
    if scale is None and target_size is None:
        return img_path
    modifier = make_modifier_scale(scale) if scale is not None else make_modifier_resized(target_size)
    return _insert_before_ext(img_path, "_" + modifier)


# ------------------------------------------------------------------------------------------------------ the plan
class Plan(NamedTuple):
    """The chunks of one call: a separable grid, so everything is per axis."""
    slices: np.ndarray                  # ``stack_splitter``'s object grid of slice triples
    max_pixels: Tuple[int, int, int]    # the chunk size in effect (``target_size`` recomputes it)
    sub_roi_size: Optional[Tuple[int, int, int]]   # every chunk's target shape (``target_size``), or None
    starts: Tuple[np.ndarray, ...]      # per axis: chunk origins
    n_in: Tuple[np.ndarray, ...]        # per axis: chunk extents
    n_out: Tuple[np.ndarray, ...]       # per axis: resized extents
    offsets: Tuple[np.ndarray, ...]     # per axis: where a resized chunk starts in the output (cumulative extents)
    total_shape: Tuple[int, int, int]   # ``get_split_stack_total_shape``
    antialias: bool


def plan_chunks(shape3: Sequence[int], rescale: Optional[float] = None,
                target_size_zyx: Optional[Sequence[int]] = None, max_pixels: Sequence[int] = MAX_PIXELS) -> Plan:
    """The reference's chunk plan (transformer.py:227-249) and every chunk's resized extent: ``np.round(scale *
    chunk_shape)`` for ``rescale`` (half to even, as ``skimage.transform.rescale`` rounds), ``floor(target_size /
    num_chunks)`` for every chunk of a ``target_size``, whose chunk size is first evened out to ``ceil(shape /
    ceil(shape / max_pixels))``.  With BOTH given the reference still evens the chunk size out (its ``if target_size:``
    stands beside, not behind, the test for ``rescale``) and then rescales the evened chunks by ``rescale``; so does
    this.  A chunk with an empty resized extent is a ``ValueError`` naming chunk and axis."""
    shape3 = tuple(int(v) for v in shape3[:3])
    if rescale is None and target_size_zyx is None:
        raise ValueError("rescale or target_size is needed")
    sub = None
    if target_size_zyx is not None and len(target_size_zyx):
        num_chunks = np.ceil(np.divide(shape3, max_pixels))
        max_pixels = np.ceil(np.divide(shape3, num_chunks)).astype(int)
        sub = np.floor(np.divide(target_size_zyx, num_chunks)).astype(int)
    mp_ = tuple(int(v) for v in max_pixels)
    slices, _ = chunking.stack_splitter(shape3, mp_)
    starts, n_in, n_out, offsets = [], [], [], []
    for a in range(3):
        idx = [0, 0, 0]
        st, ni = [], []
        for k in range(slices.shape[a]):
            idx[a] = k
            sl = slices[tuple(idx)][a]
            st.append(sl.start)
            ni.append(sl.stop - sl.start)
        ni = np.array(ni, dtype=np.int64)
        if rescale is not None:
            no = np.round(np.float64(rescale) * ni).astype(np.int64)
        else:
            no = np.full(len(ni), int(sub[a]), dtype=np.int64)
        for k in np.flatnonzero(no < 1):
            raise ValueError(f"chunk {int(k)} along axis {a} ({'zyx'[a]}), {int(ni[k])} voxels thick, is resized to an "
                             f"empty extent ({int(no[k])})")
        starts.append(np.array(st, dtype=np.int64))
        n_in.append(ni)
        n_out.append(no)
        offsets.append(np.concatenate(([0], np.cumsum(no)[:-1])).astype(np.int64))
    total = tuple(int(no.sum()) for no in n_out)
    return Plan(slices, mp_, None if sub is None or rescale is not None else tuple(int(v) for v in sub), tuple(starts), tuple(n_in),
                tuple(n_out), tuple(offsets), total, rescale is None)


def axis_table(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """``preprocess.zoom_axis_table`` in 'mirror' mode, and for an axis of length 1 what SciPy does there (the single
    sample: coordinate 0, weights 1 and 0) -- the transposition keeps 'reflect' for such chunks, only
    ``make_isotropic`` switches to 'edge'."""
    from . import preprocess
    if int(n_in) == 1:
        return (np.zeros((int(n_out), 2), dtype=np.int32),
                np.tile(np.array([1.0, 0.0]), (int(n_out), 1)))
    return preprocess.zoom_axis_table(int(n_in), int(n_out), "mirror")


def compact_axis_table(idx: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(pick, idx_compact)``: the sorted source positions an axis table reads, and the table remapped to positions
    in that list -- ``pick[idx_compact] == idx`` everywhere, so a pass evaluated at ``pick`` and stored compacted is
    read by ``idx_compact`` exactly where the dense array was read by ``idx``."""
    idx = np.asarray(idx, dtype=np.int32)
    pick = np.unique(idx.reshape(-1)).astype(np.int32)
    return pick, np.searchsorted(pick, idx).astype(np.int32)


#: test hook: ``{sigma: half kernel}`` to use instead of this NumPy's weights (``np.exp`` is not bit-stable across NumPy
#: releases, and the golden fixture was made under NumPy 1.26)
AA_WEIGHTS_OVERRIDE: Optional[Dict[float, np.ndarray]] = None


def aa_weights(sigma: float, radius: int) -> np.ndarray:
    """Half kernel ``w[0 .. radius]`` of one anti-aliasing pass (``scipy.ndimage._filters._gaussian_kernel1d``); the
    one-tap kernel of a radius 0 is exactly ``[1.0]``."""
    if not radius:
        return np.array([1.0])
    if AA_WEIGHTS_OVERRIDE is not None and float(sigma) in AA_WEIGHTS_OVERRIDE:
        w = np.ascontiguousarray(AA_WEIGHTS_OVERRIDE[float(sigma)], dtype=np.float64)
        if len(w) != radius + 1:
            raise ValueError(f"override for sigma {sigma} holds {len(w)} weights, radius {radius} needs {radius + 1}")
        return w
    return kernels1d.gaussian_half_kernel(float(sigma), 0, int(radius))


def aa_sigmas(in_shape: Sequence[int], out_shape: Sequence[int]) -> np.ndarray:
    """``resize``'s anti-aliasing sigmas, ``max(0, (in / out - 1) / 2)`` per axis (zero wherever nothing shrinks)."""
    factors = np.divide(np.asarray(in_shape, dtype=np.int64), np.asarray(out_shape, dtype=np.int64))
    return np.maximum(0, (factors - 1) / 2)


# ------------------------------------------------------------------------------------------------ the device side
class _Source:
    """The image, or one layer of it, on the device in FILE orientation, addressed in the orientation of the output:
    per-channel views whose strides are the file's, permuted (a plane swap costs no copy), and whose base is shifted
    so that chunk coordinates of the whole swapped volume find their voxels in a layer's box."""

    def __init__(self, tensor, axes, lo: int, keep=None):
        self.tensor = tensor
        self.keep = keep
        multichannel = tensor.ndim == 4
        st = tensor.stride()
        self.strides = tuple(int(st[axes[a]]) for a in range(3))
        code = nat.NP_TO_MMX[dimg.np_dtype_of(tensor)]
        base = int(tensor.data_ptr()) - lo * self.strides[0] * tensor.element_size()
        n_chl = tensor.shape[3] if multichannel else 1
        self.views = [nat.Volume(base + c * tensor.element_size(), code, 0, *self.strides) for c in range(n_chl)]

    def wait(self) -> None:
        """The current stream waits for this source's upload, if one is still in flight: called right before the
        first kernel that reads it, so that the copy stream runs beside whatever was launched before."""
        if self.keep is not None:
            self.keep.stream_wait()

    def close(self):
        if self.keep is not None:
            self.keep.close()
        self.keep = self.tensor = None


def _upload(arr, axes, lo: int, hi: int, dev, whole: bool) -> _Source:
    """Planes ``[lo, hi)`` of the swapped volume = a box of the file along file axis ``axes[0]``."""
    from .volume import DeviceVolume
    box = [slice(None)] * arr.ndim
    if not whole:
        box[axes[0]] = slice(lo, hi)
    sub = arr[tuple(box)]
    # (z- and y-boxes of a memory map stream from where they lie; an x-box has no packed planes: one packed copy)
    # (the constructor returns with a streamed upload still in flight: `_Source.wait` orders the kernels behind it)
    dv = DeviceVolume(sub, dev, streamed=None if axes[0] in (0, 1) else False)
    return _Source(dv.tensor, axes, 0 if whole else lo, dv)


def _run_batch(src: _Source, raw_dtype: np.dtype, chunks, out_t, antialias: bool, sparse: bool = True) -> None:
    """One batch: ``chunks`` = ``(origin zyx, in shape, output offset zyx, out shape)`` in the swapped volume."""
    L = nat.lib()
    dev = out_t.device
    stream = dimg.stream()
    nb = len(chunks)
    raw_code = nat.NP_TO_MMX[np.dtype(raw_dtype)]
    f32 = raw_code == nat.MMX_F32
    mid_code = nat.MMX_F32 if f32 else nat.MMX_F64
    mid_t = torch.float32 if f32 else torch.float64
    sz, sy, sx = src.strides
    n_chl = len(src.views)
    ost = out_t.stride()
    keep = []
    src.wait()

    # ---- the clip range: raw min / max of every chunk over all of its channels
    blocks = np.zeros(nb, dtype=nat.BLOCK_DTYPE)
    for i, (o, shp, _, _) in enumerate(chunks):
        blocks[i] = (o[0] * sz + o[1] * sy + o[2] * sx, shp[0], shp[1], shp[2], i, 0, 0)
    d_blocks = dimg.to_dev(blocks, dev)
    mm = np.empty((nb, 2))
    mm[:, 0], mm[:, 1] = np.inf, -np.inf
    d_mm = torch.from_numpy(mm).to(dev)
    for v in src.views:
        nat.check(L.mmx_minmax_batch(ctypes.byref(v), d_blocks.data_ptr(), blocks.ctypes.data, nb, d_mm.data_ptr(),
                                     stream), "mmx_minmax_batch")

    # ---- the anti-aliasing passes of this batch: (sigma, radius) per chunk and axis; an axis no chunk filters is skipped
    radii = np.zeros((nb, 3), dtype=np.int32)
    sigmas = np.zeros((nb, 3))
    if antialias:
        for i, (_, shp, _, oshp) in enumerate(chunks):
            sg = aa_sigmas(shp, oshp)
            for a in range(3):
                if sg[a] > 1e-15:                  # (scipy.ndimage.gaussian_filter skips the others)
                    sigmas[i, a] = sg[a]
                    radii[i, a] = kernels1d.kernel_radius(sg[a])
    pass_axes = [a for a in range(3) if (sigmas[:, a] > 0).any()]
    tables = {a: {} for a in range(3)}             # (n_in, n_out) -> (idx, wts, pick, idx_compact)
    for _, shp, _, oshp in chunks:
        for a in range(3):
            key = (int(shp[a]), int(oshp[a]))
            if key not in tables[a]:
                idx, wts = axis_table(*key)
                # (dense: every position is "picked" and the tables stay as they are)
                tables[a][key] = (idx, wts) + (compact_axis_table(idx) if sparse
                                              else (np.arange(key[0], dtype=np.int32), idx))

    for c in range(n_chl):
        cur = nat.DsView(src.views[c].d_data, src.views[c].dtype, 0, sz, sy, sx)
        offs = [int(b["src_off"]) for b in blocks]
        ext = [[int(v) for v in shp] for _, shp, _, _ in chunks]
        for a in pass_axes:
            pick_off, picks, at = {}, [], 0
            rec = np.zeros(nb, dtype=nat.DS_CHUNK_DTYPE)
            oext = []
            for i, (_, shp, _, oshp) in enumerate(chunks):
                key = (int(shp[a]), int(oshp[a]))
                if key not in pick_off:
                    pick_off[key] = at
                    picks.append(tables[a][key][2])
                    at += len(picks[-1])
                e = list(ext[i])
                e[a] = len(tables[a][key][2])
                oext.append(e)
            mx = np.max(np.array(oext), axis=0)
            dst_sy = int(mx[2])
            dst_sz = dst_sy * int(mx[1])
            slot = dst_sz * int(mx[0])
            for i, (_, shp, _, oshp) in enumerate(chunks):
                t3 = [0, 0, 0]
                t3[a] = pick_off[(int(shp[a]), int(oshp[a]))]
                rec[i] = (offs[i], i * slot, ext[i][0], ext[i][1], ext[i][2], oext[i][0], oext[i][1], oext[i][2], i,
                          t3[0], t3[1], t3[2], (0, 0))
            pitch = int(radii[:, a].max()) + 1
            wts = np.zeros((nb, pitch))
            for i in range(nb):
                # (a chunk without a pass of its own along this axis: the one-tap kernel [1.0] copies, exactly)
                wts[i, :radii[i, a] + 1] = aa_weights(sigmas[i, a], int(radii[i, a]))
            h_r = np.ascontiguousarray(radii[:, a])
            h_pick = np.ascontiguousarray(np.concatenate(picks), dtype=np.int32)
            buf = torch.empty(nb * slot, dtype=mid_t, device=dev)
            d_rec, d_w, d_r, d_pick = (dimg.to_dev(h, dev) for h in (rec, wts, h_r, h_pick))
            nat.check(L.mmx_ds_gauss_pick_batch(ctypes.byref(cur), d_rec.data_ptr(), rec.ctypes.data, nb, a,
                                                d_w.data_ptr(), d_r.data_ptr(), h_r.ctypes.data, pitch,
                                                d_pick.data_ptr(), h_pick.ctypes.data, len(h_pick), dst_sy, dst_sz,
                                                nb * slot, buf.data_ptr(), stream), "mmx_ds_gauss_pick_batch")
            keep.append((buf, d_rec, d_w, d_r, d_pick))
            cur = nat.DsView(buf.data_ptr(), mid_code, 0, dst_sz, dst_sy, 1)
            offs = [i * slot for i in range(nb)]
            ext = oext
        # ---- the zoom, through dense tables along the axes left as they were and remapped ones along the compacted
        tab_off, tabs_i, tabs_w, at = {}, [], [], 0
        rec = np.zeros(nb, dtype=nat.DS_CHUNK_DTYPE)
        for i, (_, shp, ooff, oshp) in enumerate(chunks):
            t3 = []
            for a in range(3):
                key = (a, int(shp[a]), int(oshp[a]))
                if key not in tab_off:
                    idx, wts, _, idx_c = tables[a][key[1:]]
                    tab_off[key] = at
                    tabs_i.append(idx_c if a in pass_axes else idx)
                    tabs_w.append(wts)
                    at += len(idx)
                t3.append(tab_off[key])
            rec[i] = (offs[i], ooff[0] * ost[0] + ooff[1] * ost[1] + ooff[2] * ost[2] + c, ext[i][0], ext[i][1],
                      ext[i][2], oshp[0], oshp[1], oshp[2], i, t3[0], t3[1], t3[2], (0, 0))
        h_idx = np.ascontiguousarray(np.concatenate(tabs_i), dtype=np.int32)
        h_wts = np.ascontiguousarray(np.concatenate(tabs_w), dtype=np.float64)
        d_rec, d_idx, d_wts = (dimg.to_dev(h, dev) for h in (rec, h_idx, h_wts))
        dst = nat.DsView(out_t.data_ptr(), mid_code, 0, int(ost[0]), int(ost[1]), int(ost[2]))
        nat.check(L.mmx_ds_zoom_batch(ctypes.byref(cur), ctypes.byref(dst), out_t.numel(), d_rec.data_ptr(),
                                      rec.ctypes.data, nb, d_idx.data_ptr(), h_idx.ctypes.data, len(h_idx),
                                      d_wts.data_ptr(), d_mm.data_ptr(), raw_code, stream), "mmx_ds_zoom_batch")
        keep.append((d_rec, d_idx, d_wts))
    # the tables and intermediates above are read by kernels still in flight: they are released behind them
    torch.cuda.current_stream().synchronize()


def resize_chunk(roi: np.ndarray, out_shape: Sequence[int], antialias: bool) -> np.ndarray:
    """One ``(z, y, x[, c])`` array resized on its own to ``out_shape`` (z, y, x): what every chunk of
    :func:`downsample` goes through, and all of ``preprocess.rescale_resize``."""
    from .volume import _require_gpu
    roi = np.asarray(roi)
    if roi.dtype not in nat.NP_TO_MMX:
        raise NotImplementedError(f"down-sampling of {roi.dtype} images is not built")
    out_shape = tuple(int(v) for v in out_shape)
    if min(out_shape) < 1 or min(roi.shape) < 1:
        raise ValueError(f"a {roi.shape[:3]} array resized to {out_shape} is empty")
    dev = _require_gpu()
    n_chl = roi.shape[3] if roi.ndim == 4 else 1
    odt = torch.float32 if roi.dtype == np.float32 else torch.float64
    out_t = torch.empty(out_shape + (n_chl,), dtype=odt, device=dev)
    src = _upload(roi, _PLANE_AXES["xy"], 0, roi.shape[0], dev, True)
    try:
        _run_batch(src, roi.dtype, [((0, 0, 0), tuple(int(v) for v in roi.shape[:3]), (0, 0, 0), out_shape)], out_t,
                   antialias)
    finally:
        src.close()
    return (out_t if roi.ndim == 4 else out_t[..., 0]).cpu().numpy()


def downsample(img, rescale: Optional[float] = None, target_size: Optional[Sequence[int]] = None,
               plane: Optional[str] = None, max_pixels: Sequence[int] = MAX_PIXELS, out=None,
               layer_bytes: Optional[int] = None, sparse: bool = True) -> np.ndarray:
    """A ``(z, y, x[, c])`` image re-oriented to ``plane`` and down-sampled chunk by chunk as ``transpose_img`` does:
    ``rescale`` (a factor; takes precedence) or ``target_size`` (x, y, z, as the reference's callers give it); with both,
    the chunks are evened out as for ``target_size`` and rescaled by ``rescale``, as the reference does.
    Returns the float64 (float32 for a float32 image) result, written into ``out`` when given (the memory map of the
    output file).  ``layer_bytes`` overrides :data:`LAYER_BYTES`.  ``sparse=False`` evaluates the anti-aliasing passes at
    every position instead of the picked ones (the same kernels, dense: what measurements compare against)."""
    from .volume import DeviceVolume, _require_gpu
    if rescale is None and target_size is None:
        raise ValueError("rescale or target_size is needed")
    if plane is not None and plane not in _PLANE_AXES:
        raise ValueError(f"plane must be one of {tuple(_PLANE_AXES)}, not {plane!r}")
    axes = _PLANE_AXES[plane or "xy"]
    resident = isinstance(img, DeviceVolume)
    if resident:
        if img.z_off or img.y_off:
            raise ValueError("a DeviceVolume that holds a box of its image cannot be down-sampled")
        img.wait_all()
    elif not isinstance(img, np.ndarray):
        img = np.asarray(img)
    dtype, fshape, _ = dimg.describe(img)
    if len(fshape) not in (3, 4):
        raise ValueError("image must be (z, y, x) or (z, y, x, c)")
    multichannel = len(fshape) == 4
    if np.dtype(dtype) not in nat.NP_TO_MMX:
        raise NotImplementedError(f"down-sampling of {dtype} images is not built "
                                  f"({', '.join(str(d) for d in nat.NP_TO_MMX)} are)")
    shape3 = tuple(int(fshape[axes[a]]) for a in range(3))
    tsz = [int(v) for v in target_size][::-1] if target_size is not None and len(target_size) else None
    plan = plan_chunks(shape3, rescale, tsz, max_pixels)         # (raises before any launch)
    n_chl = fshape[3] if multichannel else 1
    odt = np.dtype(np.float32 if np.dtype(dtype) == np.float32 else np.float64)
    oshape = plan.total_shape + ((n_chl,) if multichannel else ())
    if out is not None and (tuple(out.shape) != oshape or out.dtype != odt):
        raise ValueError(f"out must be {oshape} {odt}, not {tuple(out.shape)} {out.dtype}")

    dev = img.tensor.device if resident else _require_gpu()
    out_t = torch.empty(plan.total_shape + (n_chl,), dtype=getattr(torch, odt.name), device=dev)
    grid = plan.slices.shape

    def layer_chunks(kz):
        return [((int(plan.starts[0][kz]), int(plan.starts[1][ky]), int(plan.starts[2][kx])),
                 (int(plan.n_in[0][kz]), int(plan.n_in[1][ky]), int(plan.n_in[2][kx])),
                 (int(plan.offsets[0][kz]), int(plan.offsets[1][ky]), int(plan.offsets[2][kx])),
                 (int(plan.n_out[0][kz]), int(plan.n_out[1][ky]), int(plan.n_out[2][kx])))
                for ky in range(grid[1]) for kx in range(grid[2])]

    def batches(kz):
        chunks = layer_chunks(kz)
        for i in range(0, len(chunks), nat.MMX_MAX_BLOCKS):
            yield chunks[i:i + nat.MMX_MAX_BLOCKS]

    if resident:
        src = _Source(img.tensor, axes, 0)
        for kz in range(grid[0]):
            for b in batches(kz):
                _run_batch(src, dtype, b, out_t, plan.antialias, sparse)
    else:
        budget = layer_bytes if layer_bytes is not None else LAYER_BYTES
        if budget is None:
            budget = int(0.6 * dimg.free_bytes())
        if img.nbytes <= budget:
            src = _upload(img, axes, 0, shape3[0], dev, True)
            try:
                for kz in range(grid[0]):
                    for b in batches(kz):
                        _run_batch(src, dtype, b, out_t, plan.antialias, sparse)
            finally:
                src.close()
        else:
            # one layer of chunks at a time: the next layer's upload is started here and waited for in its own _run_batch
            bounds = [(int(plan.starts[0][kz]), int(plan.starts[0][kz] + plan.n_in[0][kz])) for kz in range(grid[0])]
            nxt = _upload(img, axes, *bounds[0], dev, False)
            for kz in range(grid[0]):
                cur, nxt = nxt, None
                try:
                    if kz + 1 < grid[0]:
                        nxt = _upload(img, axes, *bounds[kz + 1], dev, False)
                    for b in batches(kz):
                        _run_batch(cur, dtype, b, out_t, plan.antialias, sparse)
                except BaseException:
                    if nxt is not None:
                        nxt.close()
                    raise
                finally:
                    cur.close()
    res = out_t if multichannel else out_t[..., 0]
    host = res.cpu().numpy()
    if out is not None:
        out[...] = host
        return out
    return host


# ------------------------------------------------------------------------------------------------- transpose_img
def transpose_img(filename: str, series: Optional[int], plane: Optional[str] = None,
                  rescale: Optional[float] = None, target_size: Optional[Sequence[int]] = None):
    """``transformer.transpose_img`` (reference transformer.py:152-323): re-orient ``<base>_image5d.npy`` to ``plane``
    and / or down-sample it by ``rescale`` (takes precedence) or to about ``target_size`` (x, y, z), and write
    ``<base>_<modifier>_image5d.npy`` with its metadata -- resolutions, sizes, scaling, plane and the intensity bounds of
    the result.  All channels are transposed.  ``target_size=None`` reads ``config.atlas_profile["target_size"]`` when
    an atlas profile is set.  Returns the output memory map (the reference returns nothing)."""
    if target_size is None:
        prof = getattr(config, "atlas_profile", None)
        if prof is not None:
            target_size = prof["target_size"]
    if plane is None and rescale is None and target_size is None:
        print("No transposition to perform, skipping")
        return None

    time_start = time.time()
    img5d = importer.read_file(filename, series)
    info = img5d.meta
    image5d = img5d.img
    if image5d is None or info is None:
        raise FileNotFoundError(f"no image5d array and metadata for {filename}")
    sizes = info["sizes"]

    modifier = ""
    if plane is not None:
        modifier = make_modifier_plane(plane)
    if rescale is not None:
        modifier += make_modifier_scale(rescale)
    elif target_size:
        modifier += make_modifier_resized(target_size)
    filename_image5d, filename_info = importer.make_filenames(filename, series, modifier=modifier)

    offset = 0 if image5d.ndim <= 3 else 1
    scaled = rescale is not None or target_size is not None
    # what the result's intensity bounds will be measured in: a refusal (float32 without the NumPy release named,
    # preprocess.FLOAT32_RULES) surfaces here, ahead of the rescale
    out_dtype = (np.dtype(np.float32 if image5d.dtype == np.float32 else np.float64) if scaled else image5d.dtype)
    if not importer._bounds_dtype_ok(out_dtype):
        raise NotImplementedError(f"percentiles of {out_dtype} images ({importer._BOUNDS_NAMES}; float32 once "
                                  f"preprocess.FLOAT32_RULES names the NumPy release)")
    if scaled and image5d.dtype not in nat.NP_TO_MMX:
        raise NotImplementedError(f"down-sampling of {image5d.dtype} images is not built")
    if plane is not None and plane not in config.PLANE:
        raise ValueError(f"plane must be one of {config.PLANE}, not {plane!r}")

    image5d_swapped = image5d
    if plane is not None and plane != config.PLANE[0]:
        image5d_swapped = np.swapaxes(image5d_swapped, offset, offset + 1)
        res = config.resolutions[0]
        res[0], res[1] = res[1], res[0]
        if plane == config.PLANE[2]:
            image5d_swapped = np.swapaxes(image5d_swapped, offset, offset + 2)
            res[0], res[2] = res[2], res[0]

    scaling = None
    if scaled:
        vol = image5d[0] if offset > 0 else image5d        # (file orientation: the swap is done by strides)
        shape3 = (image5d_swapped[0] if offset > 0 else image5d_swapped).shape[:3]
        tsz = [int(v) for v in target_size][::-1] if target_size else None
        plan = plan_chunks(shape3, rescale, tsz, MAX_PIXELS)
        rescaled_shape = np.array(plan.total_shape + tuple(vol.shape[3:]))
        if offset > 0:
            rescaled_shape = np.concatenate(([1], rescaled_shape))
        image5d_transposed = np.lib.format.open_memmap(
            filename_image5d, mode="w+", dtype=out_dtype, shape=tuple(int(v) for v in rescaled_shape))
        downsample(vol, rescale, target_size if target_size else None, plane, MAX_PIXELS,
                   out=image5d_transposed[0] if offset > 0 else image5d_transposed)
        if rescale is not None:
            config.resolutions = np.multiply(config.resolutions, 1 / rescale)
        else:
            config.resolutions = np.multiply(config.resolutions, (image5d_swapped.shape / rescaled_shape)[1:4])
        sizes[0] = rescaled_shape
        scaling = importer.calc_scaling(image5d_swapped, image5d_transposed)
    else:
        image5d_transposed = np.lib.format.open_memmap(
            filename_image5d, mode="w+", dtype=image5d_swapped.dtype, shape=image5d_swapped.shape)
        if plane == config.PLANE[1] or plane == config.PLANE[2]:
            if offset:
                image5d_transposed[0, :] = np.fliplr(image5d_swapped[0, :])
            else:
                image5d_transposed[:] = np.fliplr(image5d_swapped[:])
        else:
            image5d_transposed[:] = image5d_swapped[:]
        sizes[0] = image5d_swapped.shape

    image5d_transposed.flush()
    importer.save_image_info(
        filename_info, info["names"], sizes, config.resolutions, info["magnification"], info["zoom"],
        *importer.calc_intensity_bounds(image5d_transposed), scaling, plane)
    print("saved transposed file to {} with shape {}".format(filename_image5d, image5d_transposed.shape))
    print("time elapsed (s): {}".format(time.time() - time_start))
    return image5d_transposed


# ------------------------------------------------------------------------------------------------ preprocess_img
def _get_enum(s, enum_class):
    """``libmag.get_enum``: the member named ``s`` (any case), ``None`` when there is none."""
    if s:
        try:
            return enum_class[s.upper()]
        except (AttributeError, KeyError):
            pass
    return None


def rotate_img(roi, rotate=None, order=None, _keep=False, _out=None):
    """``transformer.rotate_img`` (reference transformer.py:326-350): ``roi`` (z, y, x[, c]) through the rotations
    ``rotate["rotation"] = ((angle, axis), ...)`` in order, each on the previous result (``cv_nd.rotate_nd``), at the
    interpolation ``order`` (``None``: ``rotate["order"]``).  ``rotate=None`` reads ``config.atlas_profile["rotate"]``.
    The volume stays on the device between the rotations and leaves it once; a host array comes back for a host array,
    a ``DeviceVolume`` for a ``DeviceVolume``.  ``rotate["resize"]`` true, orders other than 0 and 1 and float32 at
    order 1 are a ``NotImplementedError`` (:mod:`rotate`).  The one deliberate divergence: ``rotate["rotation"] = None``
    (the profile's default: no rotation) returns a copy of the image unchanged, where the reference's loop fails on
    ``None`` with a ``TypeError``."""
    if rotate is None:
        prof = getattr(config, "atlas_profile", None)
        if prof is None:
            raise NotImplementedError("rotate_img: no atlas profile is set (config.atlas_profile); setting up atlas "
                                      "profiles stays in the reference: pass the rotate settings or set the profile")
        rotate = prof["rotate"]
    if order is None:
        order = rotate["order"]
    rotation = rotate["rotation"]
    if rotation is None:
        rotation = ()
    for r in rotation:
        print("rotating by", r)
    return rot.rotate_chain(roi, rotation, order, rotate["resize"], "rotate_img", _keep, _out)


def tasks_ahead(preprocs, dtype):
    """``[(task, the voxel type it will see)]`` of the names ``preprocs`` on an image of ``dtype``, as far as can be told
    ahead of running anything: float64 once a ``saturate``, ``remap`` or ``denoise`` stands ahead, the image's own until
    then (``rotate`` keeps the type).  A name that is no task is skipped with a warning.  Known gaps, left as they are:
    a multichannel ``remap`` hands on the image's own dtype, and so does ``saturate`` of a flat channel (percentiles
    equal: unchanged)."""
    tasks = []
    for preproc in preprocs:
        task = _get_enum(preproc, config.PreProcessKeys)
        if task is None:
            config.logger.warning("No preprocessing task found for: %s", preproc)
            continue
        stays = all(t is config.PreProcessKeys.ROTATE for t, _ in tasks)
        tasks.append((task, np.dtype(dtype) if stays else np.dtype(np.float64)))
    return tasks


def _check_denoise(dtype, shape, channel) -> None:
    if dtype.kind in "iu":
        # (np.clip of raw counts to [clip_min, clip_max] gives a two-valued image: nothing anyone runs)
        raise NotImplementedError(
            "the whole-image task 'denoise' of an image that was not stretched to 0-1 stays in the reference "
            "(an integer image with neither 'saturate' nor 'remap' ahead of it in the task list)")
    _, chls = equalize._setup_channels(shape, channel)
    equalize.denoise_check_args(dtype, list(chls), "the whole-image task 'denoise'")


def _check_rotate(dtype, shape, channel) -> None:
    prof = getattr(config, "atlas_profile", None)
    if prof is None:
        raise NotImplementedError("the whole-image task 'rotate' reads config.atlas_profile, and none is set: "
                                  "setting up atlas profiles stays in the reference")
    if prof["rotate"]["rotation"] is not None:
        rot.check_args(dtype, prof["rotate"]["order"], prof["rotate"]["resize"], "the whole-image task 'rotate'")


#: task -> (what it refuses ahead of everything, from ``(voxel type ahead, (z, y, x[, c]) shape, channel)``; how it runs)
_TASKS = {
    config.PreProcessKeys.SATURATE: (None, lambda roi, channel, **kw: equalize.saturate_roi(roi, channel=channel, **kw)),
    config.PreProcessKeys.DENOISE: (_check_denoise, lambda roi, channel, **kw: equalize.denoise_roi(roi, channel, **kw)),
    config.PreProcessKeys.REMAP: (None, lambda roi, channel, **kw: equalize.remap_intensity(roi, channel, **kw)),
    config.PreProcessKeys.ROTATE: (_check_rotate, lambda roi, channel, **kw: rotate_img(roi, **kw)),
}


def preprocess_img(image5d, preprocs, channel, out_path):
    """``transformer.preprocess_img`` (reference transformer.py:353-393): run the whole-image tasks ``preprocs`` (names
    of ``config.PreProcessKeys``, one or a sequence) on ``image5d[0]`` in the order given, each on the previous result,
    for ``channel`` (``None``: all), and write ``<out_path base>_image5d.npy`` with its ``_meta.yml`` (the settings in
    :mod:`config`, the intensity bounds of the result).  ``saturate``, ``denoise`` and ``remap`` (:mod:`equalize`) and
    ``rotate`` (:func:`rotate_img`, all channels, the settings of ``config.atlas_profile``) run on the device.  Refused
    with a ``NotImplementedError`` before anything runs, from the voxel type each task will see (:func:`tasks_ahead`):
    ``denoise`` of an integer image with neither ``saturate`` nor ``remap`` ahead of it (raw counts clipped to the
    profile's 0-1 bounds: that stays in the reference), of a float32 image, or with a truthy ``tot_var_denoise`` in a
    channel's profile (:func:`equalize.denoise_check_args`); ``rotate`` without an atlas profile or with settings
    :func:`rotate_img` refuses.  The last task's result goes z-slab by z-slab into the memory map of the output file,
    which is returned (``(1, z, y, x[, c])``); between tasks the image stays on the device.  ``None`` for ``preprocs``
    prints and returns ``None``."""
    import os
    if preprocs is None:
        print("No preprocessing tasks to perform, skipping")
        return None
    if not (isinstance(preprocs, (list, tuple)) or np.ndim(preprocs) != 0):
        preprocs = [preprocs]
    tasks = []
    for task, dtype in tasks_ahead(preprocs, image5d.dtype):
        check = _TASKS[task][0]
        if check is not None:
            check(dtype, tuple(image5d.shape[1:]), channel)
        tasks.append(task)

    # a float32 image that leaves as float32 (no task, `rotate` alone, or `remap` on several channels) has its intensity
    # bounds measured in float32: refused here, ahead of the tasks, unless preprocess.FLOAT32_RULES names the NumPy release
    if (np.dtype(image5d.dtype) == np.float32 and config.PreProcessKeys.SATURATE not in tasks
            and (config.PreProcessKeys.REMAP not in tasks or image5d.ndim > 4)
            and not importer._bounds_dtype_ok(np.float32)):
        raise NotImplementedError(f"percentiles of float32 images ({importer._BOUNDS_NAMES}; float32 once "
                                  f"preprocess.FLOAT32_RULES names the NumPy release)")

    filename_image5d, filename_info = importer.make_filenames(out_path)
    made = []

    def make_out(shape, dtype):
        mm = np.lib.format.open_memmap(filename_image5d, mode="w+", dtype=dtype, shape=(1,) + tuple(shape))
        made.append(mm)
        return mm[0]

    roi = image5d[0]
    for i, task in enumerate(tasks):
        config.logger.info("Pre-processing task: %s", task)
        last = i == len(tasks) - 1
        roi = _TASKS[task][1](roi, channel, **(dict(_out=make_out) if last else dict(_keep=True)))
    if not made:
        # (no task ran: the image as it stands)
        make_out(roi.shape, roi.dtype)[...] = roi
    image5d_out = made[-1]
    image5d_out.flush()
    lows, highs = importer.calc_intensity_bounds(image5d_out)
    importer.save_image_info(filename_info, [os.path.basename(out_path)], [image5d_out.shape], config.resolutions,
                             config.magnification, config.zoom, lows, highs)
    return image5d_out

