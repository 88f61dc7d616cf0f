"""Blob classifier (mirror of ``magmap.cv.classifier``): a model scores one 2-D image patch per detected blob and the
thresholded score goes into the table's ``confirmed`` column.

Same public surface as the reference (magmap/cv/classifier.py): :func:`extract_patches` (:16-55),
:func:`classify_patches` (:58-77), :func:`setup_classification_roi` (:80-146), :func:`classify_blobs` (:149-218) and
:class:`ClassifyImage` (:221-352) with the reference's selection rules and error types.

What changes is *where the patches are cut*: the reference slices, reduces and divides one patch per blob in a Python
loop, spread over a process pool in chunks of 100 planes; here the image is on the device (or goes up in chunks of
whole planes) and ``mmx_extract_patches`` gathers every patch of a batch in one launch, bit-equal to NumPy's arithmetic.
The model itself is PyTorch's: a TorchScript archive (``torch.jit.load``) that takes ``(N, 1, H, W)`` float32 patches
with values in [0, 1] and returns one score per patch.  A Keras model is still loaded the reference's way where
``tensorflow`` is installed.  A NumPy ``roi`` without a GPU takes the host statement of the same formula
(:func:`extract_patches`), which is what the tests compare the kernel with.
"""
from __future__ import annotations

import os
from time import time
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from . import config, detector

_logger = config.logger.getChild(__name__)

#: patches cut and scored per step: one kernel launch and one forward pass of the model (64 MiB of float32 patches of
#: size 16); tests lower it
PATCH_BATCH = 65536


def _extents(size: int) -> Tuple[int, int]:
    """``(back, fwd)``: a patch is rows ``[y - back, y + fwd)`` and columns ``[x - back, x + back)`` -- ``back`` on
    BOTH sides along x, so an odd size has one column less than rows (the reference's extent, kept as it is)."""
    size = int(size)
    if size < 2 or size > nat.MMX_PATCH_MAX_SIZE:
        raise ValueError(f"patch size {size} outside [2, {nat.MMX_PATCH_MAX_SIZE}]")
    return size // 2, -(size // -2)


def _blob_coords(blobs) -> np.ndarray:
    zyx = np.asarray(blobs)[:, :3].astype(int)
    return zyx.reshape(-1, 3)


def _check_patches(zyx: np.ndarray, size: int, shape3, z_lo: int = 0, z_hi: Optional[int] = None) -> None:
    """Every patch inside ``(nz, ny, nx)`` (planes ``[z_lo, z_hi)`` of it), or ``ValueError``: where the reference fails
    on an empty slice or a ragged stack, and the kernel's precondition -- checked on the host before anything runs."""
    back, fwd = _extents(size)
    nz, ny, nx = (int(v) for v in shape3[:3])
    z_hi = nz if z_hi is None else z_hi
    if len(zyx) == 0:
        raise ValueError("need at least one blob to extract patches for")
    z, y, x = zyx[:, 0], zyx[:, 1], zyx[:, 2]
    bad = (z < z_lo) | (z >= z_hi) | (y < back) | (y + fwd > ny) | (x < back) | (x + back > nx)
    if np.any(bad):
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"the size-{size} patch of blob {i} at {tuple(int(v) for v in zyx[i])} leaves planes "
                         f"[{z_lo}, {z_hi}) of a region of shape {(nz, ny, nx)} ({int(bad.sum())} of {len(zyx)} do)")


def _extract_patches_host(roi: np.ndarray, zyx: np.ndarray, size: int) -> np.ndarray:
    """The formula on the host: ``patch = roi[z, y - back : y + fwd, x - back : x + back, ...]``, ``patch / max(patch)``
    for every blob at once.  NumPy's true divide gives float64 for integer and float64 voxels and float32 for float32
    ones, its maximum propagates NaN, and 0 / 0 is NaN."""
    back, fwd = _extents(size)
    rows = np.arange(-back, fwd)
    cols = np.arange(-back, back)
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for lo in range(0, len(zyx), PATCH_BATCH):
            part = zyx[lo:lo + PATCH_BATCH]
            patch = roi[part[:, 0, None, None], part[:, 1, None, None] + rows[:, None], part[:, 2, None, None] + cols]
            peak = np.max(patch.reshape(len(part), -1), axis=1)
            out.append(patch / peak.reshape((-1,) + (1,) * (patch.ndim - 1)))
    x = out[0] if len(out) == 1 else np.concatenate(out)
    return x.reshape(x.shape + (1,))


def _as_device_volume(roi):
    """A ``DeviceVolume`` as it is, a device tensor wrapped in one (no copy), ``None`` for anything on the host."""
    from . import volume
    import torch
    if isinstance(roi, volume.DeviceVolume):
        return roi
    if isinstance(roi, torch.Tensor) and roi.device.type == "cuda":
        return volume.DeviceVolume(roi, device=roi.device)
    return None


def _patches_device(dvol, channel: int, zyx: np.ndarray, size: int, ref: bool = True, f32: bool = False):
    """``mmx_extract_patches`` for blobs ``zyx`` (host, already checked) of one channel of ``dvol``: ``(ref, f32)``
    device tensors ``(N, size_y, size_x)`` -- the reference's dtype / the float32 model copy -- or ``None`` each."""
    import torch
    back, fwd = _extents(size)
    dev = dvol.tensor.device
    n = len(zyx)
    if not 0 <= int(channel) < dvol.n_channels:
        raise ValueError(f"channel {channel} of an image with {dvol.n_channels}")
    out_dtype = torch.float32 if dvol.np_dtype == np.float32 else torch.float64
    shape = (n, back + fwd, 2 * back)
    d_ref = torch.empty(shape, dtype=out_dtype, device=dev) if ref else None
    d_f32 = torch.empty(shape, dtype=torch.float32, device=dev) if f32 else None
    d_zyx = torch.from_numpy(np.ascontiguousarray(zyx, dtype=np.int32)).to(dev)
    dvol.stream_wait(boxes=[(int(zyx[:, 0].min()), int(zyx[:, 0].max()) + 1, 0, int(dvol.shape[1]))])
    vol = dvol.view(channel, False)
    nat.check(nat.lib().mmx_extract_patches(vol, d_zyx.data_ptr(), n, int(size),
                                            d_ref.data_ptr() if ref else None, d_f32.data_ptr() if f32 else None,
                                            torch.cuda.current_stream(dev).cuda_stream), "mmx_extract_patches")
    return d_ref, d_f32


def _held_planes(dvol) -> Tuple[int, int]:
    return int(dvol.z_off), int(dvol.z_off) + int(dvol.tensor.shape[0])


def extract_patches(roi, blobs, size: int = 16, channel: Optional[int] = None):
    """One 2-D patch per blob, each divided by its own maximum -> ``(N, size_y, size_x, 1)``.

    ``roi``: ``(z, y, x[, c])``.  A NumPy array takes the host statement of the formula and returns a NumPy array (a 4-D
    ``roi`` gives patches that keep their channel axis and share one maximum, as in the reference).  A
    ``DeviceVolume`` or a device tensor goes through the HIP kernel and returns a device tensor; a multichannel one
    needs ``channel`` (an extension: the reference's callers hand over ``roi[..., chl]``).  ``blobs``: rows of
    ``z, y, x, ...``, truncated to integers.  float64 for integer and float64 voxels, float32 for float32 ones.  In both
    paths a patch that would leave the roi raises ``ValueError`` before anything is computed."""
    zyx = _blob_coords(blobs)
    dvol = _as_device_volume(roi)
    if dvol is None:
        roi = np.asarray(roi)
        _check_patches(zyx, size, roi.shape)
        return _extract_patches_host(roi, zyx, size)
    if dvol.multichannel and channel is None:
        raise ValueError("a multichannel device image needs `channel`")
    if dvol.y_off or int(dvol.tensor.shape[1]) != int(dvol.shape[1]):
        raise ValueError("patches are cut from whole planes: this volume holds some rows only")
    _check_patches(zyx, size, dvol.shape, *_held_planes(dvol))
    d_ref, _ = _patches_device(dvol, channel or 0, zyx, size)
    return d_ref.unsqueeze(-1)


def _model_device(model):
    try:
        return next(iter(model.parameters())).device
    except (AttributeError, StopIteration, TypeError):
        return None


def _scores_torch(model, x32):
    """Scores of a callable model for float32 patches ``(N, size_y, size_x)`` (a tensor on the device the model is to
    run on): ``(N, 1, size_y, size_x)`` batches of ``PATCH_BATCH`` under ``no_grad`` -> an ``(N, ...)`` tensor."""
    import torch
    out = []
    step = max(1, int(PATCH_BATCH))
    with torch.no_grad():
        for lo in range(0, len(x32), step):
            batch = x32[lo:lo + step].unsqueeze(1)
            out.append(torch.as_tensor(model(batch)).reshape(len(batch), -1))
    return out[0] if len(out) == 1 else torch.cat(out)


def _is_keras(model) -> bool:
    return hasattr(model, "predict")


def classify_patches(model, x, thresh: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """``(y_pred, y_score)`` of patches ``x`` as :func:`extract_patches` returns them.

    A model with ``.predict`` is called as the reference calls Keras: ``predict(x)`` on the host array.  Any other
    callable (a ``torch.nn.Module``, a TorchScript module) is fed float32 ``(N, 1, size_y, size_x)`` tensors in batches
    of ``PATCH_BATCH`` under ``torch.no_grad()`` -- on the device ``x`` lives on, or the model's for a host ``x``.
    Scores are squeezed; ``y_pred = (y_score > thresh)`` as int, so a NaN score gives 0."""
    import torch
    if _is_keras(model):
        if isinstance(x, torch.Tensor):
            x = x.cpu().numpy()
        y_score = np.asarray(model.predict(x)).squeeze()
    else:
        if isinstance(x, torch.Tensor):
            t = x
        else:
            t = torch.from_numpy(np.ascontiguousarray(x))
            dev = _model_device(model)
            if dev is not None:
                t = t.to(dev)
        if t.ndim == 4 and t.shape[-1] == 1:
            t = t.squeeze(-1)
        y_score = _scores_torch(model, t.to(torch.float32)).cpu().numpy().squeeze()
    y_pred = (y_score > thresh).astype(int).squeeze()
    return y_pred, y_score


def _roi_geometry(img_shape, subimg_offset, subimg_size, patch_size: int):
    """The boxes of :func:`setup_classification_roi` (reference :110-142) for an image of ``img_shape`` (z, y, x):
    ``(border_near, border_far, blobs_near, blobs_far, subimg_offset)``.  The sub-image is clipped to the image and
    grown by ``patch_size // 2`` in y and x for the patches of blobs at its edge; where the image ends before that
    border does, the box in which blobs are classified shrinks by the missing part instead."""
    shape = np.asarray(img_shape[:3], dtype=int)
    offset = np.asarray(subimg_offset, dtype=int)
    far = np.minimum(offset + np.asarray(subimg_size, dtype=int), shape)
    border = np.array((0, patch_size // 2, patch_size // 2))
    near_full = offset - border
    far_full = far + border
    border_near = np.maximum(near_full, 0)
    border_far = np.minimum(far_full, shape)
    blobs_near = np.where(near_full < 0, -near_full, offset)
    blobs_far = np.where(far_full > shape, 2 * shape - far_full, far)
    return border_near, border_far, blobs_near, blobs_far, offset


def _roi_mask(blobs: "detector.Blobs", geom, blobs_relative: bool):
    border_near, _, blobs_near, blobs_far, offset = geom
    rel_offset = blobs_near - offset if blobs_relative else blobs_near
    _, mask = detector.get_blobs_in_roi(blobs.blobs, rel_offset, blobs_far - blobs_near, reverse=False)
    return mask, offset - border_near


def setup_classification_roi(image5d, subimg_offset: Sequence[int], subimg_size: Sequence[int],
                             blobs: "detector.Blobs", patch_size: int, blobs_relative: bool = False):
    """``(roi, blobs_roi_mask, blobs_shift)``: the sub-image with its patch border (a view of ``image5d[0]``), the rows of
    ``blobs`` that are classified in it, and what to add to their coordinates (after taking ``subimg_offset`` off
    absolute ones) to address ``roi``."""
    geom = _roi_geometry(image5d.shape[1:4], subimg_offset, subimg_size, patch_size)
    border_near, border_far = geom[:2]
    roi = image5d[0][tuple(slice(int(a), int(b)) for a, b in zip(border_near, border_far))]
    mask, shift = _roi_mask(blobs, geom, blobs_relative)
    return roi, mask, shift


def load_model(path, device=None):
    """The model behind ``path``: a callable is used as it is (an extension); a TorchScript archive is loaded with
    ``torch.jit.load(path, map_location=device)``; any other file is loaded the reference's way when ``tensorflow``
    imports, and is a ``ModuleNotFoundError`` when it does not."""
    import torch
    if callable(path) or _is_keras(path):
        return path
    if not os.path.exists(path):
        raise IOError(f"classifier model {path} does not exist")
    try:
        model = torch.jit.load(path, map_location=device)
        model.eval()
        return model
    except (RuntimeError, ValueError) as exc:
        _logger.debug("%s is no TorchScript archive (%s)", path, exc)
    try:
        from tensorflow.keras.models import load_model as keras_load_model
    except ModuleNotFoundError:
        raise ModuleNotFoundError(
            "Tensorflow is required for classification with a model that is no TorchScript archive. Please install, "
            "eg with 'pip install tensorflow', or export the model with torch.jit.save.") from None
    return keras_load_model(path)


def _use_device(image) -> bool:
    """Whether patches of ``image`` are cut by the kernel: a GPU is visible and the voxels are of a type it reads.
    Without a GPU, and for other voxel types (which NumPy divides as they are), the host statement of the formula runs."""
    import torch
    from . import volume
    if isinstance(image, volume.DeviceVolume) or (isinstance(image, torch.Tensor) and image.device.type == "cuda"):
        return True
    if not torch.cuda.is_available():
        return False
    if np.dtype(image.dtype) not in volume._NP_TO_MMX:
        _logger.warning("classifier: %s voxels are not read on the device, cutting patches on the host", image.dtype)
        return False
    return True


def _predict_device(model, dvol, channel: int, zyx: np.ndarray, size: int) -> np.ndarray:
    """Predictions (int, ``(N,)``) for blobs ``zyx`` of one channel of a device volume: per ``PATCH_BATCH`` blobs one
    launch of the patch kernel and one pass of the model."""
    _check_patches(zyx, size, dvol.shape, *_held_planes(dvol))
    keras = _is_keras(model)
    preds = []
    step = max(1, int(PATCH_BATCH))
    for lo in range(0, len(zyx), step):
        d_ref, d_f32 = _patches_device(dvol, channel, zyx[lo:lo + step], size, ref=keras, f32=not keras)
        y_pred, _ = classify_patches(model, d_ref.unsqueeze(-1) if keras else d_f32)
        preds.append(np.atleast_1d(y_pred))
    return np.concatenate(preds)


def _predict_host(model, roi_chl: np.ndarray, zyx: np.ndarray, size: int) -> np.ndarray:
    y_pred, _ = classify_patches(model, extract_patches(roi_chl, zyx, size))
    return np.atleast_1d(y_pred)


def classify_blobs(path, image5d, subimg_offset: Sequence[int], subimg_size: Sequence[int], channels: Sequence[int],
                   blobs: "detector.Blobs", patch_size: int = 16, blobs_relative: bool = False):
    """Classify the blobs of one sub-image by the image patches around them; the predictions go into the ``confirmed``
    column of ``blobs.blobs``.  Returns ``(blobs_roi_mask, classifications)``: the rows inside the sub-image and their
    ``confirmed`` values.  ``path``: a TorchScript (or Keras) model file, or the model itself.  With a GPU the
    sub-image goes to the device and the kernel cuts the patches; without one the host formula does."""
    import torch
    roi, roi_mask, shift = setup_classification_roi(image5d, subimg_offset, subimg_size, blobs, patch_size,
                                                    blobs_relative)
    on_device = _use_device(roi)
    dev = torch.device("cuda", torch.cuda.current_device()) if on_device else torch.device("cpu")
    model = load_model(path, dev)
    dvol = None
    try:
        for chl in channels:
            _logger.info("Classifying blobs in channel: %s", chl)
            _, chl_mask = blobs.blobs_in_channel(blobs.blobs, chl, True)
            mask = np.logical_and(roi_mask, chl_mask)
            if np.sum(mask) < 1:
                continue
            coords = np.add(blobs.blobs[mask, :3], shift)
            if not blobs_relative:
                coords -= np.asarray(subimg_offset)
            zyx = _blob_coords(coords)
            if on_device:
                if dvol is None:
                    from . import volume
                    dvol = volume.DeviceVolume(roi, device=dev, streamed=False)
                y_pred = _predict_device(model, dvol, chl if dvol.multichannel else 0, zyx, patch_size)
            else:
                y_pred = _predict_host(model, roi if roi.ndim < 4 else roi[..., chl], zyx, patch_size)
            blobs.set_blob_confirmed(blobs.blobs, y_pred, mask=mask)
    finally:
        if dvol is not None:
            dvol.close()
    return roi_mask, blobs.get_blob_confirmed(blobs.blobs)[roi_mask]


def _plane_chunks(img, limit: int):
    """``[(z_lo, z_hi)]``: runs of whole planes of a host ``(z, y, x[, c])`` image of at most ``limit / 2`` bytes (one
    chunk is read while the next goes up); a single plane may exceed it."""
    from .stack_detect import _image_bytes
    nz = int(img.shape[0])
    plane = max(1, _image_bytes(img) // max(1, nz))
    step = max(1, (int(limit) // 2) // plane)
    return [(z, min(z + step, nz)) for z in range(0, nz, step)]


class ClassifyImage:
    """Whole-image classification (reference :221-352).  The reference shares the image and the table with its worker
    processes through these class attributes; here :meth:`classify_chunk` reads them, and nothing forks."""
    image5d = None
    blobs = None

    @classmethod
    def classify_whole_image(cls, model_path=None, image5d=None, channels: Optional[Sequence[int]] = None,
                             blobs: Optional["detector.Blobs"] = None, **kwargs):
        """Classify every blob of ``blobs`` whose patch lies inside the image, channel by channel of ``channels``.

        Defaults as in the reference: ``config.classifier.model``, ``config.img5d.img``, the channels of
        ``config.channel``, ``config.blobs``; ``FileNotFoundError`` when there is no model, image or table.
        ``image5d``: ``(t, z, y, x[, c])``, the first time point is read; a ``DeviceVolume`` of it is taken as it is.
        ``kwargs``: ``patch_size`` (16), ``blobs_relative``.  A blob is classified iff
        ``patch_size // 2 <= y < ny - patch_size // 2``, the same in x, and ``0 <= z < nz``; the others keep their
        ``confirmed`` value.

        On the device: one pass per channel over all selected blobs when the image is resident or fits
        ``stack_detect._resident_limit()``, otherwise chunks of whole planes with the next chunk on its way up
        meanwhile -- patches lie in one plane, so no halo is needed and the results are the same either way, and the
        same as the reference's walk in chunks of 100 planes.  Under a process group every rank classifies the whole
        table itself: no collectives."""
        import torch
        from . import stack_detect, volume
        if not model_path:
            model_path = config.classifier.model
            if not model_path:
                raise FileNotFoundError("No classifier model found")
        if image5d is None and config.img5d is not None:
            image5d = config.img5d.img
        if image5d is None:
            raise FileNotFoundError("No image found")
        resident = image5d if isinstance(image5d, volume.DeviceVolume) else None
        img = None if resident is not None else image5d[0]
        shape = resident.shape if resident is not None else img.shape
        if channels is None:
            channels = detector._channels_of(len(shape) + 1, shape[3] if len(shape) > 3 else 1, config.channel, 4)[1]
        if blobs is None:
            blobs = config.blobs
            if blobs is None:
                raise FileNotFoundError("No blobs found")
        patch_size = int(kwargs.pop("patch_size", 16))
        blobs_relative = bool(kwargs.pop("blobs_relative", False))
        if kwargs:
            raise TypeError(f"unexpected arguments {sorted(kwargs)}")
        start = time()
        geom = _roi_geometry(shape[:3], (0, 0, 0), shape[:3], patch_size)
        roi_mask, _ = _roi_mask(blobs, geom, blobs_relative)     # (offset 0: the coordinates address the image as they are)
        on_device = resident is not None or _use_device(img)
        dev = (resident.tensor.device if resident is not None else
               torch.device("cuda", torch.cuda.current_device()) if on_device else torch.device("cpu"))
        model = load_model(model_path, dev)
        jobs = []                                           # (channel, row mask, coordinates)
        for chl in channels:
            _, chl_mask = blobs.blobs_in_channel(blobs.blobs, chl, True)
            mask = np.logical_and(roi_mask, chl_mask)
            if np.sum(mask) >= 1:
                jobs.append((chl, mask, _blob_coords(blobs.blobs[mask])))
        _logger.info("Classifying whole image: %s blobs in %s channels", sum(len(j[2]) for j in jobs), len(jobs))
        if not jobs:
            return
        if not on_device:
            for chl, mask, zyx in jobs:
                blobs.set_blob_confirmed(blobs.blobs, _predict_host(model, img if img.ndim < 4 else img[..., chl], zyx,
                                                                    patch_size), mask=mask)
        elif resident is not None or stack_detect._image_bytes(img) <= stack_detect._resident_limit():
            dvol = resident if resident is not None else volume.DeviceVolume(img, device=dev, streamed=True)
            try:
                for chl, mask, zyx in jobs:
                    blobs.set_blob_confirmed(
                        blobs.blobs, _predict_device(model, dvol, chl if dvol.multichannel else 0, zyx, patch_size),
                        mask=mask)
            finally:
                if resident is None:
                    dvol.close()
        else:
            cls._classify_plane_chunks(model, img, dev, jobs, blobs, patch_size, stack_detect._resident_limit())
        _logger.debug("Time elapsed to classify whole image: %s", time() - start)

    @staticmethod
    def _classify_plane_chunks(model, img, dev, jobs, blobs, patch_size: int, limit: int) -> None:
        """A host image too large to be resident: chunk k is a ``DeviceVolume`` of planes ``[z_lo, z_hi)`` that answers
        for the whole image, chunk k + 1 is on its way up while the blobs of chunk k are classified."""
        from . import volume
        chunks = _plane_chunks(img, limit)
        preds = [np.zeros(len(zyx), dtype=int) for _, _, zyx in jobs]

        def upload(k):
            z_lo, z_hi = chunks[k]
            return volume.DeviceVolume(img[z_lo:z_hi], device=dev, streamed=True, z_off=z_lo, full_shape=img.shape[:3])

        nxt = upload(0)
        try:
            for k, (z_lo, z_hi) in enumerate(chunks):
                cur, nxt = nxt, None
                try:
                    if k + 1 < len(chunks):
                        nxt = upload(k + 1)
                    for j, (chl, _, zyx) in enumerate(jobs):
                        rows = np.flatnonzero((zyx[:, 0] >= z_lo) & (zyx[:, 0] < z_hi))
                        if len(rows):
                            preds[j][rows] = _predict_device(model, cur, chl if cur.multichannel else 0, zyx[rows],
                                                             patch_size)
                finally:
                    cur.close()
        finally:
            if nxt is not None:
                nxt.close()
        for (_, mask, _), pred in zip(jobs, preds):
            blobs.set_blob_confirmed(blobs.blobs, pred, mask=mask)

    @classmethod
    def classify_chunk(cls, model_path, subimg_offset: Sequence[int], subimg_size: Sequence[int],
                       channels: Sequence[int], **kwargs):
        """:func:`classify_blobs` on one sub-image of :attr:`image5d` with :attr:`blobs` ->
        ``(subimg_offset, blobs_mask, classifications)``.  The reference's workers reopen the image through its CLI when
        the attributes are unset; here that is a ``FileNotFoundError``."""
        if cls.image5d is None or cls.blobs is None:
            raise FileNotFoundError("No image found: set ClassifyImage.image5d and ClassifyImage.blobs")
        mask, classifications = classify_blobs(model_path, cls.image5d, subimg_offset, subimg_size, channels,
                                               cls.blobs, **kwargs)
        return subimg_offset, mask, classifications
