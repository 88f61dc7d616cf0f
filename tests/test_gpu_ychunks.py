"""Images whose block layers exceed the device: ``DeviceVolume`` as a box of planes AND rows of a larger volume, the
staged upload of such a box straight out of a memory map (source plane pitch), and the stack detected y-chunk by y-chunk
(``stack_detect._zy_chunks``) against the resident image and the oracle."""
import threading

import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _two_channels(c0, seed, n_blobs):
    from magellanmapper_amd import synth
    other = synth.make_volume(seed, c0.shape, n_blobs)
    return np.stack((c0, np.maximum(other, (c0.astype(np.int32) * 7 // 10).astype(c0.dtype))), axis=-1)


@pytest.fixture(scope="module")
def big():
    from magellanmapper_amd import synth
    return synth.make_volume(31, (24, 64, 48), 30)


# blocks inside planes [5, 17) and rows [9, 40): the whole box, its corners, an odd-sized one in the middle
BOX = (slice(5, 17), slice(9, 40))
BOX_ORIGINS = [(5, 9, 0), (5, 9, 0), (6, 21, 7), (8, 20, 16), (5, 30, 3)]
BOX_SHAPES = [(12, 31, 48), (7, 13, 20), (9, 17, 33), (9, 20, 32), (12, 10, 45)]


@pytest.mark.parametrize("channels", [1, 2])
def test_a_box_of_planes_and_rows_answers_for_the_whole_volume(gpu, big, channels):
    """``DeviceVolume(big[5:17, 9:40], z_off=5, y_off=9, full_shape=...)``: LoG cubes and blobs of blocks inside the box
    equal the whole resident volume's bit for bit (the kernels address ``origin . strides`` from a base pointer shifted
    back by the offsets); a block that leaves the box is refused, and so are order statistics, which take whole planes."""
    from magellanmapper_amd import _native as nat, blob_log as bl, config, roi_prof, stack_detect
    img = big if channels == 1 else _two_channels(big, 32, 20)
    whole = bl.DeviceVolume(img)
    part = bl.DeviceVolume(img[BOX], z_off=5, y_off=9, full_shape=img.shape[:3])
    assert part.shape == whole.shape and part.tensor.shape[:2] == (12, 31) and (part.z_off, part.y_off) == (5, 9)
    assert bl.DeviceVolume(img[BOX], z_off=5, y_off=9, full_shape=img.shape).shape == whole.shape
    space = bl.ScaleSpace.make(2.0, 3.0, 2)
    n_blobs = 0
    for c in range(channels):
        want = bl.log_cube_blocks(whole, c, BOX_ORIGINS, BOX_SHAPES, space)
        got = bl.log_cube_blocks(part, c, BOX_ORIGINS, BOX_SHAPES, space)
        for w, g in zip(want, got):
            np.testing.assert_array_equal(g, w)
        assert max(float(np.abs(w).max()) for w in want) > 0
        want, want_peaks = bl.blob_log_blocks(whole, c, BOX_ORIGINS, BOX_SHAPES, 2.0, 3.0, 2, 0.05, 0.5, return_peaks=True)
        got, got_peaks = bl.blob_log_blocks(part, c, BOX_ORIGINS, BOX_SHAPES, 2.0, 3.0, 2, 0.05, 0.5, return_peaks=True)
        for w, g, wp, gp in zip(want, got, want_peaks, got_peaks):
            np.testing.assert_array_equal(g, w)
            np.testing.assert_array_equal(gp[0], wp[0])
            np.testing.assert_array_equal(gp[1], wp[1])
        n_blobs += sum(len(w) for w in want)
    assert n_blobs > 5
    # blocks that leave the box
    for origin, shape in (((5, 8, 0), (12, 20, 48)), ((5, 30, 0), (12, 11, 48)), ((4, 9, 0), (5, 5, 5))):
        with pytest.raises(ValueError, match="holds"):
            bl.log_cube_blocks(part, 0, [origin], [shape], space)
    # the box must lie inside the volume, x and channels whole
    for kw in (dict(z_off=5, y_off=34), dict(z_off=13, y_off=9), dict(z_off=5, y_off=-1)):
        with pytest.raises(ValueError, match="do not lie"):
            bl.DeviceVolume(img[BOX], full_shape=img.shape[:3], **kw)
    with pytest.raises(ValueError, match="do not lie"):
        bl.DeviceVolume(img[BOX][:, :, :40], z_off=5, y_off=9, full_shape=img.shape[:3])
    # order statistics are over whole planes
    with pytest.raises(ValueError, match="whole planes"):
        part.order_stats(0, [0, 1, 2, 3])
    with pytest.raises(ValueError, match="whole planes"):
        bl.DeviceVolume(img[5:17, :40], z_off=5, full_shape=img.shape[:3]).order_stats(0, [0, 1, 2, 3], [(5, 6)])
    # a stack handed a volume that lacks rows its blocks touch is refused before any kernel runs
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    bk = stack_detect.setup_blocks(roi_prof.ROIProfile(segment_size=40, denoise_size=None), img.shape[:3])
    rows = bl.DeviceVolume(img[:, 9:40], y_off=9, full_shape=img.shape[:3])
    with pytest.raises(nat.MmxError, match=r"rows \[9, 40\) but this rank's blocks touch planes \[0, 24\) and rows \[0, 64\)"):
        stack_detect.StackDetector.detect_blobs_sub_rois(None, rows, bk.sub_roi_slices, bk.sub_rois_offsets, None, None,
                                                         False, [0])


@pytest.mark.parametrize("channels", [1, 2])
def test_a_box_of_a_memory_map_goes_up_from_where_it_lies(gpu, monkeypatch, tmp_path, channels):
    """``_SlabUpload`` of ``mm[z_lo:z_hi, y_lo:y_hi]``: planes a whole image plane apart.  The one native call
    (``mmx_host_stage_upload_pitched``) and the Python loop both land the box's bytes, in z-slabs and in y-band cells;
    ``close()`` in the middle ends the call at the next region and leaves no staging thread."""
    from magellanmapper_amd import _native as nat, blob_log as bl, volume
    from magellanmapper_amd.buffers import _NativeEvent
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    rng = np.random.default_rng(12)
    data = rng.integers(0, 65535, (70, 96, 64) + ((2,) if channels == 2 else ())).astype(np.uint16)
    np.save(tmp_path / "img.npy", data)
    mm = np.load(tmp_path / "img.npy", mmap_mode="r")
    box = mm[7:61, 13:90]
    assert not box.flags.writeable and not box.flags.c_contiguous and isinstance(box, np.memmap)
    assert volume._plane_pitch(box) == data[0].nbytes
    want = torch.from_numpy(np.ascontiguousarray(data[7:61, 13:90])).view(torch.int16)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 5 * box[0].nbytes)
    for cells in (None, ([30, 54], [40, 77])):
        for native in (True, False):
            monkeypatch.setattr(volume, "NATIVE_STAGING", native)
            dv = bl.DeviceVolume(box, streamed=True, cells=cells, z_off=7, y_off=13, full_shape=data.shape[:3])
            up = dv._upload
            assert up is not None and len(up.regions) > 2 and (cells is None or any(r[2] > 0 for r in up.regions))
            side = torch.cuda.Stream()
            # (coordinates of the whole image: planes [7, 19), rows [13, 43) are the box's first 12 x 30)
            dv.stream_wait(None, [side], [(7, 19, 13, 43)])
            with torch.cuda.stream(side):
                head = dv.tensor[:12, :30].clone()
            dv.wait_all()
            side.synchronize()
            assert up.all_queued() and up.thread is None and isinstance(up._events[0], _NativeEvent) == native
            assert torch.equal(dv.tensor.cpu().view(torch.int16), want)
            assert torch.equal(head.cpu().view(torch.int16), want[:12, :30])
            assert dv.shape[:3] == data.shape[:3] and tuple(dv.tensor.shape[:2]) == (54, 77)
    # cancelled in flight: the call returns, whatever was queued has landed intact, later planes are refused
    monkeypatch.setattr(volume, "NATIVE_STAGING", True)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", box[0].nbytes)
    dv = bl.DeviceVolume(box, streamed=True, z_off=7, y_off=13, full_shape=data.shape[:3])
    up = dv._upload
    dv.stream_wait(7 + 3)
    dv.close()
    assert up.thread is None and (up.cancelled or up.all_queued()) and 3 <= up.n_queued <= up.n_slabs
    assert not [t for t in threading.enumerate() if t.name == "mmx-upload" and t.is_alive()]
    torch.cuda.synchronize()
    n = up.bounds[up.n_queued - 1]
    assert torch.equal(up.out[:n].cpu().view(torch.int16), want[:n])
    if not up.all_queued():
        with pytest.raises(nat.MmxError, match="cancelled"):
            up.event_for(len(box))
    # a source the native loop cannot read in place (rows cut as well) takes the Python loop and still lands
    odd = mm[7:61, 13:90, 3:50]
    assert volume._plane_pitch(odd) is None
    dv = bl.DeviceVolume(odd, streamed=True)
    dv.wait_all()
    assert torch.equal(dv.tensor.cpu().view(torch.int16),
                       torch.from_numpy(np.ascontiguousarray(data[7:61, 13:90, 3:50])).view(torch.int16))


def _row_limit(shape3, row_bytes):
    """``MAX_RESIDENT_BYTES`` = 2 x the bytes of the two thickest adjacent block rows of the thickest layer, from
    ``setup_blocks``: every layer thicker than ``85 / 230`` of that exceeds ``limit // 2``, every run of two block rows
    fits."""
    from magellanmapper_amd import config, stack_detect
    bk = stack_detect.setup_blocks(config.get_roi_profile(0), shape3)
    gz, gy = bk.sub_roi_slices.shape[:2]
    layers = [bk.sub_roi_slices[(l, 0, 0)][0].indices(shape3[0])[:2] for l in range(gz)]
    rows = [bk.sub_roi_slices[(0, j, 0)][1].indices(shape3[1])[:2] for j in range(gy)]
    thick = max(b - a for a, b in layers)
    pair = max(d[1] - c[0] for c, d in zip(rows, rows[1:]))
    return 2 * thick * pair * row_bytes, layers, rows


@pytest.mark.parametrize("ahead", ["1", "0"])
@pytest.mark.parametrize("channels,denoise", [(1, None), (1, 25), (2, 25), (2, None)])
@pytest.mark.parametrize("shape", [(90, 230, 80), (30, 230, 80)])
def test_a_stack_whose_layers_exceed_the_device_is_detected_y_chunk_by_y_chunk(gpu, monkeypatch, tmp_path, shape, channels,
                                                                              denoise, ahead):
    """A memory-mapped stack whose block layers do not fit ``MAX_RESIDENT_BYTES // 2`` goes up in boxes of whole block
    rows (``DeviceVolume(z_off=, y_off=)``), the next box uploading while this one is detected; same final table -- and
    co-localisation flags -- as the resident image, row for row; the single-channel raw case also equals the oracle.  The
    (30, 230, 80) stack is ONE layer of blocks, which z-chunks alone never cut.

    Of the (90, 230, 80) stack the two 45-plane layers exceed ``limit // 2`` and are cut; its last layer, planes
    [80, 90), takes 10 x 230 rows against the 45 x 85 that fit, so by the planner's rule it stays a z-chunk with all 230
    rows: the condition "no chunk volume holds all rows" is asserted for every layer that exceeds ``limit // 2``, and
    "no chunk volume is larger than ``limit // 2``" for all of them."""
    from magellanmapper_amd import blob_log as bl, config, stack_detect, synth, volume
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(stack_detect, "PRUNE_AHEAD", ahead)
    vol = synth.make_volume(81, shape, 60 * shape[0] // 30)
    if channels == 2:
        vol = _two_channels(vol, 82, 40 * shape[0] // 30)
    np.save(tmp_path / "big.npy", vol[None])
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(num_sigma=3, denoise_size=denoise, segment_size=40))
    for p in config.roi_profiles:
        p.update(config.roi_profile)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "big"
    monkeypatch.setattr(config, "near_max", [-1.0] * channels)
    chans = list(range(channels))

    def run():
        img5d = stack_detect.Image5d(np.load(tmp_path / "big.npy", mmap_mode="r"))
        _, _, blobs = stack_detect.detect_blobs_blocks("big", img5d, None, None, chans, False, False, True, channels > 1)
        return blobs

    made = []
    init = bl.DeviceVolume.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append((self.z_off, self.y_off, tuple(self.tensor.shape[:2]), tuple(self.shape[:3])))
    monkeypatch.setattr(bl.DeviceVolume, "__init__", spy)
    try:
        row_bytes = shape[2] * channels * 2
        limit, layers, rows = _row_limit(shape, row_bytes)
        assert len(rows) == 6 and limit // 2 < max(b - a for a, b in layers) * shape[1] * row_bytes
        monkeypatch.setattr(stack_detect, "MAX_RESIDENT_BYTES", 1 << 40)
        whole = run()
        # (blocks whose overlap prune falls back to SciPy's pair order make small volumes of their own)
        assert all(m[0] == 0 and m[1] == 0 for m in made) and made[0][2] == shape[:2]
        assert all(m[2][1] == m[3][1] for m in made)                    # every volume holds all of its rows
        del made[:]
        monkeypatch.setattr(stack_detect, "MAX_RESIDENT_BYTES", limit)
        parts = run()
        chunks = [m for m in made if m[3] == shape]                     # the volumes made for chunks of the stack
        assert chunks and all(m[2] != shape[:2] for m in chunks)
        assert len({m[1] for m in chunks if m[1] > 0}) >= 2
        for z_off, y_off, (nz, ny), _ in chunks:
            assert nz * ny * row_bytes <= limit // 2
            if nz * shape[1] * row_bytes > limit // 2:
                assert ny < shape[1]                                    # a layer that does not fit: never all 230 rows
                assert ny <= max(d[1] - c[0] for c, d in zip(rows, rows[1:]))
            assert (z_off, z_off + nz) in layers and y_off in [r[0] for r in rows]
        fitting = [m for m in chunks if m[2][1] == shape[1]]
        assert [(m[0], m[2][0]) for m in fitting] == ([(80, 10)] if shape[0] == 90 else [])
        assert whole.blobs is not None and len(whole.blobs) > (100 if shape[0] == 90 else 30)
        np.testing.assert_array_equal(parts.blobs, whole.blobs)
        if channels > 1:
            np.testing.assert_array_equal(parts.colocalizations, whole.colocalizations)
        if channels == 1 and denoise is None:
            from oracle import magmap_oracle as mmo
            want, _ = mmo.detect_blobs_blocks(vol, None, [dict(config.roi_profile)], config.resolutions)
            key = lambda t: t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]
            np.testing.assert_array_equal(key(parts.blobs), key(want))
    finally:
        config.setup_roi_profiles(None)
