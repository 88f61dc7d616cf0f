"""Host-resident volumes: the z-slab upload that runs beside the detection (``blob_log._SlabUpload``; the reference's
callers hand a memory-mapped ``image5d.npy``, magmap/io/importer.py:794, magmap/cv/stack_detect.py:386-390)."""
import numpy as np
import pytest

from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _stack(vol, denoise):
    from magellanmapper_amd import config, stack_detect
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(num_sigma=3, denoise_size=denoise, segment_size=40))
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "upload"
    img5d = stack_detect.Image5d(vol[None])
    _, _, blobs = stack_detect.detect_blobs_blocks("upload", img5d, None, None, None, False, False, True, False)
    return blobs.blobs


@pytest.mark.parametrize("denoise", [None, 25])
@pytest.mark.parametrize("source", ["pageable", "memmap", "readonly"])
def test_streamed_upload_gives_the_resident_volumes_table(gpu, monkeypatch, tmp_path, source, denoise):
    """The same stack detected from a volume that is uploaded in one synchronous copy and from one that goes up in
    slabs of 9 planes while its first blocks are already being detected (raw and per-block preprocessing): identical
    tables, and the slab path was really taken."""
    from magellanmapper_amd import blob_log as bl, config, synth, volume
    vol = synth.make_volume(17, (100, 72, 80), 60)
    try:
        monkeypatch.setattr(volume, "STREAM_UPLOAD", False)
        want = _stack(vol, denoise)
        monkeypatch.setattr(volume, "STREAM_UPLOAD", True)
        monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
        monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 9 * vol[0].nbytes)
        made = []
        init = bl._SlabUpload.__init__
        monkeypatch.setattr(bl._SlabUpload, "__init__", lambda self, *a: (init(self, *a), made.append(self))[0])
        if source == "memmap":
            np.save(tmp_path / "v.npy", vol)
            src = np.load(tmp_path / "v.npy", mmap_mode="r")
        elif source == "readonly":
            src = vol.copy()
            src.flags.writeable = False
        else:
            src = vol
        got = _stack(src, denoise)
        # (block rows ending at y = 45 and 72, layers ending at z = 45, 85, 100: the volume went up y-band by y-band within
        #  each layer of blocks, every band in pieces of at most 9 planes' worth of bytes)
        assert made and made[0].n_slabs >= 12 and made[0].all_queued()
        assert {r[2:] for r in made[0].regions} == {(0, 45), (45, 72)} and {r[0] for r in made[0].regions} >= {0, 45, 85}
        assert want is not None and got is not None
        np.testing.assert_array_equal(got, want)
    finally:
        config.setup_roi_profiles(None)


def test_a_small_host_stack_in_one_chunk_still_runs_the_stack_finisher(gpu, monkeypatch, tmp_path):
    """A small host image -- all its blocks one batch of at most ``GRAPH_BLOCKS`` -- handed over as a read-only memory map
    goes up streamed and is STILL finished by the one native call (``_StackFinisher.run`` ran and made the table): a stack
    that lost it would take the call-by-call path and give the same table, so the call is counted.  The table equals the
    one of the same image resident on the device (``DeviceVolume``) row for row, and the oracle's.
    ``synth.make_volume(23, (40, 72, 80), 40)``: seed 23, 40 blobs asked for."""
    from magellanmapper_amd import blob_log as bl, config, stack_detect, stack_tables, synth, volume
    from oracle import magmap_oracle as mmo
    vol = synth.make_volume(23, (40, 72, 80), 40)
    assert vol.dtype == np.uint16 and vol.ndim == 3
    np.save(tmp_path / "small.npy", vol[None])
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(num_sigma=3, denoise_size=None, segment_size=40))
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "small"
    ran = []
    real = stack_tables._StackFinisher.run

    def counted(self, *a, **k):
        out = real(self, *a, **k)
        ran.append((self, out))
        return out
    monkeypatch.setattr(stack_tables._StackFinisher, "run", counted)
    try:
        n_blocks = stack_detect.setup_blocks(config.roi_profile, vol.shape).sub_roi_slices.size
        assert 1 < n_blocks <= bl.GRAPH_BLOCKS
        img5d = stack_detect.Image5d(np.load(tmp_path / "small.npy", mmap_mode="r"))
        assert not img5d.img.flags.writeable
        _, _, got = stack_detect.detect_blobs_blocks("small", img5d, None, None, None, False, False, full_roi=True)
        assert len(ran) == 1 and ran[0][1] is not None and ran[0][0].result is not None
        del ran[:]
        held = stack_detect.Image5d(vol[None])
        held.device_volume = bl.DeviceVolume(vol)
        _, _, want = stack_detect.detect_blobs_blocks("small", held, None, None, None, False, False, full_roi=True)
        assert want.blobs is not None and got.blobs is not None and len(want.blobs) >= 20
        np.testing.assert_array_equal(got.blobs, want.blobs)
        ref, _ = mmo.detect_blobs_blocks(vol, None, [dict(config.roi_profile)], config.resolutions)
        key = lambda t: t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]
        np.testing.assert_array_equal(key(got.blobs), key(ref))
    finally:
        config.setup_roi_profiles(None)


def test_pinned_source_is_copied_without_staging_and_partial_waits_work(gpu, monkeypatch):
    """A pinned tensor: every slab copy is queued at construction (no thread); `stream_wait(z)` orders a stream after the
    slabs below z only, `wait_all` after everything; the device copy equals the source."""
    from magellanmapper_amd import blob_log as bl, synth, volume
    vol = synth.make_volume(3, (64, 48, 56), 10)
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 8 * vol[0].nbytes)
    src = torch.from_numpy(vol.view(np.int16)).pin_memory() if not hasattr(torch, "uint16") else \
        torch.from_numpy(vol).pin_memory()
    assert bl.DeviceVolume(src)._upload is None          # (a writeable buffer: copied before the constructor returns)
    dv = bl.DeviceVolume(src, streamed=True)
    up = dv._upload
    assert up is not None and up.thread is None and up.n_slabs == 8 and up.all_queued()
    assert up.event_for(1) is up.events[0] and up.event_for(8) is up.events[0] and up.event_for(9) is up.events[1]
    assert up.event_for(64) is up.events[-1]
    side = torch.cuda.Stream()
    dv.stream_wait(20, [side])
    with torch.cuda.stream(side):
        head = dv.tensor[:20].clone()
    dv.wait_all()
    assert dv._upload is None
    side.synchronize()
    np.testing.assert_array_equal(head.cpu().numpy().view(vol.dtype), vol[:20])
    np.testing.assert_array_equal(dv.tensor.cpu().numpy().view(vol.dtype), vol)


def test_a_failing_source_is_reported_by_the_waiter(gpu, monkeypatch):
    """An exception in the staging thread surfaces where the detection waits for the slab (not as a hang)."""
    from magellanmapper_amd import _native as nat, blob_log as bl, volume

    class Bad(np.ndarray):
        def __getitem__(self, item):
            raise OSError("disk gone")
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    src = np.zeros((8, 16, 16), dtype=np.uint16).view(Bad)
    dv = bl.DeviceVolume.__new__(bl.DeviceVolume)
    dv._upload = bl._SlabUpload(src, torch.device("cuda", 0))
    dv.shape = (8, 16, 16)
    with pytest.raises(nat.MmxError, match="upload of the image failed"):
        dv.stream_wait(8)


@pytest.mark.parametrize("denoise", [None, 25])
def test_three_tiles_streamed_equal_the_oracle_per_tile(gpu, monkeypatch, tmp_path, denoise):
    """`stack_detect.detect_blobs_tiles`: three tiles of a stack as memory-mapped image5d files, tile k + 1 uploading
    (in slabs) while tile k is detected, device buffers reused -- every tile's table equals the oracle's for that tile."""
    from magellanmapper_amd import blob_log as bl, config, stack_detect, synth, volume
    from oracle import magmap_oracle as mmo
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 16 * 64 * 72 * 2)
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(num_sigma=3, denoise_size=denoise, segment_size=40))
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "tiles"
    vols, tiles = [], []
    for k in range(3):
        v = synth.make_volume(40 + k, (70, 64, 72), 40)
        np.save(tmp_path / f"t{k}.npy", v[None])
        vols.append(v)
        tiles.append(stack_detect.Image5d(np.load(tmp_path / f"t{k}.npy", mmap_mode="r")))
    uploads = []
    init = bl._SlabUpload.__init__
    monkeypatch.setattr(bl._SlabUpload, "__init__", lambda self, *a: (init(self, *a), uploads.append(self))[0])
    key = lambda t: t[np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))]
    try:
        seen = []
        for k, blobs in stack_detect.detect_blobs_tiles("tiles", tiles):
            if k < 2:
                assert len(uploads) == k + 2          # tile k + 1 was queued before tile k's table came back
            want, _ = mmo.detect_blobs_blocks(vols[k], None, [dict(config.roi_profile)], config.resolutions)
            assert want is not None and blobs.blobs is not None and blobs.blobs.shape == want.shape
            np.testing.assert_array_equal(key(blobs.blobs), key(want))
            seen.append(k)
        assert seen == [0, 1, 2] and len(uploads) == 3 and all(t.device_volume is None for t in tiles)
    finally:
        config.setup_roi_profiles(None)


def test_small_uploads_through_the_pinned_ring_arrive_intact(gpu):
    """``buffers.to_device``: arrays of up to a quarter of the ring go through consecutive pinned slots and an asynchronous
    copy (several slots for the co-localisation's blob rows of a batch), larger ones through the plain copy; the ring
    wraps without a slot being overwritten before its copy has run -- kernels queued in between keep the copies pending
    while the host moves on."""
    import torch
    from magellanmapper_amd import buffers
    dev = torch.device("cuda", 0)
    ring = buffers._UploadRing
    rng = np.random.default_rng(5)
    sizes = [1, 7, ring.SLOT_BYTES - 1, ring.SLOT_BYTES, ring.SLOT_BYTES + 1, 5 * ring.SLOT_BYTES + 3, ring.MAX_BYTES,
             ring.MAX_BYTES + 1]
    sent = []
    busy = torch.zeros(1 << 24, device=dev)
    for rep in range(40):                            # several times round the ring
        for n in sizes:
            a = rng.integers(0, 256, n, dtype=np.uint8)
            busy.add_(1.0)                           # (something for the copies to queue behind)
            sent.append((a, buffers._to_device_bytes(a, dev)))
    torch.cuda.synchronize()
    for a, t in sent:
        assert t.device.type == "cuda" and np.array_equal(t.cpu().numpy(), a)
    f = rng.standard_normal((300, 5))
    assert np.array_equal(buffers.to_device(f, dev).cpu().numpy(), f)
    assert buffers.to_device(np.zeros((0, 3)), dev).shape == (0, 3)


def test_writeable_sources_are_copied_before_the_constructor_returns(gpu, monkeypatch):
    """The default: an ordinary array or a pinned tensor may be refilled right after ``DeviceVolume(...)`` returns (a
    double-buffered tile), so it is copied synchronously; only sources nobody can write to -- read-only arrays, read-only
    memory maps -- go up in the background without being asked."""
    from magellanmapper_amd import blob_log as bl, synth, volume
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 4 * 48 * 56 * 2)
    vol = synth.make_volume(8, (40, 48, 56), 10)
    keep = vol.copy()
    dv = bl.DeviceVolume(vol)
    assert dv._upload is None
    vol[:] = 0                                      # the caller reuses its buffer at once
    np.testing.assert_array_equal(dv.tensor.cpu().numpy().view(keep.dtype), keep)
    ro = keep.copy()
    ro.flags.writeable = False
    dv2 = bl.DeviceVolume(ro)
    assert dv2._upload is not None and dv2._upload.n_slabs == 10
    dv2.wait_all()
    assert dv2._upload is None
    np.testing.assert_array_equal(dv2.tensor.cpu().numpy().view(keep.dtype), keep)
    assert bl.DeviceVolume(ro, streamed=False)._upload is None


def test_close_cancels_what_has_not_been_staged_and_joins_the_thread(gpu, monkeypatch):
    """``DeviceVolume.close`` in the middle of an upload (a share of blocks that ends early, a failed detection, an
    abandoned tile): the staging thread stops at the next slab and is joined, waiters for later planes are told, the
    slabs already queued still land, and the device block can go back to the allocator at once -- the copy stream holds
    it (``record_stream``) until its copies have run."""
    import time
    from magellanmapper_amd import _native as nat, blob_log as bl, volume

    class Slow(np.ndarray):
        def __getitem__(self, item):
            time.sleep(0.02)
            return super().__getitem__(item)
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 2 * 32 * 32 * 2)
    monkeypatch.setattr(volume, "_STAGE_THREADS", 2)
    data = np.arange(64 * 32 * 32, dtype=np.uint16).reshape(64, 32, 32)
    dv = bl.DeviceVolume.__new__(bl.DeviceVolume)
    dv._upload = up = bl._SlabUpload(data.view(Slow), torch.device("cuda", 0))
    dv.tensor, dv.shape = up.out, (64, 32, 32)
    dv.stream_wait(2)                               # the first slab has been queued
    dv.close()
    assert dv._upload is None and up.thread is None and up.cancelled
    n_done = len(up.events)
    assert 1 <= n_done < up.n_slabs
    with pytest.raises(nat.MmxError, match="cancelled"):
        up.event_for(64)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(up.out[:up.bounds[n_done - 1]].cpu().numpy().view(np.uint16),
                                  data[:up.bounds[n_done - 1]])
    dv.close()                                      # (idempotent)
    del dv, up
    fresh = torch.zeros(64 * 32 * 32, dtype=torch.int16, device="cuda")     # may take the very block just freed
    torch.cuda.synchronize()
    assert int(fresh.abs().sum().item()) == 0


def test_an_abandoned_tile_generator_releases_the_tile_it_prefetched(gpu, monkeypatch, tmp_path):
    """A consumer that stops after the first tile: the generator's clean-up cancels the upload of the tile it had
    announced and drops both device copies."""
    from magellanmapper_amd import config, stack_detect, synth, volume
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 8 * 64 * 72 * 2)
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(num_sigma=2, denoise_size=None, segment_size=40))
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "tiles"
    tiles = []
    for k in range(3):
        np.save(tmp_path / f"a{k}.npy", synth.make_volume(50 + k, (48, 64, 72), 20)[None])
        tiles.append(stack_detect.Image5d(np.load(tmp_path / f"a{k}.npy", mmap_mode="r")))
    try:
        gen = stack_detect.detect_blobs_tiles("tiles", tiles)
        k, blobs = next(gen)
        assert k == 0 and blobs.blobs is not None
        ups = [t.device_volume._upload for t in tiles[1:] if t.device_volume is not None]
        gen.close()
        assert all(t.device_volume is None for t in tiles)
        assert all(u is None or (u.thread is None and (u.cancelled or u.all_queued())) for u in ups)
    finally:
        config.setup_roi_profiles(None)


_TILE_RANK_SCRIPT = '''
import os, sys
import numpy as np
sys.path.insert(0, {root!r})
import torch
import torch.distributed as td
from magellanmapper_amd import config, dist, stack_detect, volume
from oracle import magmap_oracle as mmo

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)                            # (both ranks share the one GPU of a test box)
td.init_process_group("gloo")
try:
    c5 = {c5!r}
    volume._STREAM_MIN_BYTES = 0
    volume._STREAM_CHUNK_BYTES = 12 * 100 * 110 * (4 if c5 else 2)
    config.setup_roi_profiles(None)
    profile = dict(num_sigma=3, denoise_size=25 if c5 else None, segment_size=64)
    config.roi_profile.update(profile)
    for p in config.roi_profiles:
        p.update(profile)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "tiles"
    config.near_max = [-1.0, -1.0]
    n_tiles = 4
    tiles = [stack_detect.Image5d(np.load(os.path.join({tmp!r}, f"t{{k}}.npy"), mmap_mode="r")) for k in range(n_tiles)]
    calls = []
    real = dist.all_gather_rows
    dist.all_gather_rows = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    got = list(stack_detect.detect_blobs_tiles("tiles", tiles, coloc=c5, shard="tiles"))
    assert [k for k, _ in got] == dist.tile_share(n_tiles) == [rank, rank + 2]
    assert not calls                                # no exchange while detecting: every tile was this rank's alone
    everything = stack_detect.gather_tiles(got)
    assert calls and [k for k, _ in everything] == list(range(n_tiles))
    key = lambda t: np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))
    profiles = [dict(config.roi_profile)] * (2 if c5 else 1)
    for k, blobs in (everything if rank == 0 else got):
        vol = np.load(os.path.join({tmp!r}, f"t{{k}}.npy"))[0]
        if c5:
            want, stages = mmo.detect_blobs_blocks(vol, [0, 1], profiles, config.resolutions, near_max=[-1.0, -1.0],
                                                   coloc=True)
            np.testing.assert_array_equal(blobs.blobs, want)
            np.testing.assert_array_equal(blobs.colocalizations, stages["colocs"])
            assert set(np.unique(want[:, 6])) == {{0.0, 1.0}}
        else:
            want, _ = mmo.detect_blobs_blocks(vol, None, profiles, config.resolutions)
            assert blobs.colocalizations is None
            np.testing.assert_array_equal(blobs.blobs[key(blobs.blobs)], want[key(want)])
        assert len(want) > 30
    assert all(t.device_volume is None for t in tiles)
    torch.cuda.synchronize()
    print(f"TILE_RANK_OK {{rank}} {{[k for k, _ in got]}}", flush=True)
finally:
    td.destroy_process_group()
'''


@pytest.mark.parametrize("c5", [False, True])
def test_four_tiles_over_two_ranks_equal_the_oracle_per_tile(gpu, tmp_path, c5):
    """BASELINE.json configs[4] sharded BY TILE, as far as one GPU goes: four memory-mapped tiles over two ranks (gloo,
    sharing this GPU), ``detect_blobs_tiles(shard="tiles")`` -- rank r detects tiles r and r + 2 as one process would,
    tile r + 2 uploading while tile r is detected, no collective entered -- then ``gather_tiles``: every tile's final
    table (and, C5-shaped: two channels, per-block preprocessing, the co-localisation flags) equals the oracle's for
    that tile, on the rank that detected it and, after the gather, on rank 0 for all four."""
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    from magellanmapper_amd import synth
    for k in range(4):
        shape = (56, 100, 110)
        c0 = synth.make_volume(60 + 2 * k, shape, 45)
        if c5:
            c1 = np.maximum(synth.make_volume(61 + 2 * k, shape, 45).astype(np.int32), (c0.astype(np.int32) * 7) // 10)
            c0 = np.stack((c0, c1.astype(np.uint16)), axis=-1)
        np.save(tmp_path / f"t{k}.npy", c0[None])
    script = tmp_path / "tile_ranks.py"
    script.write_text(_TILE_RANK_SCRIPT.format(root=ROOT, tmp=str(tmp_path), c5=c5))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "TILE_RANK_OK 0 [0, 2]" in run.stdout and "TILE_RANK_OK 1 [1, 3]" in run.stdout


@pytest.mark.parametrize("source", ["pinned", "readonly"])
def test_block_row_by_block_row_upload_lands_every_voxel_and_orders_the_waits(gpu, monkeypatch, source):
    """``cells = (z ends, y ends)``: the image goes up y-band by y-band within each z-layer (``mmx_copy_rect_h2d``: a band
    is one rectangle per piece, strided on the device, strided in a pinned source or packed in the staging buffer); the
    device copy equals the source -- 3-D and (z, y, x, c) -- and a block's wait is the event of the LAST region, in upload
    order, that holds any of its voxels."""
    from magellanmapper_amd import blob_log as bl, volume
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    rng = np.random.default_rng(3)
    for shape in ((50, 60, 72), (33, 40, 24, 2)):
        data = rng.integers(0, 65535, shape).astype(np.uint16)
        plane_bytes = int(np.prod(shape[1:])) * 2
        monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 3 * plane_bytes)
        cells = ([20, 45, shape[0]], [16, 30, shape[1]])
        if source == "pinned":
            src = torch.from_numpy(data).pin_memory()
        else:
            src = data.copy()
            src.flags.writeable = False
        dv = bl.DeviceVolume(src, streamed=True, cells=cells)
        up = dv._upload
        assert up is not None and (up.thread is None) == (source == "pinned")
        regions = up.regions
        # (z, y) order: all bands of layer [0, 20) before any of [20, 45); a band wider than the chunk is cut along z
        assert regions[0][:1] + regions[0][2:] == (0, 0, 16) and regions[-1][1] == shape[0] and regions[-1][3] == shape[1]
        firsts = [i for i, r in enumerate(regions) if r[0] == 0]
        assert firsts == sorted(firsts) and max(firsts) < min(i for i, r in enumerate(regions) if r[0] >= 20)
        assert sum((r[1] - r[0]) * (r[3] - r[2]) for r in regions) == shape[0] * shape[1]       # a partition
        # a block in layer 1, row 0: waits for the last piece of band 0 of layer [20, 45) -- not for band 1 or layer 2
        want = max(i for i, r in enumerate(regions) if r[0] < 40 and r[1] > 18 and r[2] < 14 and r[3] > 0)
        assert regions[want][2:] == (0, 16) and regions[want][1] <= 45
        ev = up.event_for_boxes([(18, 40, 0, 14)])
        side = torch.cuda.Stream()
        dv.stream_wait(None, [side], [(18, 40, 0, 14)])
        with torch.cuda.stream(side):
            part = dv.tensor[18:40, 0:14].clone()
        assert ev is up.events[want]
        dv.wait_all()
        side.synchronize()
        np.testing.assert_array_equal(part.cpu().numpy().view(np.uint16), data[18:40, 0:14])
        np.testing.assert_array_equal(dv.tensor.cpu().numpy().view(np.uint16), data)
        assert dv._upload is None


def test_native_staging_loop_equals_the_python_loop_and_can_be_cancelled(gpu, monkeypatch):
    """Plain arrays and memory maps are staged by ONE native call (``mmx_host_stage_upload``: no interpreter lock between
    regions); array subclasses take the Python loop.  Both land the same bytes, z-slabs and block-row cells alike, the
    waits see the native call's progress counter, and ``close()`` in the middle ends the call at the next region."""
    from magellanmapper_amd import _native as nat, blob_log as bl, volume
    from magellanmapper_amd.buffers import _NativeEvent
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    rng = np.random.default_rng(9)
    data = rng.integers(0, 65535, (70, 96, 64)).astype(np.uint16)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", 5 * data[0].nbytes)
    ro = data.copy()
    ro.flags.writeable = False
    for cells in (None, ([30, 70], [40, 96])):
        got = {}
        for native in (True, False):
            monkeypatch.setattr(volume, "NATIVE_STAGING", native)
            dv = bl.DeviceVolume(ro, streamed=True, cells=cells)
            up = dv._upload
            side = torch.cuda.Stream()
            dv.stream_wait(None, [side], [(0, 12, 0, 30)])          # (a wait while the staging is still running)
            with torch.cuda.stream(side):
                head = dv.tensor[:12, :30].clone()
            dv.wait_all()
            side.synchronize()
            assert up.all_queued() and up.thread is None and isinstance(up._events[0], _NativeEvent) == native
            np.testing.assert_array_equal(head.cpu().numpy().view(np.uint16), data[:12, :30])
            got[native] = dv.tensor.cpu().numpy().view(np.uint16)
        np.testing.assert_array_equal(got[True], data)
        np.testing.assert_array_equal(got[False], data)
    # cancelled in flight: the call returns, whatever was queued has landed intact, later planes are refused
    monkeypatch.setattr(volume, "NATIVE_STAGING", True)
    monkeypatch.setattr(volume, "_STREAM_CHUNK_BYTES", data[0].nbytes)
    big = np.ascontiguousarray(np.broadcast_to(data, (6,) + data.shape).reshape(-1, 96, 64))
    big.flags.writeable = False
    dv = bl.DeviceVolume(big, streamed=True)
    up = dv._upload
    dv.stream_wait(3)
    dv.close()
    assert up.thread is None and (up.cancelled or up.all_queued()) and 3 <= up.n_queued <= up.n_slabs
    torch.cuda.synchronize()
    n = up.bounds[up.n_queued - 1]
    np.testing.assert_array_equal(up.out[:n].cpu().numpy().view(np.uint16), big[:n])
    if not up.all_queued():
        with pytest.raises(nat.MmxError, match="cancelled"):
            up.event_for(len(big))


@pytest.mark.parametrize("ahead", ["1", "0"])
@pytest.mark.parametrize("channels,denoise", [(1, None), (1, 25), (2, 25), (2, None)])
def test_an_image_too_large_to_be_resident_is_detected_z_chunk_by_z_chunk(gpu, monkeypatch, tmp_path, channels, denoise, ahead):
    """``stack_detect.MAX_RESIDENT_BYTES``: a memory-mapped image larger than the device may hold goes up in chunks of
    whole block layers, each a device volume of its own that answers for the whole image (``DeviceVolume(z_off=...)``), the
    next chunk uploading while this one is detected; the tables land in the one arena and are pruned once (ahead, region by
    region, or at the end).  Same final table -- and co-localisation flags -- as the resident image, row for row; the
    single-channel raw case also against the oracle."""
    from magellanmapper_amd import blob_log as bl, config, stack_detect, synth, volume
    monkeypatch.setattr(volume, "_STREAM_MIN_BYTES", 0)
    monkeypatch.setattr(stack_detect, "PRUNE_AHEAD", ahead)
    shape = (230, 72, 80)
    vol = synth.make_volume(71, shape, 140)
    if channels == 2:
        other = synth.make_volume(72, shape, 90)
        vol = np.stack((vol, np.maximum(other, (vol.astype(np.int32) * 7 // 10).astype(vol.dtype))), axis=-1)
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
        made.append((self.z_off, self.tensor.shape[0]))
    monkeypatch.setattr(bl.DeviceVolume, "__init__", spy)
    try:
        monkeypatch.setattr(stack_detect, "MAX_RESIDENT_BYTES", 1 << 40)
        whole = run()
        # (blocks whose overlap prune falls back to SciPy's pair order make small volumes of their own)
        assert all(m[0] == 0 for m in made) and made[0][1] == shape[0]
        del made[:]
        plane = int(np.prod(vol.shape[1:])) * 2
        monkeypatch.setattr(stack_detect, "MAX_RESIDENT_BYTES", 200 * plane)     # (230 planes: two block layers per chunk)
        parts = run()
        chunks = [m for m in made if m[0] > 0]
        assert made[0][0] == 0 and made[0][1] < shape[0] and len(chunks) >= 2
        assert all(b[0] > a[0] for a, b in zip(chunks, chunks[1:])) and chunks[-1][0] + chunks[-1][1] == shape[0]
        assert max(n for _, n in made) < shape[0]
        assert whole.blobs is not None and len(whole.blobs) > 100
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


_SLAB_RANK_SCRIPT = r'''
import os, sys
sys.path.insert(0, {root!r})
import numpy as np, torch
import torch.distributed as td
from magellanmapper_amd import blob_log as bl, config, dist, stack_detect, volume
from oracle import magmap_oracle as mmo

rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(0)                            # (both ranks share the one GPU of a test box)
td.init_process_group("gloo")
try:
    c5 = {c5!r}
    volume._STREAM_MIN_BYTES = 0
    config.setup_roi_profiles(None)
    profile = dict(num_sigma=3, denoise_size=25 if c5 else None, segment_size=40)
    config.roi_profile.update(profile)
    for p in config.roi_profiles:
        p.update(profile)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "slab"
    config.near_max = [-1.0, -1.0]
    made = []
    init = bl.DeviceVolume.__init__
    def spy(self, *a, **k):
        init(self, *a, **k)
        made.append((self.z_off, self.tensor.shape[0], self.shape[0]))
    bl.DeviceVolume.__init__ = spy
    img5d = stack_detect.Image5d(np.load(os.path.join({tmp!r}, "whole.npy"), mmap_mode="r"))
    chans = [0, 1] if c5 else [0]
    _, _, blobs = stack_detect.detect_blobs_blocks("slab", img5d, None, None, chans, False, False, True, c5)
    # this rank's planes only: rank 0 from plane 0, rank 1 from further up, neither the whole image
    z_off, planes, full = made[0]
    assert full == 160 and planes < 160 and (z_off == 0) == (rank == 0), made[0]
    vol = np.load(os.path.join({tmp!r}, "whole.npy"))[0]
    profiles = [dict(config.roi_profile)] * len(chans)
    if rank == 0:
        if c5:
            want, stages = mmo.detect_blobs_blocks(vol, [0, 1], profiles, config.resolutions, near_max=[-1.0, -1.0],
                                                   coloc=True)
            np.testing.assert_array_equal(blobs.blobs, want)
            np.testing.assert_array_equal(blobs.colocalizations, stages["colocs"])
        else:
            want, _ = mmo.detect_blobs_blocks(vol, None, profiles, config.resolutions)
            key = lambda t: np.lexsort(tuple(t[:, i] for i in range(t.shape[1] - 1, -1, -1)))
            np.testing.assert_array_equal(blobs.blobs[key(blobs.blobs)], want[key(want)])
        assert len(want) > 30
    # the same image twice as the tiles of a stack, every tile's BLOCKS over both ranks: the prefetch of a tile takes this
    # rank's planes only as well, the next tile's while this one is detected
    del made[:]
    tiles = [stack_detect.Image5d(np.load(os.path.join({tmp!r}, "whole.npy"), mmap_mode="r")) for _ in range(2)]
    n_seen = 0
    for k, tb in stack_detect.detect_blobs_tiles("slabtiles", tiles, chans, c5, False, shard=None):
        if rank == 0:
            np.testing.assert_array_equal(tb.blobs, blobs.blobs)
            if c5:
                np.testing.assert_array_equal(tb.colocalizations, blobs.colocalizations)
        n_seen += 1
    slabs = [m for m in made if m[2] == 160 and m[1] < 160]
    assert n_seen == 2 and len(slabs) == 2 and all((m[0] == 0) == (rank == 0) for m in slabs), made
    assert not any(m[1] == 160 for m in made)               # nobody uploaded a whole tile
    torch.cuda.synchronize()
    print(f"SLAB_RANK_OK {{rank}} {{z_off}} {{planes}}", flush=True)
finally:
    td.destroy_process_group()
'''


@pytest.mark.parametrize("c5", [False, True])
def test_two_ranks_upload_only_their_own_planes_of_a_memory_mapped_image(gpu, tmp_path, c5):
    """The BLOCK split of one host image over two ranks (gloo, sharing this GPU): every rank's device volume holds the
    planes its own blocks touch and answers for the whole image (``DeviceVolume(z_off=...)``) -- a rank of N uploads a
    N-th of the image over its own link, not the image up to its share's end -- and rank 0's final table (C5-shaped: with
    the co-localisation flags) equals the oracle's for the whole image."""
    import os
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    from magellanmapper_amd import synth
    shape = (160, 72, 80)
    c0 = synth.make_volume(91, shape, 110)
    if c5:
        c1 = np.maximum(synth.make_volume(92, shape, 80).astype(np.int32), (c0.astype(np.int32) * 7) // 10)
        c0 = np.stack((c0, c1.astype(np.uint16)), axis=-1)
    np.save(tmp_path / "whole.npy", c0[None])
    script = tmp_path / "slab_ranks.py"
    script.write_text(_SLAB_RANK_SCRIPT.format(root=ROOT, tmp=str(tmp_path), c5=c5))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    assert "SLAB_RANK_OK 0 0 " in run.stdout and "SLAB_RANK_OK 1 " in run.stdout
