#!/usr/bin/env python3
"""The benchmark volume (C3, 2048 x 2048 x 1024 uint16, 8.6 GB) detected from a MEMORY MAP with stack_detect.MAX_RESIDENT_BYTES
so small that a layer of blocks no longer fits and is cut into runs of block rows (stack_detect._zy_chunks), beside the
z-chunks of one whole layer each: the table's digest against C3_DIGEST (tests/test_gpu_configs.py) and what the cuts cost
(the rows two neighbouring block rows share go up twice).  On a tree without _zy_chunks only the z-chunk run is made.

    python tools/exp/ychunked_c3.py [out.json]
"""
import hashlib, json, os, re, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np, torch
import bench
from magellanmapper_amd import blob_log as bl, config, stack_detect, synth

dev = torch.device("cuda", 0)
shape, seed = bench.CONFIGS["c3"]["shape"], bench.CONFIGS["c3"]["seed"]
fd, path = tempfile.mkstemp(suffix=".npy", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
os.close(fd)
try:
    np.save(path, synth.make_volume_device(shape, seed, dev).cpu().numpy()[None])
    torch.cuda.empty_cache()
    config.resolutions = bench.RESOLUTIONS
    config.filename = "ychunked"
    config.setup_roi_profiles(None)
    config.roi_profile.update(dict(bench._BASE_PROFILE, **bench.CONFIGS["c3"]["profile"]))
    for p in config.roi_profiles:
        p.update(config.roi_profile)
    config.near_max = [-1.0]
    with open(os.path.join(ROOT, "tests", "test_gpu_configs.py")) as f:
        want = re.search(r'^C3_DIGEST = "([0-9a-f]{40})"', f.read(), re.M).group(1)
    bk = stack_detect.setup_blocks(config.get_roi_profile(0), shape)
    plane = shape[1] * shape[2] * 2
    layer = max(s[0].indices(shape[0])[1] - s[0].indices(shape[0])[0] for s in bk.sub_roi_slices[:, 0, 0])
    made = []
    init = bl.DeviceVolume.__init__

    def spy(self, *a, **k):
        init(self, *a, **k)
        if tuple(self.shape[:3]) == tuple(shape):
            made.append((int(self.z_off), int(getattr(self, "y_off", 0))) + tuple(int(v) for v in self.tensor.shape[:2]))
    bl.DeviceVolume.__init__ = spy

    def run(limit):
        stack_detect.MAX_RESIDENT_BYTES = limit
        times = []
        for _ in range(4):
            del made[:]
            img5d = stack_detect.Image5d(np.load(path, mmap_mode="r"))
            t0 = time.perf_counter()
            _, _, blobs = stack_detect.detect_blobs_blocks("ychunked", img5d, None, None, [0], False, False, True, False)
            torch.cuda.synchronize()
            times.append(round((time.perf_counter() - t0) * 1e3, 1))
        digest = hashlib.sha1(np.ascontiguousarray(blobs.blobs).tobytes()).hexdigest()
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        torch.cuda.reset_peak_memory_stats()
        return dict(max_resident_bytes=int(limit), chunk_volumes=len(made), distinct_y_off=sorted({m[1] for m in made}),
                    largest_chunk_bytes=max(m[2] * m[3] * shape[2] * 2 for m in made),
                    uploaded_over_image_bytes=round(sum(m[2] * m[3] for m in made) / (shape[0] * shape[1]), 4),
                    ms_per_call=times, ms_best_of_last_3=min(times[1:]), blobs=int(len(blobs.blobs)), table_sha1=digest,
                    equals_C3_DIGEST=digest == want, peak_device_GiB=round(peak, 2))

    out = {"volume": list(shape), "source": "memory-mapped .npy", "block_grid": list(bk.sub_roi_slices.shape),
           "thickest_layer_planes": int(layer), "has_zy_chunks": hasattr(stack_detect, "_zy_chunks"),
           # one whole layer per chunk: limit // 2 = the thickest layer
           "z_chunks_of_one_layer": run(2 * layer * plane)}
    if out["has_zy_chunks"]:
        # a third of a layer per chunk: every layer is cut into runs of block rows
        out["y_chunks_third_of_a_layer"] = run(2 * layer * plane // 3)
    line = json.dumps(out)
    print(line, flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
finally:
    os.unlink(path)
