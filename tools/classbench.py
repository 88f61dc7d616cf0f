#!/usr/bin/env python3
"""Time the classifier's patch extraction (``mmx_extract_patches``) on the benchmark volume's own blob table.

    python tools/classbench.py [--out profiles/r12_classify.json] [--commit SHA]
                               [--parent-step-ms A B C] [--step-ms D]

The benchmark volume (``synth``, 1024 x 2048 x 2048 uint16, seed 3) is generated on the device and detected with
``bench.py``'s c3 profile; the blobs of the resulting table whose size-16 patches lie inside the image (the rim rule of
``classifier.setup_classification_roi``) are the workload -- about 3e5 patches.

* the kernel: ``--calls`` launches between two HIP events, ``--windows`` windows, median and spread, for the float32
  model copy alone (what a classification launches) and for both outputs; every shape is warmed up first;
* the host: the NumPy statement of the reference's formula (``classifier.extract_patches`` on the host copy of the
  same volume, same table), wall clock, best of ``--host-runs`` -- context: what a host pays, never a target;
* the two results are compared bit for bit over the whole table.

``--parent-step-ms`` / ``--step-ms``: step times of ``python bench.py`` (no model set) on the same box for the parent
commit (its run-to-run spread) and for this commit, recorded beside the kernel figures.  Needs a GPU."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_classify.json"))
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 2048, 2048))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--size", type=int, default=16, help="patch size")
    ap.add_argument("--calls", type=int, default=20, help="launches per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit these figures belong to (recorded)")
    ap.add_argument("--parent-step-ms", type=float, nargs="*", default=None)
    ap.add_argument("--step-ms", type=float, nargs="*", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("classbench needs a GPU (there is no CPU fallback)")
    import bench
    from magellanmapper_amd import _native as nat, classifier, config, stack_detect, synth
    from magellanmapper_amd.volume import DeviceVolume
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    nat.keep_host_heap()
    shape = tuple(int(v) for v in args.shape)
    size = int(args.size)

    # ---- the benchmark volume and its own table
    config.resolutions = bench.RESOLUTIONS
    config.filename = "classbench"
    config.setup_roi_profiles(None)
    profile = dict(bench._BASE_PROFILE, **bench.CONFIGS["c3"]["profile"])
    config.roi_profile.update(profile)
    config.near_max = [-1.0]
    dvol = DeviceVolume(synth.make_volume_device(shape, args.seed, dev), dev)
    img5d = stack_detect.Image5d(np.broadcast_to(np.zeros(1, dtype=np.uint16), (1,) + shape))     # (geometry only)
    img5d.device_volume = dvol
    t0 = time.perf_counter()
    _, _, blobs = stack_detect.detect_blobs_blocks("classbench", img5d, None, None, [0], False, False, True, False)
    detect_s = time.perf_counter() - t0
    table = blobs.blobs
    mask, _ = classifier._roi_mask(blobs, classifier._roi_geometry(shape, (0, 0, 0), shape, size), False)
    zyx = np.ascontiguousarray(table[mask, :3].astype(np.int32))
    n = len(zyx)
    classifier._check_patches(zyx, size, shape)
    back, fwd = classifier._extents(size)
    elems = (back + fwd) * 2 * back

    # ---- the kernel
    L = nat.lib()
    stream = torch.cuda.current_stream().cuda_stream
    vol = dvol.view(0, False)
    d_zyx = torch.from_numpy(zyx).to(dev)
    d_ref = torch.empty((n, back + fwd, 2 * back), dtype=torch.float64, device=dev)
    d_f32 = torch.empty((n, back + fwd, 2 * back), dtype=torch.float32, device=dev)

    def time_kernel(ref, f32):
        def call():
            nat.check(L.mmx_extract_patches(vol, d_zyx.data_ptr(), n, size, d_ref.data_ptr() if ref else None,
                                            d_f32.data_ptr() if f32 else None, stream), "mmx_extract_patches")
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(args.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                call()
            e1.record()
            e1.synchronize()
            per_call.append(e0.elapsed_time(e1) / args.calls)
        per_call.sort()
        med = float(np.median(per_call))
        written = n * elems * ((8 if ref else 0) + (4 if f32 else 0))
        return {"ms_median": round(med, 4), "ms_min": round(per_call[0], 4), "ms_max": round(per_call[-1], 4),
                "windows": args.windows, "calls_per_window": args.calls, "bytes_written": written,
                "write_GBps": round(written / (med * 1e-3) / 1e9, 1), "patches_per_s": round(n / (med * 1e-3))}

    kernel = {"float32_model_copy": time_kernel(False, True), "both_outputs": time_kernel(True, True)}

    # ---- the host: the same formula in NumPy over the same table, and the comparison
    host_vol = dvol.tensor.cpu().numpy()
    host_s = []
    for _ in range(max(1, args.host_runs)):
        t0 = time.perf_counter()
        want = classifier.extract_patches(host_vol, zyx, size)
        host_s.append(time.perf_counter() - t0)
    got = d_ref.cpu().numpy()
    identical = bool(np.array_equal(got, want[..., 0], equal_nan=True))
    identical32 = bool(np.array_equal(d_f32.cpu().numpy(), want[..., 0].astype(np.float32), equal_nan=True))
    if not (identical and identical32):
        raise SystemExit("device patches differ from the host formula")

    result = {"what": "mmx_extract_patches on the benchmark volume's own blob table: one size-%d patch per blob, divided "
                      "by its maximum" % size,
              "device": torch.cuda.get_device_name(0), "commit": args.commit,
              "shape": list(shape), "dtype": "uint16", "seed": args.seed, "patch_size": size,
              "blobs_in_table": int(len(table)), "patches": int(n), "detection_s_first_call": round(detect_s, 3),
              "kernel": kernel,
              "host": {"what": "classifier.extract_patches on the host copy of the volume (NumPy gather, maximum, true "
                               "divide; float64 out), wall clock",
                       "s_best": round(min(host_s), 4), "s_all": [round(s, 4) for s in host_s],
                       "cores_visible": os.cpu_count(), "numpy": np.__version__},
              "identical_to_host": identical and identical32}
    if args.parent_step_ms:
        p = sorted(args.parent_step_ms)
        result["bench_step_ms_no_model"] = {
            "cmd": "python bench.py --gpus 1 (c3), same box, one call", "parent_runs": p,
            "parent_spread": [p[0], p[-1]], "this_commit_runs": sorted(args.step_ms or []),
            "inside_parent_spread": bool(args.step_ms) and all(p[0] <= s <= p[-1] for s in args.step_ms),
            "none_above_parent_max": bool(args.step_ms) and all(s <= p[-1] for s in args.step_ms)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
