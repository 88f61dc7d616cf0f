#!/usr/bin/env python3
"""Time the passes of the whole-image denoise (``equalize.denoise_roi``, the ``denoise`` task) on the device.

    python tools/denoise_imgbench.py [--out profiles/r20_denoise_img.json] [--shape 1024x2048x2048] [--repeats 3]

On the nuclei-like synthetic (``synth.make_volume_device``, seed 3), resident on the device, as uint16 and as the
float64 image ``saturate`` leaves of it, with the default profile:

* the kernel time, HIP events around the launch, median over the repetitions after one warm-up, of the sum, the three
  correlate passes, and the erosion of the whole volume; beside each the bytes it moves per voxel (its own reads and
  writes, each counted once), its float64 operations per voxel (97 per correlate pass: 64 additions and 33 products, none
  fused; 2 for the clip, 3 for the unsharp mask, 6 minima for the erosion), and both as fractions of the device copy of
  the same run (``mmx_calib_stream`` kind 1) and of the float64 vector rate without FMA (256 CUs x 64 lanes x 2.4 GHz =
  39.3 Top/s);
* the whole ``denoise_roi`` call, result left on the device, with the erosion on (a threshold below the mean) and off;
* the chain ``saturate`` -> ``denoise`` of the resident uint16 volume, nothing leaving the device, and -- on a reduced
  shape, both ways -- the same chain from a host array to a host array with the intermediate through the host;
* the CPU oracle (``oracle.preprocess_oracle.denoise_roi``: SciPy, one core) on a 256^3 piece: the only "before".

For comparison the per-tile kernels of the block path: ``DESIGN.md`` section 4c / ``tools/ppbench.py``, 47.5 us per 25^3
tile and CU for three passes of about 68 operations per voxel (clamped taps folded at compile time).

Needs a GPU: without one it fails."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F64_TOPS = 39.3            # 256 CUs x 64 lanes x 2.4 GHz, one unfused float64 operation per lane and clock
TAP_OPS = 97


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="1024x2048x2048")
    ap.add_argument("--small", default="256x1024x2048", help="the shape of the host-to-host chain")
    ap.add_argument("--cpu", default="256x256x256", help="the piece the CPU oracle is timed on")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("denoise_imgbench needs a GPU (there is no CPU fallback)")
    from magellanmapper_amd import _native as nat, config, device_image, equalize, preprocess, synth
    from magellanmapper_amd.volume import DeviceVolume
    from oracle import preprocess_oracle as ppo
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = nat.lib()
    stream = torch.cuda.current_stream().cuda_stream
    config.setup_roi_profiles(None)
    config.near_max = [40000.0]
    prof = config.roi_profile
    lo, hi, strength = float(prof["clip_min"]), float(prof["clip_max"]), float(prof["unsharp_strength"])
    weights = preprocess.gauss_weights()

    def timed(fn, repeats=args.repeats):
        """Median milliseconds of ``fn`` between two events on the current stream, after one warm-up."""
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), [round(v, 3) for v in ms]

    def walled(fn, repeats=args.repeats):
        """Median wall milliseconds of ``fn`` (which synchronises), after one warm-up."""
        fn()
        walls = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            walls.append((time.perf_counter() - t0) * 1e3)
        return {"ms": round(float(np.median(walls)), 2), "runs_ms": [round(v, 2) for v in walls]}

    n = (1 << 30) // 4
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    copy_ms, _ = timed(lambda: nat.check(L.mmx_calib_stream(1, a.data_ptr(), b.data_ptr(), n, stream), "calib"), 5)
    copy_rate = 2 * n * 4 / copy_ms / 1e6
    del a, b
    shape = tuple(int(v) for v in args.shape.split("x"))
    nz, ny, nx = shape
    nvox = int(np.prod(shape, dtype=np.int64))
    rec = {"tool": "tools/denoise_imgbench.py", "device": torch.cuda.get_device_name(0), "shape": list(shape),
           "profile": {k: prof[k] for k in ("clip_min", "clip_max", "unsharp_strength", "erosion_threshold")},
           "copy_gb_s": round(copy_rate, 1),
           "copy_how": "mmx_calib_stream kind 1, 1 GiB in + 1 GiB out, read + write bytes over time",
           "f64_tops_ceiling": F64_TOPS,
           "f64_ceiling_how": "256 CUs x 64 lanes x 2.4 GHz, unfused float64 operations (SciPy's arithmetic has no FMA)",
           "tile_kernels_for_comparison": "DESIGN.md 4c / tools/ppbench.py: pp_blur_kernel 47.5 us per 25^3 tile and CU, "
                                          "three passes of ~68 operations per voxel",
           "dtypes": {}}
    print("device copy: %.0f GB/s" % copy_rate)

    def row(ms, runs, nbytes, ops):
        rate = nbytes * nvox / ms / 1e6
        tops = ops * nvox / ms / 1e9
        return {"ms": round(ms, 3), "runs_ms": runs, "bytes_per_voxel": nbytes, "gb_s": round(rate, 1),
                "of_copy": round(rate / copy_rate, 3), "f64_ops_per_voxel": ops, "f64_tops": round(tops, 2),
                "of_f64_ceiling": round(tops / F64_TOPS, 3)}

    u16 = synth.make_volume_device(shape, args.seed, dev)
    for name in ("uint16", "float64"):
        if name == "uint16":
            vol = DeviceVolume(u16)
        else:
            vol = DeviceVolume(equalize.saturate_roi(DeviceVolume(u16), _keep=True))
            assert vol.np_dtype == np.float64
        esize = vol.tensor.element_size()
        src = device_image.view(vol, 0)
        buf_a = torch.empty(nvox, dtype=torch.float64, device=dev)
        buf_b = torch.empty(nvox, dtype=torch.float64, device=dev)
        sums = torch.zeros(2, dtype=torch.int64, device=dev)
        drec = rec["dtypes"][name] = {"kernels": {}}

        def blur(axis, d_in, d_out, last):
            nat.check(L.mmx_dn_blur(ctypes.byref(src), nz, ny, nx, axis, weights.ctypes.data, lo, hi,
                                    d_in.data_ptr() if d_in is not None else None, d_out.data_ptr(), last, strength,
                                    stream), "mmx_dn_blur")
        passes = [
            ("sum", lambda: nat.check(L.mmx_dn_sum(ctypes.byref(src), nz, ny, nx, sums.data_ptr(), stream),
                                      "mmx_dn_sum"), esize, 2 if name == "float64" else 1),
            ("blur_z", lambda: blur(0, None, buf_a, 0), esize + 8, TAP_OPS + 2),
            ("blur_y", lambda: blur(1, buf_a, buf_b, 0), 16, TAP_OPS),
            ("blur_x_unsharp", lambda: blur(2, buf_b, buf_a, 1), 16 + esize, TAP_OPS + 2 + 3),
            ("erode", lambda: nat.check(L.mmx_dn_erode(buf_a.data_ptr(), nz, ny, nx, 0, nz, buf_b.data_ptr(), stream),
                                        "mmx_dn_erode"), 16, 6),
        ]
        total = 0.0
        for key, fn, nbytes, ops in passes:
            ms, runs = timed(fn)
            total += ms
            drec["kernels"][key] = r = row(ms, runs, nbytes, ops)
            print("%-8s %-15s %9.3f ms  %7.1f GB/s (%.2f of the copy)  %6.2f Top/s (%.2f of the ceiling)" % (
                name, key, ms, r["gb_s"], r["of_copy"], r["f64_tops"], r["of_f64_ceiling"]))
        drec["kernels_total_ms"] = round(total, 3)
        drec["kernels_total_without_erosion_ms"] = round(total - drec["kernels"]["erode"]["ms"], 3)
        del buf_a, buf_b
        torch.cuda.empty_cache()

        def call():
            out = equalize.denoise_roi(vol, _keep=True)
            torch.cuda.synchronize()
            del out
        for label, thr in (("erosion_on", 1e-9), ("erosion_off", 0)):
            prof["erosion_threshold"] = thr
            stats = {}
            equalize.denoise_roi(vol, _keep=True, _stats=stats)
            drec["denoise_roi_resident_" + label] = dict(walled(call), verdicts=stats.get("verdicts", []))
            print("%-8s denoise_roi resident, %s: %.1f ms" % (name, label, drec["denoise_roi_resident_" + label]["ms"]))
        prof["erosion_threshold"] = rec["profile"]["erosion_threshold"]
        if name == "float64":
            del vol
        torch.cuda.empty_cache()

    def chain_resident(first):
        sat = equalize.saturate_roi(first, _keep=True)
        out = equalize.denoise_roi(DeviceVolume(sat), _keep=True)
        torch.cuda.synchronize()
        del sat, out
    vol = DeviceVolume(u16)
    rec["chain_saturate_denoise_resident"] = walled(lambda: chain_resident(vol))
    print("saturate -> denoise, resident: %.1f ms" % rec["chain_saturate_denoise_resident"]["ms"])
    del vol, u16
    torch.cuda.empty_cache()

    # ---- the same chain on a reduced shape: nothing leaving the device, and host array to host array with the
    # intermediate through the host
    small = tuple(int(v) for v in args.small.split("x"))
    host = synth.make_volume_device(small, args.seed, dev).cpu().numpy()
    svol = DeviceVolume(host)
    res_small = walled(lambda: chain_resident(svol))
    del svol

    def chain_host():
        return equalize.denoise_roi(equalize.saturate_roi(host))
    rec["reduced_shape"] = {"shape": list(small), "chain_resident": res_small, "chain_through_host": walled(chain_host, 2)}
    print("reduced %s: resident %.1f ms, through the host %.1f ms" % (
        args.small, res_small["ms"], rec["reduced_shape"]["chain_through_host"]["ms"]))

    # ---- the CPU oracle on a piece: the only "before"
    cpu = tuple(int(v) for v in args.cpu.split("x"))
    piece = equalize.saturate_roi(np.ascontiguousarray(host[:cpu[0], :cpu[1], :cpu[2]]))
    profs = [dict(prof, erosion_threshold=1e-9)]
    t0 = time.perf_counter()
    want = ppo.denoise_roi(piece, profs)
    cpu_s = time.perf_counter() - t0
    prof["erosion_threshold"] = 1e-9
    got = equalize.denoise_roi(piece)
    rec["cpu_oracle"] = {"shape": list(piece.shape), "seconds": round(cpu_s, 2),
                         "ns_per_voxel": round(cpu_s * 1e9 / piece.size, 1), "equal_to_device": bool(np.array_equal(got, want)),
                         "note": "SciPy / NumPy on one core, erosion on"}
    print("CPU oracle %s: %.2f s (%.0f ns per voxel), equal to the device: %s" % (
        args.cpu, cpu_s, rec["cpu_oracle"]["ns_per_voxel"], rec["cpu_oracle"]["equal_to_device"]))

    text = json.dumps(rec, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
