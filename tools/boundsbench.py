#!/usr/bin/env python3
"""Time the intensity-bound order statistics (``mmx_order_stats``) on the benchmark volume.

    python tools/boundsbench.py [--out profiles/r07_bounds.json] [--c3-step-ms MS]

On the benchmark volume (``synth``, 1024 x 2048 x 2048 uint16, seed 3) and on a constant volume of the same size:
per-plane mode (1 024 groups of one plane: what ``importer.measure_near_bounds`` runs) and whole-image mode (one group
of 4.3e9 voxels: ``importer.calc_intensity_bounds``).  Every timed shape is warmed up; a window is ``--calls`` calls
between two device events, ``--windows`` windows per shape, median and spread over the windows.  Bytes read = key bytes
(levels) x bytes of the channel; the rate is quoted against a device copy measured the way ``bench.py --full`` measures
it (``mmx_calib_stream`` kind 1, 1 GiB in + 1 GiB out).  ``np.percentile`` on 16 evenly spaced planes on the CPU gives
the host cost per plane and its extrapolation to 1 024 planes (context: what the reference pays, never a target).
Needs a GPU: without one it fails."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_bounds.json"))
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 2048, 2048))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--c3-step-ms", type=float, default=None,
                    help="one C3 detection step as `python bench.py` reports it on this box (recorded for comparison)")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("boundsbench needs a GPU (there is no CPU fallback)")
    from magellanmapper_amd import _native as nat, importer, synth
    from magellanmapper_amd.volume import DeviceVolume
    L = nat.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    shape = tuple(int(v) for v in args.shape)
    nz, ny, nx = shape
    n_vox = nz * ny * nx
    stream = torch.cuda.current_stream().cuda_stream

    # ---- the device copy rate, as bench.py --full measures it
    n = 1 << 28
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for it in range(3):
        if it == 1:
            ev[0].record()
        nat.check(L.mmx_calib_stream(1, a.data_ptr(), b.data_ptr(), n, stream), "mmx_calib_stream")
    ev[1].record()
    torch.cuda.synchronize()
    copy_gbps = 2 * 2 * n * 4 / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9
    del a, b

    def tables(mode):
        groups = [(z, z + 1) for z in range(nz)] if mode == "per_plane" else [(0, nz)]
        table = np.zeros(len(groups), dtype=nat.RANK_GROUP_DTYPE)
        for g, (z0, z1) in enumerate(groups):
            table[g]["z0"], table[g]["z1"] = z0, z1
            table[g]["rank"] = importer._bounds_ranks((z1 - z0) * ny * nx, 0.5, 99.5)[0]
        return table

    def time_mode(dv, mode):
        table = tables(mode)
        d_groups = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
        d_stats = torch.empty((len(table), 4), dtype=torch.float64, device=dev)
        d_nan = torch.empty(len(table), dtype=torch.int32, device=dev)
        wb = int(L.mmx_order_stats_workspace(len(table)))
        d_work = torch.empty(wb, dtype=torch.uint8, device=dev)
        vol = dv.view(0, False)

        def call():
            nat.check(L.mmx_order_stats(vol, nz, ny, nx, d_groups.data_ptr(), table.ctypes.data, len(table),
                                        d_stats.data_ptr(), d_nan.data_ptr(), d_work.data_ptr(), wb, stream),
                      "mmx_order_stats")

        for _ in range(3):                      # warm-up of this shape
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
        levels = {1: 1, 2: 2, 4: 4, 8: 8}[dv.np_dtype.itemsize]
        read = levels * n_vox * dv.np_dtype.itemsize
        tbps = read / (med * 1e-3) / 1e12
        return {"groups": len(table), "ms_median": round(med, 4), "ms_min": round(per_call[0], 4),
                "ms_max": round(per_call[-1], 4), "windows": args.windows, "calls_per_window": args.calls,
                "bytes_read": read, "read_TBps": round(tbps, 3),
                "frac_of_copy_rate": round(tbps * 1e3 / copy_gbps, 3)}, d_stats.cpu().numpy()

    result = {"what": "mmx_order_stats on the benchmark volume: exact per-plane / whole-image order statistics of the "
                      "(0.5, 99.5) percentiles",
              "shape": list(shape), "dtype": "uint16", "seed": args.seed, "device": torch.cuda.get_device_name(0),
              "copy_GBps": round(copy_gbps, 1),
              "copy_how": "mmx_calib_stream kind 1, 1 GiB in + 1 GiB out, read + write bytes over time (bench.py --full)",
              "c3_step_ms_bench_py": args.c3_step_ms, "inputs": {}}

    synth_t = synth.make_volume_device(shape, args.seed, dev)
    # ---- the CPU side first (the planes come from the device copy): np.percentile on 16 evenly spaced planes
    cpu_s = []
    zs = [int(v) for v in np.linspace(0, nz - 1, 16).round()]
    cpu_vals = {}
    for z in zs:
        plane = synth_t[z].cpu().numpy()
        t0 = time.perf_counter()
        cpu_vals[z] = np.percentile(plane, (0.5, 99.5))
        cpu_s.append(time.perf_counter() - t0)
    result["cpu"] = {"what": "np.percentile(plane, (0.5, 99.5)) of one 2048 x 2048 uint16 plane, one core (NumPy's "
                             "selection is single-threaded)",
                     "planes_timed": len(zs), "s_per_plane_median": round(float(np.median(cpu_s)), 4),
                     "s_per_plane_min": round(min(cpu_s), 4), "s_per_plane_max": round(max(cpu_s), 4),
                     "s_1024_planes_EXTRAPOLATED": round(float(np.median(cpu_s)) * nz, 1),
                     "cores_used": 1, "cores_visible": os.cpu_count(), "numpy": np.__version__}

    for name in ("synth", "constant"):
        if name == "synth":
            t = synth_t
        else:
            del dv, t, synth_t
            torch.cuda.empty_cache()
            t = torch.full(shape, 500, dtype=torch.uint16, device=dev)
        dv = DeviceVolume(t)
        rec = {}
        for mode in ("per_plane", "whole_image"):
            rec[mode], stats = time_mode(dv, mode)
            if name == "synth" and mode == "per_plane":     # the timed call computes what the CPU computed
                for z in zs:
                    rk, lo_g, hi_g = importer._bounds_ranks(ny * nx, 0.5, 99.5)
                    got = [importer.percentile_from_order_stats(stats[z, 0], stats[z, 1], lo_g, np.uint16),
                           importer.percentile_from_order_stats(stats[z, 2], stats[z, 3], hi_g, np.uint16)]
                    if not np.array_equal(got, cpu_vals[z]):
                        raise SystemExit(f"plane {z}: device {got} != np.percentile {cpu_vals[z]}")
                rec["checked_planes_equal_numpy"] = len(zs)
            if name == "constant":
                if not np.all(stats == 500.0):
                    raise SystemExit("constant volume: wrong order statistics")
        result["inputs"][name] = rec
    s, c = result["inputs"]["synth"], result["inputs"]["constant"]
    result["constant_over_synth"] = {m: round(c[m]["ms_median"] / s[m]["ms_median"], 3) for m in ("per_plane", "whole_image")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
