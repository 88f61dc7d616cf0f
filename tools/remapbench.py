#!/usr/bin/env python3
"""Time the passes of the whole-image preprocessing (``remap`` = ``equalize_adapthist``, ``saturate``) on the device.

    python tools/remapbench.py [--out profiles/r18_preproc_img.json] [--shapes 1024x2048x2048 256x512x512] [--repeats 5]

For every shape, on the nuclei-like synthetic (``synth.make_volume_device``, uint16, seed 3) and on a uniform-random
uint16 volume, resident on the device, with the default kernel (shape // 8), clip limit 0.01 and 256 bins:

* the kernel time of every pass, HIP events around the launch, median over the repetitions after one warm-up:
  min / max (2 B per voxel read), tile histograms (2), apply (2 read + 2 written), output (2 + 8, into a device slab;
  the copy to the host is not part of it), and of ``saturate``: the order statistics (the radix select, two passes over
  uint16) and the stretch (2 + 8);
* the host time of ``mmx_host_eq_maps`` between the launches;
* the bytes per second each voxel pass achieves beside a device copy measured in the same run (``mmx_calib_stream``
  kind 1, 1 GiB in + 1 GiB out, read + write bytes over time);
* on the smaller shape, the whole call with the result on the host, and the NumPy restatement of the test suite
  (``tests/preproc_img_support.py``, one core) on the same volume: context, never a target.  The restatement cannot hold
  the benchmark volume: ``equalize_adapthist`` keeps the padded image as int64 several times over.

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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", nargs="+", default=["1024x2048x2048", "256x512x512"])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--restate-below", type=int, default=1 << 27, help="voxels up to which the host parts run")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("remapbench needs a GPU (there is no CPU fallback)")
    from magellanmapper_amd import _native as nat, config, device_image as dimg, equalize as eq, importer, synth
    from magellanmapper_amd.volume import DeviceVolume
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = nat.lib()
    stream = torch.cuda.current_stream().cuda_stream
    config.setup_roi_profiles(None)

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

    n = (1 << 30) // 4
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    copy_ms, _ = timed(lambda: nat.check(L.mmx_calib_stream(1, a.data_ptr(), b.data_ptr(), n, stream), "calib"))
    copy_rate = 2 * n * 4 / copy_ms / 1e6
    del a, b
    rec = {"tool": "tools/remapbench.py", "device": torch.cuda.get_device_name(0),
           "copy_gb_s": round(copy_rate, 1),
           "copy_how": "mmx_calib_stream kind 1, 1 GiB in + 1 GiB out, read + write bytes over time",
           "parameters": "default kernel (shape // 8), clip_limit 0.01, nbins 256, uint16 voxels", "shapes": {}}
    print("device copy: %.0f GB/s" % copy_rate)

    for shp in args.shapes:
        shape = tuple(int(v) for v in shp.split("x"))
        nz, ny, nx = shape
        nvox = nz * ny * nx
        srec = rec["shapes"][shp] = {}
        for kind in ("nuclei", "uniform"):
            if kind == "nuclei":
                t = synth.make_volume_device(shape, args.seed, dev)
            else:
                gen = torch.Generator(device=dev)
                gen.manual_seed(args.seed)
                t = torch.empty(shape, dtype=torch.int16, device=dev)
                for z0 in range(0, nz, 64):
                    part = torch.randint(-32768, 32768, t[z0:z0 + 64].shape, dtype=torch.int32, device=dev, generator=gen)
                    t[z0:z0 + 64] = part.to(torch.int16)
                t = t.view(torch.uint16)
            dv = DeviceVolume(t)
            k, nt, clim = eq.plan(shape, None, 0.01, 256)
            n_tiles = int(np.prod(nt))
            raw_min, raw_max = eq.minmax(dv, 0)
            _, bins = eq.level_bin_table(np.uint16, raw_min, raw_max, 256)
            d_bins = dimg.to_dev(bins, dev)
            src = dimg.view(dv, 0)
            geom = nat.EqGeom((ctypes.c_int32 * 3)(*shape), (ctypes.c_int32 * 3)(*k), (ctypes.c_int32 * 3)(*nt), 256)
            d_hist = torch.empty(n_tiles * 256, dtype=torch.int32, device=dev)
            passes = {}

            def p(name, nbytes, fn, repeats=args.repeats):
                ms, runs = timed(fn, repeats)
                passes[name] = {"ms": round(ms, 3), "runs_ms": runs, "bytes_per_voxel": nbytes,
                                "gb_s": round(nbytes * nvox / ms / 1e6, 1),
                                "of_copy": round(nbytes * nvox / ms / 1e6 / copy_rate, 3)}
                print("%-16s %-8s %-10s %9.3f ms  %7.1f GB/s  (%.2f of the copy)" % (
                    shp, kind, name, ms, passes[name]["gb_s"], passes[name]["of_copy"]))

            p("minmax", 2, lambda: eq.minmax(dv, 0))
            p("hist", 2, lambda: nat.check(L.mmx_eq_hist(ctypes.byref(src), ctypes.byref(geom), d_bins.data_ptr(),
                                                         d_hist.data_ptr(), stream), "mmx_eq_hist"))
            hist = d_hist.cpu().numpy().view(np.uint32)
            maps = np.empty(n_tiles * 256, dtype=np.uint16)
            t0 = time.perf_counter()
            nat.check(L.mmx_host_eq_maps(hist.ctypes.data, n_tiles, 256, clim, int(np.prod(k)), maps.ctypes.data, None),
                      "mmx_host_eq_maps")
            passes["host_maps_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            d_maps = dimg.to_dev(maps, dev)
            tiles, coef = eq.axis_tables(shape, k, nt)
            d_tiles, d_coef = dimg.to_dev(tiles, dev), dimg.to_dev(coef, dev)
            d_out = torch.empty(nvox, dtype=torch.int16, device=dev)
            d_mm = torch.empty(2, dtype=torch.int32, device=dev)
            p("apply", 4, lambda: nat.check(L.mmx_eq_apply(ctypes.byref(src), ctypes.byref(geom), d_bins.data_ptr(),
                                                           d_maps.data_ptr(), d_tiles.data_ptr(), tiles.ctypes.data,
                                                           d_coef.data_ptr(), d_out.data_ptr(), d_mm.data_ptr(), stream),
                                            "mmx_eq_apply"))
            lmin, lmax = (int(v) for v in d_mm.cpu().numpy().view(np.uint32))
            d_table = dimg.to_dev(eq.output_table(lmin, lmax), dev)
            step, _ = dimg.slab_step(shape, 8)
            slab = torch.empty(step * ny * nx, dtype=torch.float64, device=dev)

            def output():
                for z0 in range(0, nz, step):
                    cnt = (min(nz, z0 + step) - z0) * ny * nx
                    nat.check(L.mmx_eq_output(d_out.data_ptr() + 2 * z0 * ny * nx, cnt, d_table.data_ptr(),
                                              slab.data_ptr(), stream), "mmx_eq_output")
            p("output", 10, output)
            del d_out

            if kind == "nuclei":
                prof = config.get_roi_profile(0)
                p("order_stats", 4, lambda: importer._percentiles_of_groups(dv, 0, [(0, nz)], prof["clip_vmin"],
                                                                            prof["clip_vmax"]))
                lo, hi = importer._percentiles_of_groups(dv, 0, [(0, nz)], prof["clip_vmin"], prof["clip_vmax"])

                def stretch():
                    for z0 in range(0, nz, step):
                        z1 = min(nz, z0 + step)
                        sv = dimg.view(dv, 0, z0)
                        nat.check(L.mmx_stretch(ctypes.byref(sv), z1 - z0, ny, nx, float(lo[0]),
                                                float(max(hi[0], lo[0] + 1)), slab.data_ptr(), stream), "mmx_stretch")
                p("stretch", 10, stretch)
            del slab
            passes["tiles"], passes["kernel"] = n_tiles, list(k)
            passes["remap_device_ms"] = round(sum(passes[q]["ms"] for q in ("minmax", "hist", "apply", "output"))
                                              + passes["host_maps_ms"], 3)

            if nvox <= args.restate_below:
                t0 = time.perf_counter()
                got = eq.equalize_adapthist(dv)
                passes["whole_call_to_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                if kind == "nuclei":
                    import preproc_img_support as sup
                    host = t.cpu().numpy()
                    t0 = time.perf_counter()
                    want = sup.equalize_adapthist(host, None, 0.01, 256)
                    passes["numpy_restatement_s"] = round(time.perf_counter() - t0, 2)
                    passes["equal_to_restatement"] = bool(np.array_equal(got, want))
                    print("%-16s restatement %.1f s, equal: %s" % (shp, passes["numpy_restatement_s"],
                                                                    passes["equal_to_restatement"]))
                del got
            else:
                passes["numpy_restatement_s"] = None
                passes["note"] = ("the restatement (like scikit-image) cannot hold this volume: the padded image as "
                                  "int64 several times over is far beyond the host's memory")
            srec[kind] = passes
            dv.close()
            del dv, t, d_hist
            torch.cuda.empty_cache()

    text = json.dumps(rec, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
