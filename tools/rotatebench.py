#!/usr/bin/env python3
"""Time the passes of the whole-image rotation (``rotate_nd`` / ``rotate_img``) on the device.

    python tools/rotatebench.py [--out profiles/r19_rotate.json] [--shape 1024x2048x2048] [--repeats 3]

On the nuclei-like synthetic (``synth.make_volume_device``, seed 3) as uint16 and as float64, resident on the device:

* the kernel time, HIP events around the launch, median over the repetitions after one warm-up, of the per-plane
  min / max pass (``mmx_rotate_minmax``: the volume read once) and of the warp (``mmx_rotate_warp``) about each axis at
  -30, -1 and 45 degrees, orders 0 and 1;
* each as bytes per second over the model "source read once + destination written once" (the min / max pass: source
  read once), beside the device copy of the same run (``mmx_calib_stream`` kind 1, 1 GiB in + 1 GiB out);
* the whole ``rotate_img`` call of a resident uint16 volume for the stock three-entry chain
  ``((-5, 1), (-1, 2), (-30, 0))``, result left on the device;
* on a reduced shape, the same chain from a host array to a host array, and the NumPy restatement of the test suite
  (``tests/rotate_support.py``, one core) on that volume: context, never a target.

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

CHAIN = ((-5, 1), (-1, 2), (-30, 0))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default="1024x2048x2048")
    ap.add_argument("--small", default="128x256x256", help="the shape of the host-to-host call and the restatement")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--angles", type=float, nargs="+", default=[-30.0, -1.0, 45.0])
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rotatebench needs a GPU (there is no CPU fallback)")
    from magellanmapper_amd import _native as nat, device_image as dimg, rotate as rot, synth, transformer
    from magellanmapper_amd.volume import DeviceVolume
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    L = nat.lib()
    stream = torch.cuda.current_stream().cuda_stream

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
    copy_ms, _ = timed(lambda: nat.check(L.mmx_calib_stream(1, a.data_ptr(), b.data_ptr(), n, stream), "calib"), 5)
    copy_rate = 2 * n * 4 / copy_ms / 1e6
    del a, b
    shape = tuple(int(v) for v in args.shape.split("x"))
    nvox = int(np.prod(shape, dtype=np.int64))
    rec = {"tool": "tools/rotatebench.py", "device": torch.cuda.get_device_name(0), "shape": list(shape),
           "copy_gb_s": round(copy_rate, 1),
           "copy_how": "mmx_calib_stream kind 1, 1 GiB in + 1 GiB out, read + write bytes over time",
           "model": "warp: source read once + destination written once; minmax: source read once",
           "dtypes": {}}
    print("device copy: %.0f GB/s" % copy_rate)

    u16 = synth.make_volume_device(shape, args.seed, dev)
    for name in ("uint16", "float64"):
        if name == "uint16":
            src = u16
        else:
            src = torch.empty(shape, dtype=torch.float64, device=dev)
            for z0 in range(0, shape[0], 64):
                src[z0:z0 + 64] = (u16[z0:z0 + 64].view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float64)
            src += 100.0                      # (a range that does not contain 0: the put-back of zeros is live)
        esize = src.element_size()
        dst = torch.empty_like(src)
        sv, s_elems, n_chl = dimg.view(src)
        dv, d_elems, _ = dimg.view(dst)
        shape3 = shape
        drec = rec["dtypes"][name] = {"minmax": {}, "warp": {}}

        def row(ms, runs, nbytes):
            rate = nbytes * nvox / ms / 1e6
            return {"ms": round(ms, 3), "runs_ms": runs, "bytes_per_voxel": nbytes, "gb_s": round(rate, 1),
                    "of_copy": round(rate / copy_rate, 3)}

        for axis in range(3):
            bounds = torch.empty(2 * shape[axis], dtype=torch.float64, device=dev)
            ms, runs = timed(lambda: nat.check(L.mmx_rotate_minmax(ctypes.byref(sv), s_elems, *shape3, n_chl, axis,
                                                                   bounds.data_ptr(), stream), "mmx_rotate_minmax"))
            drec["minmax"]["axis%d" % axis] = r = row(ms, runs, esize)
            print("%-8s minmax axis %d           %9.3f ms  %7.1f GB/s  (%.2f of the copy)" % (
                name, axis, ms, r["gb_s"], r["of_copy"]))
            rows, cols = rot.plane_shape(shape3, axis)
            for angle in args.angles:
                m = np.ascontiguousarray(rot.rotation_matrix(rows, cols, angle).reshape(-1))
                for order in (0, 1):
                    ms, runs = timed(lambda: nat.check(
                        L.mmx_rotate_warp(ctypes.byref(sv), s_elems, ctypes.byref(dv), d_elems, *shape3, n_chl, axis,
                                          nat.as_double_ptr(m), order, bounds.data_ptr(), stream), "mmx_rotate_warp"))
                    drec["warp"]["axis%d_angle%g_order%d" % (axis, angle, order)] = r = row(ms, runs, 2 * esize)
                    print("%-8s warp   axis %d %6g o%d  %9.3f ms  %7.1f GB/s  (%.2f of the copy)" % (
                        name, axis, angle, order, ms, r["gb_s"], r["of_copy"]))
        del dst
        if name == "uint16":
            vol = DeviceVolume(src)
            settings = {"rotation": CHAIN, "resize": False, "order": 1}

            def chain():
                out = transformer.rotate_img(vol, settings)
                torch.cuda.synchronize()
                return out
            chain()
            walls = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                chain()
                walls.append((time.perf_counter() - t0) * 1e3)
            rec["rotate_img_chain_resident_ms"] = {"rotation": [list(r) for r in CHAIN], "order": 1, "dtype": name,
                                                   "ms": round(float(np.median(walls)), 2),
                                                   "runs_ms": [round(v, 2) for v in walls]}
            print("rotate_img, chain of 3, resident uint16: %.1f ms" % np.median(walls))
        else:
            del src
        torch.cuda.empty_cache()

    # ---- context at a reduced shape: host to host, and the NumPy restatement on one core
    import contextlib
    import io
    import rotate_support as sup
    small = tuple(int(v) for v in args.small.split("x"))
    host = synth.make_volume_device(small, args.seed, dev).cpu().numpy()
    settings = {"rotation": CHAIN, "resize": False, "order": 1}
    with contextlib.redirect_stdout(io.StringIO()):
        transformer.rotate_img(host, settings)
        t0 = time.perf_counter()
        got = transformer.rotate_img(host, settings)
        call_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want = sup.rotate_img(host, CHAIN, 1)
    restate_s = time.perf_counter() - t0
    rec["reduced_shape"] = {"shape": list(small), "rotate_img_host_to_host_ms": round(call_ms, 2),
                            "numpy_restatement_s": round(restate_s, 2),
                            "equal_to_restatement": bool(np.array_equal(got, want)),
                            "note": "the restatement is vectorised NumPy on one core, not scikit-image: context only"}
    print("reduced %s: call %.1f ms, restatement %.2f s, equal: %s" % (
        args.small, call_ms, restate_s, rec["reduced_shape"]["equal_to_restatement"]))

    text = json.dumps(rec, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
