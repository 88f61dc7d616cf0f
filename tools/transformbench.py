#!/usr/bin/env python3
"""Time the whole-image down-sampling (``transformer.downsample``) on the benchmark volume.

    python tools/transformbench.py [--out profiles/r17_transform.json] [--shape 1024 2048 2048] [--repeats 5]

On the benchmark volume (``synth.make_volume_device``, 1024 x 2048 x 2048 uint16, seed 3), through the A/B harness
(``abbench``: one worker process per variant, alive for the whole run, strictly alternating after a warm-up):

* ``rescale=0.25`` and a ``target_size`` of the same ratio, the volume resident on the device and ``--from-host``
  (a pageable host copy, uploaded inside the timed call): milliseconds per volume end to end (a host clock around a call
  that ends with the result on the host), median and spread over the repetitions, and the kernels' share of it
  (the library's per-family events);
* the sparse anti-aliased path against the DENSE composition of the existing kernels (``mmx_gauss_axis_batch`` x 3 +
  ``mmx_resize_batch_as`` on a float64 copy of each converted layer) in the same run, with the digests of both results;
* the device copy rate as ``bench.py --full`` measures it (``mmx_calib_stream`` kind 1), and the rate each case moves
  its input and output once against it;
* the CPU chain (SciPy, same chunk plan, a process pool of ``--cpu-procs``) on ``--cpu-chunks`` chunks of the plan,
  extrapolated to the plan's chunk count: context (what the reference pays), never a target.

Needs a GPU: without one it fails."""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import abbench  # noqa: E402

CASES = ("rescale_resident", "target_resident", "rescale_from_host", "target_from_host")


def _target(shape, ratio):
    return tuple(int(v * ratio) for v in shape[::-1])           # (x, y, z)


# ------------------------------------------------------------------------------------------------------- worker
def worker(args) -> None:
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("transformbench needs a GPU (there is no CPU fallback)")
    from magellanmapper_amd import _native as nat, preprocess, synth, transformer as tr
    from magellanmapper_amd.volume import DeviceVolume
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    shape = tuple(args.shape)
    state = {}

    def volume(host: bool):
        if "dv" not in state:
            state["dv"] = DeviceVolume(synth.make_volume_device(shape, args.seed, dev))
        if host and "host" not in state:
            state["host"] = state["dv"].tensor.cpu().numpy()
        return state["host"] if host else state["dv"]

    def dense(dv):
        """The existing kernels' composition, layer by layer of the same plan: a float64 copy of the converted layer,
        three dense anti-aliasing passes, the resize."""
        plan = tr.plan_chunks(shape, None, list(_target(shape, args.ratio))[::-1])
        out = np.empty(plan.total_shape, dtype=np.float64)
        scale = 1.0 / np.iinfo(np.uint16).max
        for kz in range(plan.slices.shape[0]):
            z0, nz = int(plan.starts[0][kz]), int(plan.n_in[0][kz])
            conv = dv.tensor[z0:z0 + nz].to(torch.float64) * scale
            origins, shapes, news = [], [], []
            for ky in range(plan.slices.shape[1]):
                for kx in range(plan.slices.shape[2]):
                    origins.append((0, int(plan.starts[1][ky]), int(plan.starts[2][kx])))
                    shapes.append((nz, int(plan.n_in[1][ky]), int(plan.n_in[2][kx])))
                    news.append((int(plan.n_out[0][kz]), int(plan.n_out[1][ky]), int(plan.n_out[2][kx])))
            rs = preprocess.Rescaler(np.ones(3), [0])
            rs.set_blocks(origins, shapes, news)
            rs.run(DeviceVolume(conv), 0, origins, news, 0)
            blocks = rs.fetch(news)
            k = 0
            for ky in range(plan.slices.shape[1]):
                for kx in range(plan.slices.shape[2]):
                    oz, oy, ox = int(plan.offsets[0][kz]), int(plan.offsets[1][ky]), int(plan.offsets[2][kx])
                    n = news[k]
                    out[oz:oz + n[0], oy:oy + n[1], ox:ox + n[2]] = blocks[k]
                    k += 1
        return out

    def once(case):
        host = case.endswith("from_host")
        img = volume(host)
        kw = dict(rescale=args.ratio) if case.startswith("rescale") else dict(target_size=_target(shape, args.ratio))
        nat.timing_enable(True, ["generic"])
        nat.timing_read()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.variant == "dense":
            if case != "target_resident":
                raise ValueError("the dense composition is measured resident, anti-aliased")
            out = dense(img)
        else:
            out = tr.downsample(img, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        kernel_ms, launches = nat.timing_read()["generic"]
        nat.timing_enable(False)
        return out, ms, kernel_ms, launches

    def describe(req):
        out, ms, kernel_ms, launches = once(req["case"])
        return dict(case=req["case"], variant=args.variant, shape=list(shape), out_shape=list(out.shape),
                    out_dtype=str(out.dtype), sha1=hashlib.sha1(np.ascontiguousarray(out).tobytes()).hexdigest(),
                    ms=ms, kernel_ms=kernel_ms, launches=int(launches))

    def run(req):
        out, ms, kernel_ms, launches = once(req["case"])
        return dict(ms=ms, kernel_ms=kernel_ms, out_shape=list(out.shape))

    def copy_rate(req):
        L = nat.lib()
        n = 1 << 28
        a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
        b = torch.empty_like(a)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        stream = torch.cuda.current_stream().cuda_stream
        for it in range(3):
            if it == 1:
                ev[0].record()
            nat.check(L.mmx_calib_stream(1, a.data_ptr(), b.data_ptr(), n, stream), "mmx_calib_stream")
        ev[1].record()
        torch.cuda.synchronize()
        return dict(copy_gbps=2 * 2 * n * 4 / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9)

    abbench.serve(dict(describe=describe, run=run, copy_rate=copy_rate))


# ----------------------------------------------------------------------------------------------------- CPU chain
def _cpu_chunk(job):
    import transform_support as ts
    seed, shp, new, aa = job
    chunk = np.random.default_rng(seed).integers(0, 65535, shp, dtype=np.uint16)
    t0 = time.perf_counter()
    ts.resize_chunk_cpu(chunk, new, aa)
    return time.perf_counter() - t0


def cpu_chain(shape, ratio, n_chunks, procs):
    """SciPy on ``n_chunks`` full-size chunks of each plan in a pool of ``procs`` processes (the driver holds no GPU):
    wall time of the sample, and that scaled to the plan's chunk count."""
    import multiprocessing as mp
    from magellanmapper_amd import transformer as tr
    res = {}
    for name, plan in (("rescale", tr.plan_chunks(shape, ratio)),
                       ("target", tr.plan_chunks(shape, None, list(_target(shape, ratio))[::-1]))):
        shp = tuple(int(v[0]) for v in plan.n_in)
        new = tuple(int(v[0]) for v in plan.n_out)
        jobs = [(k, shp, new, plan.antialias) for k in range(n_chunks)]
        with mp.get_context("fork").Pool(procs) as pool:
            t0 = time.perf_counter()
            per = pool.map(_cpu_chunk, jobs)
            wall = time.perf_counter() - t0
        total = int(np.prod(plan.slices.shape))
        res[name] = dict(chunk_shape=list(shp), chunk_out=list(new), sample_chunks=n_chunks, procs=procs,
                         sample_wall_s=wall, per_chunk_s=[float(v) for v in per], plan_chunks=total,
                         extrapolated_volume_s=wall * total / n_chunks,
                         # (the sample's wall time includes making the random chunks; the resizes alone:)
                         extrapolated_resize_only_s=float(np.mean(per)) * total / procs)
    return res


# -------------------------------------------------------------------------------------------------------- driver
def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_transform.json"))
    ap.add_argument("--shape", type=int, nargs=3, default=(1024, 2048, 2048))
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--ratio", type=float, default=0.25)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--cpu-chunks", type=int, default=8)
    ap.add_argument("--cpu-procs", type=int, default=8)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--variant", choices=("sparse", "dense"), default="sparse")
    args = ap.parse_args()
    if args.worker:
        worker(args)
        return 0

    shape = tuple(args.shape)
    result = dict(shape=list(shape), ratio=args.ratio, target_size_xyz=list(_target(shape, args.ratio)), cases={})
    if not args.no_cpu:
        result["cpu_chain"] = cpu_chain(shape, args.ratio, args.cpu_chunks, args.cpu_procs)
    wargs = ["--worker", "--shape", *map(str, shape), "--seed", str(args.seed), "--ratio", str(args.ratio)]
    builds = {v: abbench.Worker(os.path.abspath(__file__), wargs + ["--variant", v]) for v in ("sparse", "dense")}
    try:
        copy = builds["sparse"].ask(cmd="copy_rate")["copy_gbps"]
        result["copy_gbps"] = copy
        in_bytes = int(np.prod(shape)) * 2
        for case in CASES:
            names = ["sparse", "dense"] if case == "target_resident" else ["sparse"]
            reps = args.host_repeats if case.endswith("from_host") else args.repeats
            kernel = {b: [] for b in names}

            def check(b, reply, described):
                assert reply["out_shape"] == described["out_shape"], (b, reply, described)
                kernel[b].append(reply["kernel_ms"])
            described, times = abbench.alternate(builds, names, case, args.warmup, reps, check)
            rec = {}
            for b in names:
                out_bytes = int(np.prod(described[b]["out_shape"])) * 8
                s = abbench.summarise(times[b], int(np.prod(shape)))
                k = abbench.summarise(kernel[b])
                gbps = (in_bytes + out_bytes) / (k["median_ms"] * 1e-3) / 1e9
                rec[b] = dict(end_to_end=s, kernels=k, described=described[b], in_plus_out_gbps_of_kernel_time=gbps,
                              fraction_of_copy_rate=gbps / copy)
            if len(names) == 2:
                rec["equal"] = described["sparse"]["sha1"] == described["dense"]["sha1"]
                ds, dd = rec["sparse"]["end_to_end"], rec["dense"]["end_to_end"]
                rec["sparse_faster_by_more_than_both_spreads"] = bool(
                    dd["median_ms"] - ds["median_ms"] > max(ds["spread_ms"], dd["spread_ms"]))
            result["cases"][case] = rec
            print(case, json.dumps({b: rec[b]["end_to_end"]["median_ms"] for b in names}), flush=True)
    finally:
        for w in builds.values():
            w.close()
    abbench.write_json(args.out, result)
    print(json.dumps(dict(out=args.out, cases={c: {b: v["end_to_end"]["median_ms"] for b, v in r.items()
                                                    if isinstance(v, dict)} for c, r in result["cases"].items()})))
    return 0


if __name__ == "__main__":
    sys.exit(main())
