#!/usr/bin/env python
"""Wide-row A/B measurement: this tree's libmmx_hip.so against another build of it (the parent commit's), in ONE run,
the two alternating repeat by repeat (the scheme of tools/abbench.py; tools/rowbench.py is the two-channel run of
SURVEY.md section 8f and has nothing to do with row widths).

    python tools/widerowbench.py --parent-lib /path/to/parent/libmmx_hip.so --repeats 10 --out profiles/r10_wide_rows.json

The default profile (segment_size 500) at 0.9 um / px: blocks ceil(500 / 0.9) + overlap = 562 voxels wide, row pitch 576
floats -- beyond the 512 the tiled matrix-core path stopped at.  Cases, one batch of 8 resident blocks each, the stock
sigma factors 3 .. 5 at 0.9 um / px in 5 scales (sigma 3.33 .. 5.56 px, radii 13 .. 22), through ``mmx_detect_batch``:
  a : 261 x 261 x 562 uint16;
  b : the same batch cut to 261 x 261 x 505 (row pitch 512): both builds take the tiled path -- the per-voxel yardstick;
  c : 200 x 200 x 1030 uint16;
  d : case a as float32 voxels in [0, 1] (``value_range`` 1).
Per case and build: device-event milliseconds per call after warm-up (median, min, max over the repeats), kernel path /
entry layout / rounds, the kernel families that ran (one extra call with the per-kernel events on), the number of
candidates, and a digest of the resolved peaks (``blob_log_blocks``: coordinates and float64 values), which must be equal
between the builds.  And a against the parent's b per voxel processed (nz ny px).

Each build runs in a worker process of its own (``--worker``; the library is chosen by ``MMX_LIB_PATH``), both alive for
the whole run; the driver hands out one repeat at a time, parent and new in turn.  A worker that dies ends the run."""
import argparse
import os
import sys

import abbench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES_UM = 0.9
FACTORS = (3.0, 5.0)
NUM_SIGMA = 5
THRESHOLD, OVERLAP = 0.1, 0.5
VOLUME = (517, 517, 1122)
#: name -> (block shape, origins along z, y, x, float voxels)
CASES = {
    "a": ((261, 261, 562), (0, 256), (0, 256), (0, 560), False),
    "b": ((261, 261, 505), (0, 256), (0, 256), (0, 560), False),
    "c": ((200, 200, 1030), (0, 256), (0, 256), (0, 92), False),
    "d": ((261, 261, 562), (0, 256), (0, 256), (0, 560), True),
}


def row_pitch(nx):
    return -(-nx // 32) * 32


def voxels_processed(name):
    nz, ny, nx = CASES[name][0]
    return 8 * nz * ny * row_pitch(nx)


# ---------------------------------------------------------------------------------------------------------- worker
def worker():
    import ctypes
    import torch
    from magellanmapper_amd import _native as nat, blob_log as bl, synth
    from magellanmapper_amd.rawbatch import RawBatch, timed
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    vol16 = synth.make_volume_device(VOLUME, 8, dev, density=synth.BLOBS_PER_MVOX / 4.0, blob_sigma=4.5)
    lo, hi = FACTORS[0] / RES_UM, FACTORS[1] / RES_UM
    volumes, keep = {}, {}

    def volume_of(as_float):
        if as_float not in volumes:
            volumes[as_float] = bl.DeviceVolume((vol16.to(torch.float32) / 65535.0) if as_float else vol16)
        return volumes[as_float]

    def batch_of(name):
        if name not in keep:
            shape, oz, oy, ox, as_float = CASES[name]
            dvol = volume_of(as_float)
            origins = [(z, y, x) for z in oz for y in oy for x in ox]
            lane = bl.Lane(0, lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP)
            lane.bind(dvol, len(origins))
            keep.clear()                # (one case's workspace and table at a time)
            batch = RawBatch(dvol, origins, [shape] * len(origins), lane.space, lane.threshold, lane.eps, 1 << 23,
                             value_range=1.0 if as_float else None, store_f32=int(as_float))
            keep[name] = (batch, batch.args())
        return keep[name]

    def one_call(name):
        batch, a = batch_of(name)
        info = nat.DetectInfo()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = batch.L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
        t1.record()
        nat.check(rc, "mmx_detect_batch")
        torch.cuda.synchronize()
        n_all, n_cands = batch.counts()
        assert n_all <= batch.cap, "candidate table too small"
        return dict(ms=t0.elapsed_time(t1), n_pass_rounds=info.n_pass_rounds, mask_layout=info.mask_layout,
                    zx_path=info.zx_path, entries=n_all, candidates=n_cands, radii=[int(r) for r in batch.space.radii])

    def describe(name):
        """The kernel families of one call, and the resolved peaks."""
        rep, kinds = timed(lambda: one_call(name))
        rep["kinds"] = {k: [ms, int(n)] for k, (ms, n) in kinds.items() if n}
        batch = batch_of(name)[0]
        _, peaks = bl.blob_log_blocks(batch.dvol, 0, batch.origins, batch.shapes, lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP,
                                      return_peaks=True)
        rep["peaks"], rep["peaks_sha1"] = abbench.peaks_digest(peaks)
        bl.release_buffers()
        return rep

    abbench.serve(dict(run=lambda req: one_call(req["case"]), describe=lambda req: describe(req["case"])))


# ---------------------------------------------------------------------------------------------------------- driver
def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-lib", help="libmmx_hip.so built from the commit to compare against")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker()
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        ap.error("--parent-lib: the other build of libmmx_hip.so to measure against")
    if args.repeats < 1:
        ap.error("--repeats")
    names = [c for c in args.cases.split(",") if c]
    for c in names:
        if c not in CASES:
            ap.error("unknown case %s" % c)
    me = os.path.abspath(__file__)
    builds = {"parent": abbench.Worker(me, ["--worker"], cwd=ROOT,
                                       env=dict(os.environ, MMX_LIB_PATH=os.path.abspath(args.parent_lib))),
              "new": abbench.Worker(me, ["--worker"], cwd=ROOT)}
    result = dict(volume="uint16 %d x %d x %d (z, y, x), 8 blocks per case" % VOLUME, resolution_um=RES_UM,
                  sigma_factors=FACTORS, num_sigma=NUM_SIGMA, threshold=THRESHOLD, warmup=args.warmup, cases={})
    ok = True
    try:
        for c in names:
            rec, times = abbench.alternate(builds, list(builds), c, args.warmup, args.repeats,
                                           check=abbench.same_fields("n_pass_rounds", "mask_layout", "zx_path", "candidates"))
            rec.update(block=CASES[c][0], row_pitch=row_pitch(CASES[c][0][2]), float_voxels=CASES[c][4],
                       voxels_processed=voxels_processed(c))
            for b in builds:
                rec[b]["ms_first"] = rec[b].pop("ms")
                rec[b].update(abbench.summarise(times[b]), ms=times[b])
            p, n = rec["parent"], rec["new"]
            rec["same_peaks"] = p["peaks_sha1"] == n["peaks_sha1"] and p["peaks"] == n["peaks"]
            rec["speedup"] = p["median_ms"] / n["median_ms"]
            rec["new_median_below_parent_min"] = n["median_ms"] < p["min_ms"]
            rec["new_within_parent_range"] = p["min_ms"] <= n["median_ms"] <= p["max_ms"]
            ok = ok and rec["same_peaks"]
            result["cases"][c] = rec
            print("%s %-15s parent %8.2f ms [%.2f .. %.2f] path %d rounds %d | new %8.2f ms [%.2f .. %.2f] path %d rounds %d | "
                  "x%.2f | peaks %s (%d) | candidates %d / %d" % (
                      c, "x".join(str(v) for v in CASES[c][0]), p["median_ms"], p["min_ms"], p["max_ms"], p["zx_path"],
                      p["n_pass_rounds"], n["median_ms"], n["min_ms"], n["max_ms"], n["zx_path"], n["n_pass_rounds"],
                      rec["speedup"], "equal" if rec["same_peaks"] else "DIFFER", n["peaks"], p["candidates"],
                      n["candidates"]), flush=True)
        if "a" in result["cases"] and "b" in result["cases"]:
            # the wide rows of this tree against the parent's rows of 512, per voxel processed: parity expected (the
            # per-tile work is the same), up to the parent's own spread on b plus 5 % for the second width class
            a, b = result["cases"]["a"]["new"], result["cases"]["b"]["parent"]
            ratio = (a["median_ms"] / voxels_processed("a")) / (b["median_ms"] / voxels_processed("b"))
            allowed = 1.0 + b["spread_ms"] / b["median_ms"] + 0.05
            result["a_new_vs_b_parent_per_voxel"] = dict(ratio=ratio, allowed=allowed, within=ratio <= allowed)
            print("a (new) against b (parent) per voxel processed: x%.3f (allowed x%.3f)" % (ratio, allowed), flush=True)
    finally:
        for w in builds.values():
            w.close()
    abbench.write_json(args.out, result)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
