#!/usr/bin/env python
"""int16 against uint16, and this tree against its parent on an int16 memory map -- a tool, not bench.py.

    python tools/dtypebench.py --repeats 7 --out profiles/r15_int16.json [--parent-root /path/to/parent/checkout]

1. Resident step.  One seeded volume as uint16 ``u`` and as int16 ``u - 32768``, both resident in HBM: the step is
   ``blob_log_blocks`` over its blocks (segment size 256 + overlap, 5 scales sigma 3 .. 5), raw and with ``--denoise``
   (per-block preprocessing, tiles of that size; 0 skips it), the two voxel types ALTERNATING repeat by repeat in one
   process.  The threshold of the int16 run is twice the uint16 one (its image spans [-1, 1]: twice the LoG response
   of the same blob) and ``near_max`` is put below every voxel of either, so both detect the same blobs with the same
   kernels (the int16 copy is ``x ^ 0x8000``, its Y pass adds one constant per scale): a ratio beyond the spread of
   the uint16 runs needs an explanation.
2. Against the parent (``--parent-root``: a checkout of the parent commit with its library built).  The same int16
   memory map, host file to final table (``stack_detect.detect_blobs_blocks``, raw voxels), each tree in a worker
   process of its own, the two alternating.  The parent converts the whole map to float64 on the host first, so the
   volume is sized for that copy to fit.  A gain is stated only if every run of this tree beats every run of the
   parent by more than twice the larger of the two spreads.  The tables are NOT expected to agree to the last row in
   every configuration -- with preprocessing the parent's differ by design; this part runs raw, where they do agree --
   and their digests are recorded.
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import abbench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMA = (3.0, 5.0)
NUM_SIGMA = 5
THRESHOLD, OVERLAP = 0.1, 0.5
SEGMENT, HALO = 256, 25


def block_grid(shape):
    """Blocks of SEGMENT voxels plus HALO on their inner faces, as the stack path cuts them."""
    origins, shapes = [], []
    cuts = [[(max(0, a - HALO), min(n, a + SEGMENT + HALO)) for a in range(0, n, SEGMENT)] for n in shape]
    for z0, z1 in cuts[0]:
        for y0, y1 in cuts[1]:
            for x0, x1 in cuts[2]:
                origins.append((z0, y0, x0))
                shapes.append((z1 - z0, y1 - y0, x1 - x0))
    return origins, shapes


# ------------------------------------------------------------------------------------------------ 1. resident step
def resident(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from magellanmapper_amd import blob_log as bl, config, preprocess, synth
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    shape = tuple(args.shape)
    u16 = synth.make_volume_device(shape, args.seed, dev)
    i16 = (u16.to(torch.int32) - 32768).to(torch.int16)
    vols = {"uint16": bl.DeviceVolume(u16), "int16": bl.DeviceVolume(i16)}
    assert vols["int16"].tensor.element_size() == 2
    origins, shapes = block_grid(shape)
    config.setup_roi_profiles(None)
    out = dict(shape=list(shape), blocks=len(origins), sigma=SIGMA, num_sigma=NUM_SIGMA, threshold_uint16=THRESHOLD,
               threshold_int16=2 * THRESHOLD, cases={})
    for label, dms in (("raw", None), ("denoise%d" % args.denoise, args.denoise)):
        if label != "raw" and not args.denoise:
            continue
        def step(kind):
            pre = None
            if dms:
                # near_max below every voxel: the floor of vmax never bites, for either type
                pre = preprocess.Preprocessor((dms,) * 3, near_max=[-1.0 if kind == "uint16" else -70000.0])
            stats = bl.BatchStats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = bl.blob_log_blocks(vols[kind], 0, origins, shapes, SIGMA[0], SIGMA[1], NUM_SIGMA,
                                     THRESHOLD if (kind == "uint16" or dms) else 2 * THRESHOLD, OVERLAP, pre=pre, stats=stats)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, res, stats
        rec = {}
        times = {k: [] for k in vols}
        for k in vols:
            for _ in range(args.warmup):
                _, res, stats = step(k)
            n, sha = abbench.table_digest(res)
            rec[k] = dict(blobs=n, table_sha1=sha, zx_path=bl.LAST_ZX_PATH, q16_bound=bl.LAST_Q16_BOUND,
                          nms_band=bl.LAST_NMS_BAND, candidates=int(stats.n_candidates))
        for _ in range(args.repeats):                  # uint16, int16, uint16, int16, ...
            for k in vols:
                times[k].append(step(k)[0])
        for k in vols:
            rec[k].update(abbench.summarise(times[k]), ms=times[k])
        u, i = rec["uint16"], rec["int16"]
        rec["int16_over_uint16"] = i["median_ms"] / u["median_ms"]
        rec["uint16_relative_spread"] = u["spread_ms"] / u["median_ms"]
        rec["ratio_within_uint16_spread"] = abs(rec["int16_over_uint16"] - 1.0) <= rec["uint16_relative_spread"]
        out["cases"][label] = rec
        print("%-10s uint16 %8.2f ms [%.2f .. %.2f] path %s blobs %d | int16 %8.2f ms [%.2f .. %.2f] path %s blobs %d | "
              "x%.3f (uint16 spread %.3f)" % (label, u["median_ms"], u["min_ms"], u["max_ms"], u["zx_path"], u["blobs"],
                                              i["median_ms"], i["min_ms"], i["max_ms"], i["zx_path"], i["blobs"],
                                              rec["int16_over_uint16"], rec["uint16_relative_spread"]), flush=True)
        bl.release_buffers()
    return out


# --------------------------------------------------------------------------------------------- 2. against the parent
def worker(root, path):
    """One tree (``root``) detecting the memory map at ``path`` on request: a line in, a JSON line out."""
    import numpy as np
    sys.path.insert(0, root)
    import torch
    from magellanmapper_amd import config, stack_detect
    torch.cuda.set_device(0)
    os.chdir(tempfile.mkdtemp(prefix="dtypebench_"))
    config.setup_roi_profiles(None)
    config.roi_profile.update(num_sigma=NUM_SIGMA, segment_size=SEGMENT, denoise_size=None)
    for p in config.roi_profiles:
        p.update(config.roi_profile)
    config.resolutions = np.array([[1.0, 1.0, 1.0]])
    config.filename = "dtypebench"
    config.near_max = [-1.0]

    def run(req):
        img = np.load(path, mmap_mode="r")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, blobs = stack_detect.detect_blobs_blocks("dtypebench", stack_detect.Image5d(img), None, None, None,
                                                       False, False, True, False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        n, sha = abbench.table_digest([blobs.blobs] if blobs.blobs is not None else [])
        return dict(ms=ms, blobs=n, table_sha1=sha)
    abbench.serve(dict(describe=run, run=run))


def make_map(path, shape, seed):
    """The seeded benchmark volume as int16 (``u - 32768``) in a ``(1, z, y, x)`` .npy file."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from magellanmapper_amd import synth
    dev = torch.device("cuda", 0)
    u16 = synth.make_volume_device(tuple(shape), seed, dev)
    np.save(path, (u16.to(torch.int32) - 32768).to(torch.int16).cpu().numpy()[None])


def against_parent(args):
    import numpy as np
    shape = tuple(args.map_shape)
    tmp = tempfile.mkdtemp(prefix="dtypebench_map_")
    path = os.path.join(tmp, "int16_image5d.npy")
    # (the seeded generator runs on the device, in a child that is gone before the workers start)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--make-map", path, "--map-shape",
                           *[str(v) for v in shape], "--seed", str(args.seed)], cwd=ROOT)
    env = dict(os.environ)
    env.pop("MMX_LIB_PATH", None)
    builds = {b: abbench.Worker(os.path.abspath(__file__), ["--worker", root, path], env=env, cwd=root)
              for b, root in (("parent", os.path.abspath(args.parent_root)), ("tree", ROOT))}
    out = dict(shape=list(shape), bytes_int16=int(np.prod(shape)) * 2, bytes_float64=int(np.prod(shape)) * 8,
               workload="read-only int16 memory map -> stack_detect.detect_blobs_blocks (raw voxels) -> final table")
    last = {}

    def keep_last(b, reply, _):
        last[b] = reply
    try:
        # (the first run of each is also a warm-up)
        first, times = abbench.alternate(builds, list(builds), None, max(0, args.warmup - 1), args.repeats, check=keep_last)
        for b in builds:
            out[b] = dict(abbench.summarise(times[b]), ms=times[b], blobs=last[b]["blobs"],
                          table_sha1=last[b]["table_sha1"], first_ms=first[b]["ms"])
    finally:
        for w in builds.values():
            w.close()
        try:
            os.remove(path)
            os.rmdir(tmp)
        except OSError:
            pass
    p, t = out["parent"], out["tree"]
    margin = 2.0 * max(p["spread_ms"], t["spread_ms"])
    out["same_table"] = p["table_sha1"] == t["table_sha1"]
    out["speedup_of_medians"] = p["median_ms"] / t["median_ms"]
    out["gain_stated"] = bool(t["max_ms"] + margin < p["min_ms"])
    print("memory map %s: parent %8.1f ms [%.1f .. %.1f] | tree %8.1f ms [%.1f .. %.1f] | x%.2f | gain %s | tables %s "
          "(%d / %d blobs)" % ("x".join(str(v) for v in shape), p["median_ms"], p["min_ms"], p["max_ms"], t["median_ms"],
                               t["min_ms"], t["max_ms"], out["speedup_of_medians"],
                               "stated" if out["gain_stated"] else "NOT stated", "equal" if out["same_table"] else "differ",
                               p["blobs"], t["blobs"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", nargs=2, metavar=("ROOT", "NPY"), help=argparse.SUPPRESS)
    ap.add_argument("--make-map", metavar="NPY", help=argparse.SUPPRESS)
    ap.add_argument("--shape", type=int, nargs=3, default=(512, 1024, 1024), help="resident volume, z y x")
    ap.add_argument("--map-shape", type=int, nargs=3, default=(256, 1024, 1024), help="memory-mapped volume, z y x")
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--denoise", type=int, default=25, metavar="SIZE", help="tile size of the preprocessed run (0: raw only)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit, its libmmx_hip.so built")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.worker:
        return worker(*args.worker)
    if args.make_map:
        return make_map(args.make_map, args.map_shape, args.seed)
    result = dict(tool="tools/dtypebench.py", repeats=args.repeats, warmup=args.warmup, seed=args.seed)
    if args.parent_root:
        # (before this process opens the GPU itself: three processes on the device at the most)
        result["against_parent"] = against_parent(args)
    result["resident"] = resident(args)
    abbench.write_json(args.out, result)
    return 0


if __name__ == "__main__":
    sys.exit(main())
