#!/usr/bin/env python
"""Wide-row A/B measurement: this tree's libmmx_hip.so against another build of it (the parent commit's), in ONE run,
the two alternating repeat by repeat (the scheme of tools/widebench.py; tools/rowbench.py is the two-channel run of
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
import hashlib
import json
import os
import subprocess
import sys

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
    import numpy as np
    import torch
    from magellanmapper_amd import _native as nat
    from magellanmapper_amd import blob_log as bl, synth
    L = nat.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    vol16 = synth.make_volume_device(VOLUME, 8, dev, density=synth.BLOBS_PER_MVOX / 4.0, blob_sigma=4.5)
    lo, hi = FACTORS[0] / RES_UM, FACTORS[1] / RES_UM
    cap = 1 << 23
    table = torch.zeros(cap * nat.CAND_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    volumes, keep = {}, {}

    def volume_of(as_float):
        if as_float not in volumes:
            volumes[as_float] = bl.DeviceVolume((vol16.to(torch.float32) / 65535.0) if as_float else vol16)
        return volumes[as_float]

    def args_of(name):
        if name not in keep:
            shape, oz, oy, ox, as_float = CASES[name]
            dvol = volume_of(as_float)
            origins = [(z, y, x) for z in oz for y in oy for x in ox]
            shapes = [shape] * len(origins)
            blocks, slot = bl._make_blocks(dvol, 0, origins, shapes)
            d_blocks = bl._to_device_bytes(blocks, dev)
            nb = len(blocks)
            v32, vex = dvol.view(0, True), dvol.view(0, False)
            if as_float:
                v32.value_range = 1.0
            ws = torch.empty(-(-int(L.mmx_workspace_bytes(nb, slot, NUM_SIGMA, 1)) // 4), dtype=torch.float32, device=dev)
            lane = bl.Lane(0, lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP)
            lane.bind(dvol, nb)
            space = lane.space
            a = nat.DetectArgs()
            a.vol32, a.vol_exact = ctypes.pointer(v32), ctypes.pointer(vex)
            a.d_blocks, a.h_blocks, a.n_blocks, a.n_sigma, a.slot_elems = d_blocks.data_ptr(), blocks.ctypes.data, nb, NUM_SIGMA, slot
            a.h_w0, a.h_w2 = space.w0_tab.ctypes.data, space.w2_tab.ctypes.data
            a.d_w0, a.d_w2 = lane.d_w0.data_ptr(), lane.d_w2.data_ptr()
            a.h_radius, a.h_norm = space.radii.ctypes.data, space.norms.ctypes.data
            a.d_work, a.work_bytes, a.thr, a.eps = ws.data_ptr(), ws.numel() * 4, lane.threshold, lane.eps
            a.d_cands, a.cap, a.d_count = table.data_ptr(), cap, count.data_ptr()
            a.zx_mode, a.zx_flags, a.store_f32, a.exact, a.expand = nat.MMX_ZX_AUTO, 0, int(as_float), 1, 1
            a.stream = a.tail_stream = a.pack_stream = stream
            keep.clear()                # (one case's workspace at a time)
            keep[name] = (a, lane, dvol, origins, shapes, (blocks, d_blocks, v32, vex, ws))
        return keep[name]

    def one_call(name):
        a, lane = args_of(name)[:2]
        info = nat.DetectInfo()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
        t1.record()
        nat.check(rc, "mmx_detect_batch")
        torch.cuda.synchronize()
        n_all, n_cands = (int(v) for v in count.cpu().numpy().view(np.uint32))
        assert n_all <= cap, "candidate table too small"
        return dict(ms=t0.elapsed_time(t1), n_pass_rounds=info.n_pass_rounds, mask_layout=info.mask_layout,
                    zx_path=info.zx_path, entries=n_all, candidates=n_cands, radii=[int(r) for r in lane.space.radii])

    for line in sys.stdin:
        req = json.loads(line)
        if req["cmd"] == "quit":
            break
        name = req["case"]
        if req["cmd"] == "run":
            rep = one_call(name)
        else:       # "describe": the kernel families of one call, and the resolved peaks
            nat.timing_enable(True)
            try:
                nat.timing_read()
                rep = one_call(name)
                rep["kinds"] = {k: [ms, int(n)] for k, (ms, n) in nat.timing_read().items() if n}
            finally:
                nat.timing_enable(False)
            _, _, dvol, origins, shapes = args_of(name)[:5]
            _, peaks = bl.blob_log_blocks(dvol, 0, origins, shapes, lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP, return_peaks=True)
            h = hashlib.sha1()
            n_peaks = 0
            for coords, vals in peaks:
                h.update(np.ascontiguousarray(coords).tobytes())
                h.update(np.ascontiguousarray(vals).tobytes())
                n_peaks += len(coords)
            rep["peaks"], rep["peaks_sha1"] = n_peaks, h.hexdigest()
            bl.release_buffers()
        sys.stdout.write(json.dumps(rep) + "\n")
        sys.stdout.flush()


# ---------------------------------------------------------------------------------------------------------- driver
class Worker:
    def __init__(self, lib):
        env = dict(os.environ)
        if lib:
            env["MMX_LIB_PATH"] = os.path.abspath(lib)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker"], stdin=subprocess.PIPE,
                                  stdout=subprocess.PIPE, text=True, env=env, cwd=ROOT)

    def ask(self, **req):
        self.p.stdin.write(json.dumps(req) + "\n")
        self.p.stdin.flush()
        while True:
            line = self.p.stdout.readline()
            if not line:
                raise RuntimeError("worker ended (exit status %s)" % self.p.wait())
            if line.startswith("{"):
                return json.loads(line)

    def close(self):
        try:
            self.p.stdin.write('{"cmd": "quit"}\n')
            self.p.stdin.close()
            self.p.wait(timeout=60)
        except Exception:
            self.p.kill()


def summarise(ms):
    s = sorted(ms)
    n = len(s)
    med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    return dict(median_ms=med, min_ms=s[0], max_ms=s[-1], spread_ms=s[-1] - s[0], repeats=n)


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
    builds = {"parent": Worker(args.parent_lib), "new": Worker(None)}
    result = dict(volume="uint16 %d x %d x %d (z, y, x), 8 blocks per case" % VOLUME, resolution_um=RES_UM,
                  sigma_factors=FACTORS, num_sigma=NUM_SIGMA, threshold=THRESHOLD, warmup=args.warmup, cases={})
    ok = True
    try:
        for c in names:
            rec = dict(block=CASES[c][0], row_pitch=row_pitch(CASES[c][0][2]), float_voxels=CASES[c][4],
                       voxels_processed=voxels_processed(c))
            for b, w in builds.items():
                rec[b] = w.ask(cmd="describe", case=c)          # (also the first warm-up call)
                rec[b]["ms_first"] = rec[b].pop("ms")
            for _ in range(args.warmup):
                for w in builds.values():
                    w.ask(cmd="run", case=c)
            times = {b: [] for b in builds}
            for _ in range(args.repeats):                       # parent, new, parent, new, ...
                for b, w in builds.items():
                    r = w.ask(cmd="run", case=c)
                    times[b].append(r["ms"])
                    for k in ("n_pass_rounds", "mask_layout", "zx_path", "candidates"):
                        assert r[k] == rec[b][k], (c, b, k, r[k], rec[b][k])
            for b in builds:
                rec[b].update(summarise(times[b]), ms=times[b])
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
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
