#!/usr/bin/env python
"""Wide-radius A/B measurement: this tree's libmmx_hip.so against another build of it (the parent commit's), in ONE
run, the two alternating repeat by repeat.

    python tools/widebench.py --parent-lib /path/to/parent/libmmx_hip.so --repeats 10 --out profiles/r08_wide_radius.json

What is run (bench.py is left alone: its flagship volume sits at 1 um / px, below the wide radii):
  ladder : one batch of 8 resident uint16 blocks of 261^3 with the stock factors 3 .. 5 at 0.65 um / px in 10 scales
           (sigma 4.62 .. 7.69 px, radii 18 .. 31), through ``mmx_detect_batch``;
  R25, R31, R48, R64 : the same batch with the single scale sigma = (R + 0.2) / 4.
Per case and build: device-event milliseconds per ``mmx_detect_batch`` call after warm-up (median, min, max over the
repeats), ``n_pass_rounds`` / entry layout / kernel path, the kernel families that ran (one extra call with the
per-kernel events on), the number of nominated candidates, and a digest of the resolved peaks (``blob_log_blocks``:
coordinates and float64 values) -- which must be equal between the two builds.  For the single scales of this tree the
achieved FMA rate of the three wide passes against the float32 vector peak, from the operation counts below.

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

RES_UM = 0.65
FACTORS = (3.0, 5.0)
NUM_SIGMA = 10
BLOCK = 261
STEP = 256
SINGLE_RADII = (25, 31, 48, 64)
THRESHOLD, OVERLAP = 0.1, 0.5
PEAK_F32_VECTOR_TFLOPS = 157.3        # MI355X, float32 vector (spec)
WIDE_J = 8                            # outputs per thread along the filter axis (csrc/mmx_wide.hip: kJ)


def cases():
    out = {"ladder": (FACTORS[0] / RES_UM, FACTORS[1] / RES_UM, NUM_SIGMA)}
    for r in SINGLE_RADII:
        s = (r + 0.2) / 4.0
        out["R%d" % r] = (s, s, 1)
    return out


def wide_fma_per_voxel(radius):
    """FMA (one multiply-add on one float) per voxel and sigma of the three wide passes: a run of J outputs reads
    J + 2 R inputs rounded up to whole steps of J, and every input feeds each of its J outputs once -- in Z on the pair
    (Gz, Gzz) (2 FMA), in X on the pair (P, Q's second term) and on Q's first term (3), in Y on the pair (2)."""
    ni = -(-(WIDE_J + 2 * radius) // WIDE_J) * WIDE_J
    return 7 * ni


# ---------------------------------------------------------------------------------------------------------- worker
def worker():
    import ctypes
    import numpy as np
    import torch
    from magellanmapper_amd import _native as nat
    # (the other build may be of the ABI before this one: same entry points, one timing family fewer)
    nat.MMX_ABI_VERSION = ctypes.CDLL(nat.LIB_PATH).mmx_abi_version()
    from magellanmapper_amd import blob_log as bl, synth
    L = nat.lib()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    side = STEP + BLOCK
    vol = synth.make_volume_device((side, side, side), 8, dev, density=synth.BLOBS_PER_MVOX / 8.0, blob_sigma=6.0)
    dvol = bl.DeviceVolume(vol)
    origins = [(z, y, x) for z in (0, STEP) for y in (0, STEP) for x in (0, STEP)]
    shapes = [(BLOCK,) * 3] * 8
    blocks, slot = bl._make_blocks(dvol, 0, origins, shapes)
    d_blocks = bl._to_device_bytes(blocks, dev)
    nb = len(blocks)
    v32, vex = dvol.view(0, True), dvol.view(0, False)
    ws = torch.empty(-(-int(L.mmx_workspace_bytes(nb, slot, NUM_SIGMA, 1)) // 4), dtype=torch.float32, device=dev)
    cap = 1 << 22
    table = torch.zeros(cap * nat.CAND_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    count = torch.zeros(2, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    keep = {}

    def args_of(name):
        if name not in keep:
            lo, hi, ns = cases()[name]
            lane = bl.Lane(0, lo, hi, ns, THRESHOLD, OVERLAP)
            lane.bind(dvol, nb)
            space = lane.space
            a = nat.DetectArgs()
            a.vol32, a.vol_exact = ctypes.pointer(v32), ctypes.pointer(vex)
            a.d_blocks, a.h_blocks, a.n_blocks, a.n_sigma, a.slot_elems = d_blocks.data_ptr(), blocks.ctypes.data, nb, ns, slot
            a.h_w0, a.h_w2 = space.w0_tab.ctypes.data, space.w2_tab.ctypes.data
            a.d_w0, a.d_w2 = lane.d_w0.data_ptr(), lane.d_w2.data_ptr()
            a.h_radius, a.h_norm = space.radii.ctypes.data, space.norms.ctypes.data
            a.d_work, a.work_bytes, a.thr, a.eps = ws.data_ptr(), ws.numel() * 4, lane.threshold, lane.eps
            a.d_cands, a.cap, a.d_count = table.data_ptr(), cap, count.data_ptr()
            a.zx_mode, a.zx_flags, a.store_f32, a.exact, a.expand = nat.MMX_ZX_AUTO, 0, 0, 1, 1
            a.stream = a.tail_stream = a.pack_stream = stream
            keep[name] = (a, lane)
        return keep[name]

    def one_call(name):
        a, lane = args_of(name)
        info = nat.DetectInfo()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rc = L.mmx_detect_batch(ctypes.byref(a), ctypes.byref(info))
        t1.record()
        nat.check(rc, "mmx_detect_batch")
        torch.cuda.synchronize()
        n_all, n_cands = (int(v) for v in count.cpu().numpy().view(np.uint32))
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
            lo, hi, ns = cases()[name]
            _, peaks = bl.blob_log_blocks(dvol, 0, origins, shapes, lo, hi, ns, THRESHOLD, OVERLAP, return_peaks=True)
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
    ap.add_argument("--cases", default=",".join(cases()))
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
        if c not in cases():
            ap.error("unknown case %s" % c)
    builds = {"parent": Worker(args.parent_lib), "new": Worker(None)}
    result = dict(volume="uint16 %d^3, 8 blocks of %d^3" % (STEP + BLOCK, BLOCK), resolution_um=RES_UM,
                  threshold=THRESHOLD, peak_f32_vector_tflops=PEAK_F32_VECTOR_TFLOPS, cases={})
    voxels = 8 * BLOCK ** 3
    ok = True
    try:
        for c in names:
            rec = {}
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
            rec["same_candidate_count"] = p["candidates"] == n["candidates"]
            rec["speedup"] = p["median_ms"] / n["median_ms"]
            # faster by more than the spread: the slowest new repeat beats the fastest parent repeat
            rec["faster_beyond_spread"] = n["max_ms"] < p["min_ms"]
            ok = ok and rec["same_peaks"]
            wide = n.get("kinds", {}).get("widepass")
            if wide and len(n["radii"]) == 1:
                fma = wide_fma_per_voxel(n["radii"][0]) * voxels
                tflops = 2.0 * fma / (wide[0] * 1e-3) / 1e12
                rec["wide_passes"] = dict(ms=wide[0], fma_per_voxel=wide_fma_per_voxel(n["radii"][0]), tflops=tflops,
                                          share_of_f32_vector_peak=tflops / PEAK_F32_VECTOR_TFLOPS)
            result["cases"][c] = rec
            print("%-7s parent %8.2f ms [%.2f .. %.2f] rounds %d | new %8.2f ms [%.2f .. %.2f] rounds %d | x%.2f | "
                  "peaks %s (%d) | candidates %d / %d%s" % (
                      c, p["median_ms"], p["min_ms"], p["max_ms"], p["n_pass_rounds"], n["median_ms"], n["min_ms"],
                      n["max_ms"], n["n_pass_rounds"], rec["speedup"], "equal" if rec["same_peaks"] else "DIFFER",
                      n["peaks"], p["candidates"], n["candidates"],
                      " | wide passes %.1f%% of peak" % (100 * rec["wide_passes"]["share_of_f32_vector_peak"])
                      if "wide_passes" in rec else ""), flush=True)
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
