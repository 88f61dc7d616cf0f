#!/usr/bin/env python
"""Blocks detected in parts at their real size: a tool, not a test.

    python tools/partsbench.py --out profiles/r09_parts.json [--skip-real] [--skip-cost] [--repeats 10]

real : one resident uint16 block of 843^3 -- the default profile (segment_size 500, sigma factors 3 .. 5, 10 scales) at
       0.6 um / px, kernel radii 20 .. 33 -- which raised "block too large for one workspace slot" before.  Records the
       number of parts, the workspace bytes, n_part_voxels / n_voxels and the device-event time of the batch's enqueue
       (the ``mmx_detect_batch`` call with its table uploads; warm-ups, then median / min / max over the repeats), and
       spot-checks the table against the CPU oracle on four crops of 140^3: three around the cut planes and one at a real
       corner.  A crop is an image of its own to the oracle, so only what lies further than R_max from the crop's cut
       faces says anything about the block: every oracle peak there must be in the table with the same float64 value, and
       the table must hold no other peak there.
cost : 8 resident blocks of 261^3 at kernel radius 16, detected unsplit and force-split 2 x 2 x 2
       (``blob_log.FORCED_PART_GRID``), alternating repeat by repeat: the ratio of the two times beside the voxel overhead
       of the split, ((c + 2 h) / c)^3 with the cores' side c and the halo h -- less where a box ends at a real face."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RES_UM, SEGMENT, FACTORS, NUM_SIGMA = 0.6, 500, (3.0, 5.0), 10
THRESHOLD, OVERLAP = 0.1, 0.5
CROP = 140


def _timed(fn, warmups, repeats):
    import torch
    times = []
    for k in range(warmups + repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        if k >= warmups:
            times.append(t0.elapsed_time(t1))
    return out, dict(median_ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)), repeats=repeats)


def _enqueue_all(bl, dvol, lane, origins, shapes, bufs, splits):
    """The batches of one detection, enqueued back to back (parents one per batch, the others together)."""
    jobs = []
    rest = [i for i in range(len(shapes)) if i not in splits]
    if rest:
        jobs.append(bl._enqueue_detect(dvol, lane, [origins[i] for i in rest], [shapes[i] for i in rest], bufs, 0))
    for i, sp in splits.items():
        jobs.append(bl._enqueue_detect(dvol, lane, [origins[i]], [shapes[i]], bufs, 0, split=sp))
    return jobs


def real(args):
    import torch
    from magellanmapper_amd import blob_log as bl, synth
    from oracle import blob_log_oracle as blo
    dev = torch.device("cuda", 0)
    side = int(np.ceil(SEGMENT / RES_UM)) + 9           # 834 + the overlap the reference adds: 843
    shape = (side,) * 3
    lo, hi = FACTORS[0] / RES_UM, FACTORS[1] / RES_UM
    vol = synth.make_volume_device(shape, 9, dev, density=synth.BLOBS_PER_MVOX / 8.0, blob_sigma=6.0)
    dvol = bl.DeviceVolume(vol)
    stats = bl.BatchStats()
    res, peaks = bl.blob_log_blocks(dvol, 0, [(0, 0, 0)], [shape], lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP, stats=stats,
                                    return_peaks=True)
    lane = bl.Lane(0, lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP)
    lane.bind(dvol, 1)
    radii = [int(r) for r in lane.space.radii]
    sp = bl.split_oversized(shape, bl._slot_limit(), max(radii) + 1)
    bufs = bl._buffers_for(dev)
    nat = bl.nat
    work = int(nat.lib().mmx_workspace_bytes(len(sp), int(bl._slot_elems(sp.box_shapes).max()), NUM_SIGMA, 1))
    _, timing = _timed(lambda: [j.done.synchronize() for j in _enqueue_all(bl, dvol, lane, [(0, 0, 0)], [shape], bufs, {0: sp})],
                       args.warmups, args.repeats)
    out = dict(shape=list(shape), radii=radii, parts=len(sp), grid=list(sp.grid), workspace_bytes=work,
               n_voxels=stats.n_voxels, n_part_voxels=stats.n_part_voxels, voxel_ratio=stats.n_part_voxels / stats.n_voxels,
               peaks=int(len(peaks[0][0])), blobs=int(len(res[0])), zx_path=bl.LAST_ZX_PATH, detect_batch=timing)
    # the oracle on crops: around the cut planes, and at a real corner
    rmax = max(radii)
    coords, values = peaks[0]
    cuts = [[int(c) for c in sp.cuts[ax][1:-1]] for ax in range(3)]
    centre = [cs[0] if cs else side // 2 for cs in cuts]
    starts = [tuple(max(0, min(side - CROP, c - CROP // 2)) for c in centre),
              tuple(max(0, min(side - CROP, c - CROP // 2 + (40 if ax == 0 else 0))) for ax, c in enumerate(centre)),
              tuple(max(0, min(side - CROP, c - CROP // 2 - (40 if ax == 2 else 0))) for ax, c in enumerate(centre)),
              (0, 0, 0)]
    host = vol.cpu().numpy() if hasattr(vol, "cpu") else np.asarray(vol)
    crops = []
    for st in starts:
        crop = host[st[0]:st[0] + CROP, st[1]:st[1] + CROP, st[2]:st[2] + CROP]
        _, stages = blo.blob_log(crop, lo, hi, NUM_SIGMA, THRESHOLD, OVERLAP, return_stages=True)
        o_pk = stages["peaks"].reshape(-1, 4).astype(np.int64)
        o_val = stages["peak_values"].astype(np.float64)
        # interior: further than R_max from the crop's faces that are not faces of the block
        lo_in = np.array([0 if s == 0 else rmax + 1 for s in st])
        hi_in = np.array([CROP if s + CROP == side else CROP - rmax - 1 for s in st])
        inside = ((o_pk[:, :3] >= lo_in) & (o_pk[:, :3] < hi_in)).all(axis=1)
        want = {tuple(int(v) for v in (p[:3] + np.array(st)).tolist() + [p[3]]): float(v)
                for p, v in zip(o_pk[inside], o_val[inside])}
        rel = coords[:, :3] - np.array(st)
        mine = ((rel >= lo_in) & (rel < hi_in)).all(axis=1)
        got = {tuple(int(v) for v in c): float(v) for c, v in zip(coords[mine], values[mine])}
        crops.append(dict(start=list(st), oracle_interior_peaks=len(want), table_interior_peaks=len(got),
                          identical=bool(want == got), missing=len(set(want) - set(got)), extra=len(set(got) - set(want))))
    out["crops"] = crops
    out["crops_identical"] = all(c["identical"] for c in crops)
    return out


def cost(args):
    import torch
    from magellanmapper_amd import blob_log as bl, synth
    dev = torch.device("cuda", 0)
    block, step, radius = 261, 256, 16
    sigma = (radius + 0.2) / 4.0
    side = step + block
    vol = synth.make_volume_device((side,) * 3, 8, dev, density=synth.BLOBS_PER_MVOX / 8.0, blob_sigma=4.0)
    dvol = bl.DeviceVolume(vol)
    origins = [(z, y, x) for z in (0, step) for y in (0, step) for x in (0, step)]
    shapes = [(block,) * 3] * 8
    lane = bl.Lane(0, sigma, sigma, 1, THRESHOLD, OVERLAP)
    lane.bind(dvol, 8)
    bufs = bl._buffers_for(dev)
    sp = bl.split_oversized(shapes[0], int(bl._slot_elems(shapes[0])), radius + 1, grid=(2, 2, 2))
    splits = {i: sp for i in range(8)}
    tables = {}
    for name, how in (("unsplit", {}), ("split", splits)):
        limit = bl.MAX_SLOT_ELEMS
        bl.MAX_SLOT_ELEMS, bl.FORCED_PART_GRID = (int(bl._slot_elems(shapes[0])), (2, 2, 2)) if how else (limit, None)
        try:
            tables[name] = bl.blob_log_blocks(dvol, 0, origins, shapes, sigma, sigma, 1, THRESHOLD, OVERLAP)
        finally:
            bl.MAX_SLOT_ELEMS, bl.FORCED_PART_GRID = limit, None
    same = all(np.array_equal(a, b) for a, b in zip(tables["unsplit"], tables["split"]))
    times = {"unsplit": [], "split": []}
    for k in range(args.warmups + args.repeats):
        for name, how in (("unsplit", {}), ("split", splits)):          # alternating, repeat by repeat
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            jobs = _enqueue_all(bl, dvol, lane, origins, shapes, bufs, how)
            t1.record()
            for j in jobs:
                j.done.synchronize()
            torch.cuda.synchronize()
            if k >= args.warmups:
                times[name].append(t0.elapsed_time(t1))
    med = {k: float(np.median(v)) for k, v in times.items()}
    part_vox = int(sp.box_shapes.prod(axis=1).sum())
    return dict(block=block, radius=radius, halo=radius + 1, tables_identical=bool(same),
                unsplit_ms=dict(median=med["unsplit"], min=min(times["unsplit"]), max=max(times["unsplit"])),
                split_ms=dict(median=med["split"], min=min(times["split"]), max=max(times["split"])),
                measured_ratio=med["split"] / med["unsplit"],
                voxel_overhead=part_vox / float(block ** 3),
                voxel_overhead_unclipped=((block / 2.0 + 2 * (radius + 1)) / (block / 2.0)) ** 3,
                padded_element_overhead=float(8 * int(bl._slot_elems(sp.box_shapes).max())) / float(int(bl._slot_elems(shapes[0]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmups", type=int, default=2)
    ap.add_argument("--skip-real", action="store_true")
    ap.add_argument("--skip-cost", action="store_true")
    args = ap.parse_args()
    out = {}
    if not args.skip_cost:
        out["cost"] = cost(args)
        print(json.dumps({"cost": out["cost"]}), flush=True)
    if not args.skip_real:
        out["real"] = real(args)
        print(json.dumps({"real": out["real"]}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
