#!/usr/bin/env python3
"""Digests of what the Z+X kernel and the Y pass behind it write, for tests/test_gpu_zx_row_march.py.

    MMX_LIB_PATH=<library of the parent commit> python tests/golden/make_zx_row_march_digests.py --commit <that commit>

writes tests/golden/zx_row_march_digests.json: per case the SHA-1 of the tile dwords of the real voxels and of the LoG
values, block after block, as ``mmx_log_batch_f32`` leaves them on 16-bit tiles over a workspace pre-filled with a
pattern.  Needs a GPU.  The cases are stated here once; the test imports this file for them.

The row march (``mmx_fused4.hip``) gives a wave of the pair kernel (radius 9 .. 16) several rows of its column.  What it
can get wrong depends on the rows of a block against the rows per wave (a short last run, exactly one run, one row
more), on the z tiles of a row (their parity: the ring of two across a row change; the last tile's real planes), on the
edge tables at the row change (no steady step; one ring of them) and on the width (an odd tile alone, a pair and an odd
tile).  The split-tile kernel (radius 17 .. 24) and depths whose edge tables do not fit the LDS keep the one-row march
under every value of the field; their cases pin that.

Every block must pass the tiled route: ny >= R + MMX_COL_PREFETCH (the Y pass) and nx, nz >= R.  Hence ny from R + 4 up
rather than from 1: R + 4, R + 5, and a pair (24, 25) or (32, 33) -- a multiple of 2, 4, 8 (24: of 3 as well; 33 is one
of 3) and one row more.  At radius 9, 13 rows under 15 rows per wave are the block with fewer rows than a wave takes.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "zx_row_march_digests.json")

SIGMA_OF = {9: 2.25, 12: 3.0, 16: 4.0, 17: 4.25, 20: 5.0, 24: 6.0}
MAX_NZ = 128
NX = 40
NY_MAX = 33
PATTERN = 0x5A5AC3C3
#: (radius, voxel type): both types through the pair kernel and through the split-tile kernel once, uint16 everywhere
CASES = [(R, "u16") for R in SIGMA_OF] + [(12, "u8"), (20, "u8")]
#: rows per wave forced through the flag field (0: the launch's own choice); 15 at radius 9 only (13 rows < 15)
FORCED = (1, 2, 3, 4, 8)


def march(nz, R):
    """(steady steps, edge output tiles, z tiles) of a block nz deep in the one-row march of zx4_kernel: a ring of two z
    tiles in flight, one output tile LA steps behind, steady steps in whole rings (radius <= 16) or turns of four."""
    LA = 1 if R <= 16 else 2
    group = 2 if LA == 1 else 4
    ntz = (nz + 15) // 16
    u_lo, u_hi = (R + 15) // 16, (nz - 16 - R) // 16
    tA = -(-(u_lo + LA) // 2) * 2
    nB = min(u_hi + LA + 1, ntz) - tA
    nB = nB // group * group if nB > 0 else 0
    hi0 = max(u_hi + 1, u_lo)
    return nB, u_lo + max(ntz - hi0, 0), ntz


def fits(nz, R):
    """The block's edge tables fit the kernel's LDS (``zx4_edges_fit``): three tiles at radius <= 16, four above."""
    return march(nz, R)[1] <= (3 if R <= 16 else 4)


def depths(R):
    """nz = R + 1 (no steady step); the least depth with one ring or turn of steady steps; 65, 69 and 96 planes: five and
    six z tiles -- an odd and an even count, the ring's phase across a row change -- whose last tile has 1, 5 and 16 real
    planes; at radius 20, 65 planes do not fit the LDS form."""
    group = 2 if R <= 16 else 4
    one = min(nz for nz in range(R + 1, MAX_NZ + 1) if march(nz, R)[0] == group)
    return sorted({R + 1, one, 65, 69, 96})


def rows(R):
    m = R + 4
    return [m, m + 1] + ([24, 25] if m < 24 else [32, 33])


def widths(R):
    return (max(17, R + 1) if R > 17 else 17, NX)


def shapes(R, batch):
    """The blocks of one batch: every depth at R + 4 rows and 40 columns; an odd and an even count of z tiles at every
    row count and both widths."""
    out = [(nz, R + 4, NX) for nz in batch]
    odd = [nz for nz in batch if march(nz, R)[2] & 1 and nz > R + 1]
    even = [nz for nz in batch if not march(nz, R)[2] & 1 and nz > R + 1]
    for nz in odd[-1:] + even[-1:]:
        out += [(nz, ny, nx) for ny in rows(R) for nx in widths(R) if (nz, ny, nx) not in out]
    return out


def batches(R):
    """The depths whose edge tables fit in one batch (a batch takes the LDS form only when all of its depths fit), the
    others in a second."""
    d = depths(R)
    return [b for b in ([nz for nz in d if fits(nz, R)], [nz for nz in d if not fits(nz, R)]) if b]


#: the mixed batch under the launch's own choice: many small blocks, two depth classes and two widths, enough wave-rows
#: for the rule to give the first blocks several rows per wave and the last ones one
TAPER_R = 9
TAPER_SHAPES = [(26, 13, NX), (33, 14, 17), (26, 16, NX)] * 240


class Volumes:
    def __init__(self):
        from magellanmapper_amd import blob_log as bl
        rng = np.random.default_rng(2010)
        shape = (MAX_NZ, NY_MAX, NX)
        self.host = {"u16": rng.integers(0, 65536, shape, dtype=np.uint16), "u8": rng.integers(0, 256, shape, dtype=np.uint8)}
        self.dev = {k: bl.DeviceVolume(v) for k, v in self.host.items()}


def space(R):
    from magellanmapper_amd import blob_log as bl
    sp = bl.ScaleSpace.make(SIGMA_OF[R], SIGMA_OF[R], 1)
    assert sp.radii[0] == R
    return sp


def run(vols, kind, R, shp, flags):
    """One batch of blocks through ``mmx_log_batch_f32`` on 16-bit tiles, over a workspace pre-filled with PATTERN:
    ``(LoG arrays, tile dwords of the real voxels per block, the tile half of the workspace, tile stride)``."""
    import torch
    from magellanmapper_amd import _native as nat, blob_log as bl
    L = nat.lib()
    dvol = vols.dev[kind]
    dvol.wait_all()
    dev = dvol.tensor.device
    sp = space(R)
    blocks, slot = bl._make_blocks(dvol, 0, [(0, 0, 0)] * len(shp), list(shp))
    nb = len(blocks)
    ws = torch.full((5 * nb * slot,), PATTERN, dtype=torch.int32, device=dev)
    d_blocks = bl._to_device_bytes(blocks, dev)
    v32 = dvol.view(0, True)
    path = ctypes.c_int(0)
    log_base = ws.data_ptr() + 4 * nb * slot * 4
    nat.check(L.mmx_log_batch_f32(ctypes.byref(v32), d_blocks.data_ptr(), blocks.ctypes.data, nb, slot,
                                  nat.as_double_ptr(sp.w0[0]), nat.as_double_ptr(sp.w2[0]), R, float(sp.norms[0]),
                                  log_base, ws.data_ptr(), None, 0.0, 0.0, None, nat.MMX_ZX_TILED_Q16 | flags,
                                  ctypes.byref(path), torch.cuda.current_stream().cuda_stream), "mmx_log_batch_f32")
    torch.cuda.synchronize()
    assert path.value == nat.MMX_ZX_TILED_Q16, (kind, R, path.value)
    stride = max(-(-nx // 16) * -(-nz // 16) * ny * 256 for nz, ny, nx in shp)       # (mmx_zx6_plan_make: tile_stride)
    half = ws[:2 * nb * stride].cpu().numpy().view(np.uint32)
    logs = ws[4 * nb * slot:].cpu().numpy().view(np.float32).reshape(nb, slot)
    cubes, tiles = [], []
    for i, (nz, ny, nx) in enumerate(shp):
        px = int(blocks["px"][i])
        cubes.append(logs[i, :nz * ny * px].reshape(nz, ny, px)[..., :nx].copy())
        ntx, ntz = -(-nx // 16), -(-nz // 16)
        # tile (y, c, U) at ((y ntx + c) ntz + U) x 256 dwords, 16 planes x 16 columns row-major
        t = half[i * stride:i * stride + ny * ntx * ntz * 256].reshape(ny, ntx, ntz, 16, 16)
        tiles.append(t.transpose(2, 3, 0, 1, 4).reshape(ntz * 16, ny, ntx * 16)[:nz, :, :nx].copy())
    return cubes, tiles, half, stride


def digest(arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def case_name(R, kind, i):
    return "R%d_%s_batch%d" % (R, kind, i)


def main():
    sys.path.insert(0, ROOT)
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library (MMX_LIB_PATH) was built from")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    vols = Volumes()
    out = dict(commit=a.commit, what="SHA-1 of the tile dwords of the real voxels / of the LoG values, block after block", cases={})
    for R, kind in CASES:
        for i, batch in enumerate(batches(R)):
            cubes, tiles, _, _ = run(vols, kind, R, shapes(R, batch), 0)
            out["cases"][case_name(R, kind, i)] = dict(tiles=digest(tiles), log=digest(cubes))
    cubes, tiles, _, _ = run(vols, "u16", TAPER_R, TAPER_SHAPES, 0)
    out["cases"]["taper"] = dict(tiles=digest(tiles), log=digest(cubes))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases" % len(out["cases"]))


if __name__ == "__main__":
    main()
