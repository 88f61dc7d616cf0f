#!/usr/bin/env python3
"""Digests of what the matrix-core Y pass (``ym_kernel``) writes, for tests/test_gpu_y_kblock_loop.py.

    python tests/golden/make_y_kblock_digests.py --commit <commit the library was built from>

writes tests/golden/y_kblock_digests.json: per case and array the SHA-1 of the bytes that ``mmx_log_scales_f32`` (with
entries) or ``mmx_log_batch_f32`` (without) leaves in a workspace zeroed before the call -- every scale's LoG array and
every scale's NMS entries.  Needs a GPU and the library built in-tree.  The cases are stated here once; the test imports
this file for them, so fixture and test cannot drift apart.

The k-block loop of ``ym_kernel`` consumes 32 input rows and finishes two output tiles of 16 rows per turn; what a
change of its structure can get wrong depends on the parity of the number of turns, on the last turn, on a partial last
tile and on tiles with nothing above the threshold.  Hence the y extents: 2 .. 5 row tiles and, with
``turns = (tiles + NB - 3) // 2 + 1``, both parities for each of NB = 3, 4, 5 (the block offsets of radius <= 8, 16, 24).
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "y_kblock_digests.json")

#: (nz, ny, nx): nz = 30 / 33 ends in a z quarter of 2 planes / 1 plane, nx = 29 / 37 in a partial column tile; every
#: extent is >= 24 + MMX_COL_PREFETCH, as the tiled route requires at the largest radius
SHAPES = [(30, 29, 29), (33, 32, 37), (30, 33, 37), (33, 48, 29), (30, 49, 29), (33, 64, 37), (30, 65, 37), (33, 80, 29)]
#: (min_sigma, max_sigma, num_sigma): radius 8 (NB 3); radii 12 and 16 (NB 4); radii 17 and 24 (NB 5)
LADDERS = {"nb3": (2.0, 2.0, 1), "nb4": (3.0, 4.0, 2), "nb5": (4.25, 6.0, 2)}
RADII = {"nb3": [8], "nb4": [12, 16], "nb5": [17, 24]}
#: volume -> (threshold, band, block origins)
VOLUMES = {
    "synth": (0.1, 2.5e-4, [(0, 0, 0), (3, 2, 7), (7, 1, 4), (2, 4, 11), (5, 0, 2), (1, 3, 9), (6, 2, 0), (4, 1, 13)]),
    "sparse": (0.02, 2.5e-4, [(0, 0, 0), (3, 0, 7), (7, 0, 4), (2, 0, 11), (5, 0, 2), (1, 0, 9), (6, 0, 0), (4, 0, 13)]),
}
#: case -> (volume, ladder, with entries)
CASES = {}
for _lad in LADDERS:
    CASES["synth_%s" % _lad] = ("synth", _lad, True)
    CASES["sparse_%s" % _lad] = ("sparse", _lad, True)
    CASES["synth_%s_nomask" % _lad] = ("synth", _lad, False)

_VOLUMES = {}


def volume(name):
    """``synth``: ``synth.make_volume``.  ``sparse``: small blobs on the rows y = 7, 40 and 72 only (every block starts
    at y = 0), so that the row tiles 16 .. 31 and 48 .. 63 of a column hold nothing above the threshold between tiles
    that do, and columns away from the blobs hold nothing at all."""
    from magellanmapper_amd import synth
    if name not in _VOLUMES:
        if name == "synth":
            _VOLUMES[name] = synth.make_volume(19, (40, 84, 50), 90)
        else:
            centres = [(z, y, x) for z in (6, 19, 31) for y in (7, 40, 72) for x in (6, 19, 31, 43)]
            _VOLUMES[name] = synth.make_volume(23, (40, 80, 50), centres=np.array(centres, dtype=float), amp=23000.0,
                                               blob_sigma=2.0)
    return _VOLUMES[name]


def entry_words(b, s):
    """The NMS entries of scale ``s`` of RawBatch ``b`` as ``[(n_blocks * slot) >> 5][2]`` uint64 (candidates, above)."""
    off = b.entries_base - b.ws.data_ptr()
    assert off % 4 == 0, off
    per = (b.nb * b.slot) >> 5
    lo = off // 4 + s * per * 4
    return b.ws[lo:lo + per * 4].cpu().numpy().view(np.uint64).reshape(-1, 2)


def rows_above(b, words):
    """Per block ``[y][z quad][column tile]``: whether the entry says the row's 64 values hold one above the threshold."""
    out = []
    for i, (nz, ny, nx) in enumerate(b.shapes):
        ntx, nzq = -(-nx // 16), -(-nz // 4)
        out.append(words[(i * b.slot) >> 5:][:ny * nzq * ntx].reshape(ny, nzq, ntx, 2)[..., 1] != 0)
    return out


def run_case(case, y_valu=False):
    """One case on the GPU: ``(RawBatch, {array name: host array})`` with ``log<s>`` the LoG array of scale ``s`` (float32,
    the whole batch) and, with entries, ``ent<s>`` its entry words."""
    import torch
    from magellanmapper_amd import _native as nat
    from magellanmapper_amd.rawbatch import RawBatch
    vol, lad, entries = CASES[case]
    thr, eps, origins = VOLUMES[vol]
    b = RawBatch(volume(vol), origins, SHAPES, LADDERS[lad], thr, eps, 0, zx_mode=nat.MMX_ZX_TILED_Q16,
                 zx_flags=nat.MMX_ZX_Y_VALU if y_valu else 0, exact=0, expand=0)
    assert [int(r) for r in b.space.radii] == RADII[lad], (lad, b.space.radii)
    b.ws.zero_()
    if entries:
        info = b.log_scales(b.args(d_cands=None, d_count=None))
        assert (info.zx_path, info.mask_layout) == (nat.MMX_ZX_TILED_Q16, nat.MMX_MASK_QUADS), (info.zx_path, info.mask_layout)
    else:
        mode = nat.MMX_ZX_TILED_Q16 | (nat.MMX_ZX_Y_VALU if y_valu else 0)
        for s in range(b.ns):
            path = b.log_batch(s, mode)
            assert path == nat.MMX_ZX_TILED_Q16, path
    torch.cuda.synchronize()
    arrays = {}
    logs = b.log_arrays()
    for s in range(b.ns):
        arrays["log%d" % s] = np.ascontiguousarray(logs[s])
        if entries:
            arrays["ent%d" % s] = np.ascontiguousarray(entry_words(b, s))
    return b, arrays


def digests(arrays):
    return {k: hashlib.sha1(v.tobytes()).hexdigest() for k, v in sorted(arrays.items())}


def main():
    sys.path.insert(0, ROOT)
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library under magellanmapper_amd/ was built from")
    ap.add_argument("--out", default=FIXTURE)
    a = ap.parse_args()
    out = dict(commit=a.commit, what="SHA-1 of the bytes ym_kernel leaves per case and array (workspace zeroed before the call)",
               cases={})
    for case in sorted(CASES):
        _, arrays = run_case(case)
        out["cases"][case] = digests(arrays)
        print(case, {k: (int(np.count_nonzero(v)), v.size) for k, v in arrays.items()})
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
