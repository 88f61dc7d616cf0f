"""GPU tests of the candidate path against the brute-force reference of tests/test_nms_host.py: ``peaks_kernel`` and
``peaks_sparse_kernel`` (csrc/mmx_peaks.hip) and ``expand_probes_kernel`` (csrc/mmx_rescore.hip) on synthetic cubes
written straight into the workspace -- no LoG kernel runs in parts 1-4 --, the closed loop DESIGN.md section 2 rests on
(nominate -> expand -> ``mmx_host_resolve_peaks`` = ``peak_local_max`` of the exact cube), and the NMS entries the five
real producers write, against the contract include/mmx.h states for them.  Needs a real MI355X (``-m gpu``).

Everything goes through ``_native.lib()`` / ctypes.  Every cube value is a multiple of 2^-16 and the band is 2^-12, so
each comparison of parts 1-4 is for equality; the cases, and the proof that each holds what its test relies on, are in
the host file.  One device run per case (and entry layout, word-0 choice, table capacity) is shared by the tests.

Two things the tests do not do.  (i) A batch whose slots are a permutation of the block indices: the library requires
``slot == index`` (``mmx_batch_geom_make``, "block i owns slot i") and refuses anything else with MMX_ERR_ARG, which
``test_a_batch_whose_slots_are_permuted_is_refused`` pins; there is then no unused slot either, so the poison (NaN and
1e30 in turn) sits in the pitch columns, the slot tails (``slot_elems`` is larger than the largest block) and the
unstored segments.  (ii) ``rounds > 1`` in ``peaks_sparse_kernel``: the grid covers a block's entry words in one round
until a batch holds more than 8192 x 2048 = 2^24 of them per block, which no test-sized batch does; that loop-carried
path is left uncovered."""
import ctypes

import numpy as np
import pytest

import test_nms_host as H
from test_nms_host import DENSE, MAX_DELTA, QUADS, ROWS, SPARSE, case
from gpu_support import cand_key, gpu  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64                              # rows behind a table's capacity that no kernel may touch
CAP = 1 << 16
_LAYOUTS = {None: "dense", ROWS: "rows", QUADS: "quads"}
#: every (case, entry layout) of parts 1-4: the dense kernel on the dense cases, the sparse one on both layouts
RUNS = [(n, None) for n in DENSE] + [(n, lay) for n in SPARSE for lay in (ROWS, QUADS)]
RUN_IDS = ["%s-%s" % (n, _LAYOUTS[lay]) for n, lay in RUNS]


def _blocks(shapes, slots=None):
    from magellanmapper_amd import _native as nat
    blocks = np.zeros(len(shapes), dtype=nat.BLOCK_DTYPE)
    for i, (nz, ny, nx) in enumerate(shapes):
        blocks[i] = (0, nz, ny, nx, i if slots is None else slots[i], H.pitch(nx), 0)
    return blocks


class _Run:
    """``mmx_peaks_batch`` then ``mmx_expand_probes`` on one case: the table and the counters after either call."""


_RUNS = {}


def _run(dev, name, layout=None, word0="same", cap=CAP):
    key = (name, layout, word0, cap)
    if key in _RUNS:
        return _RUNS[key]
    from magellanmapper_amd import _native as nat, blob_log as bl
    L, c = nat.lib(), case(name)
    nb, ns, slot = len(c.shapes), c.ns, c.slot_elems
    assert slot % 32 == 0 and slot > max(s[0] * s[1] * H.pitch(s[2]) for s in c.shapes)
    r = _Run()
    r.blocks = _blocks(c.shapes)
    d_blocks = bl._to_device_bytes(r.blocks, dev)
    log = torch.from_numpy(H.pack_log(c.cubes, slot, c.stored(layout))).to(dev)
    masks = None
    if layout is not None:
        ent = H.pack_entries([e for e, _ in c.entries(layout, word0)], slot)
        masks = torch.from_numpy(ent.view(np.int64)).to(dev)
        assert masks.data_ptr() % 16 == 0
    item = nat.CAND_DTYPE.itemsize
    table = torch.full(((cap + GUARD) * item,), 0xA5, dtype=torch.uint8, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    n_cands = torch.full((1,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    nat.check(L.mmx_peaks_batch(log.data_ptr(), masks.data_ptr() if masks is not None else None, layout or 0, ns,
                                d_blocks.data_ptr(), r.blocks.ctypes.data, nb, slot, c.thr, c.eps, table.data_ptr(), cap,
                                count.data_ptr(), stream), "mmx_peaks_batch")
    torch.cuda.synchronize()
    r.count = int(count.item())
    r.nominated = table.cpu().numpy().view(nat.CAND_DTYPE).copy()
    nat.check(L.mmx_expand_probes(table.data_ptr(), cap, count.data_ptr(), n_cands.data_ptr(), d_blocks.data_ptr(), nb, ns,
                                  stream), "mmx_expand_probes")
    torch.cuda.synchronize()
    r.total, r.n_cands = int(count.item()), int(n_cands.item())
    r.expanded = table.cpu().numpy().view(nat.CAND_DTYPE).copy()
    r.cap = cap
    _RUNS[key] = r
    return r


def _order(rows):
    return np.lexsort(cand_key(rows).T[::-1])


def _guard_is_intact(table, cap):
    return bool((table[cap:].view(np.uint8) == 0xA5).all())


def _assert_rows_equal(got, want, banded):
    """Candidate rows in the same order: place, value, nbr_max and flags bit for bit, the band, v64 still NaN."""
    np.testing.assert_array_equal(cand_key(got), cand_key(want))
    np.testing.assert_array_equal(got["v"].view(np.uint32), want["v"].view(np.uint32))
    np.testing.assert_array_equal(got["nbr_max"].view(np.uint32), want["nbr_max"].view(np.uint32))
    np.testing.assert_array_equal(got["flags"], want["flags"])
    np.testing.assert_array_equal(got["band"], want["band"])
    assert np.isnan(got["v64"]).all()
    if banded:
        assert (got["flags"] & H.BAND).all()
    else:
        assert not (got["flags"] & ~np.uint32(H.CONTESTED)).any() and not got["band"].any()


# ---------------------------------------------------------------- 1. the dense kernel
@pytest.mark.parametrize("name", DENSE)
def test_dense_kernel_nominates_exactly_the_reference(gpu, name):
    """``mmx_peaks_batch`` without entries on blocks of every width of the quad tail and the wave ends, 1 to 17 scales,
    poison in every float that is nobody's: the set of candidates, ``v``, ``nbr_max`` and ``flags`` bit for bit,
    ``band == 0`` and no MMX_CAND_BAND, ``*d_count``."""
    r, want = _run(gpu, name), case(name).table()
    print(name, "candidates", r.count, "reference", len(want))
    assert r.count == len(want)
    got = r.nominated[:r.count]
    _assert_rows_equal(got[_order(got)], want, banded=False)
    assert _guard_is_intact(r.nominated, r.cap)


def test_dense_table_overflow_keeps_counting_and_stays_inside(gpu):
    """``cap`` a third of the candidates: ``*d_count`` is the full count, the ``cap`` rows written are distinct members of
    the reference with their fields, the rows behind the table are untouched."""
    name = "dense_ns9"
    want = case(name).table()
    cap = len(want) // 3
    r = _run(gpu, name, cap=cap)
    assert cap >= 50 and r.count == len(want)
    got = r.nominated[:cap]
    got = got[_order(got)]
    assert len(np.unique(cand_key(got), axis=0)) == cap
    pos = {tuple(k): i for i, k in enumerate(cand_key(want))}
    idx = [pos.get(tuple(k), -1) for k in cand_key(got)]
    assert min(idx) >= 0
    _assert_rows_equal(got, want[idx], banded=False)
    assert _guard_is_intact(r.nominated, cap)


def test_a_batch_whose_slots_are_permuted_is_refused(gpu):
    """Block i owns slot i (include/mmx.h: the block in slot b starts at b x slot_elems; ``mmx_batch_geom_make``): a
    batch that numbers its slots otherwise is an argument error, not a silently different layout."""
    from magellanmapper_amd import _native as nat, blob_log as bl
    L, c = nat.lib(), case("dense_ns1")
    nb = len(c.shapes)
    blocks = _blocks(c.shapes, slots=list(range(nb - 1, -1, -1)))
    log = torch.zeros(nb * c.slot_elems, dtype=torch.float32, device=gpu)
    table = torch.zeros(16 * nat.CAND_DTYPE.itemsize, dtype=torch.uint8, device=gpu)
    count = torch.zeros(1, dtype=torch.int32, device=gpu)
    rc = L.mmx_peaks_batch(log.data_ptr(), None, 0, 1, bl._to_device_bytes(blocks, gpu).data_ptr(), blocks.ctypes.data, nb,
                           c.slot_elems, c.thr, c.eps, table.data_ptr(), 16, count.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 1, (rc, L.mmx_strerror(rc).decode())                  # MMX_ERR_ARG
    assert int(count.item()) == 0


# ---------------------------------------------------------------- 2. the sparse kernel
@pytest.mark.parametrize("layout", [ROWS, QUADS], ids=["rows", "quads"])
@pytest.mark.parametrize("name", SPARSE)
def test_sparse_kernel_nominates_exactly_the_reference(gpu, name, layout):
    """``mmx_peaks_batch`` from entries of either layout, the unstored segments of the cube poisoned: candidates, ``v``,
    ``nbr_max``, the contested flag, MMX_CAND_BAND and all 80 band bits equal the reference on the stored cube, and the
    largest and the smallest legal word 0 give the same table.  In the queue case more candidate bits than the LDS queue
    holds sit in one workgroup round, and every voxel of the plateau comes back exactly once."""
    c = case(name)
    want = c.table(layout)
    tables = []
    for word0 in ("same", "faces"):
        r = _run(gpu, name, layout, word0)
        print(name, _LAYOUTS[layout], word0, "candidates", r.count, "reference", len(want))
        assert r.count == len(want)
        got = r.nominated[:r.count]
        got = got[_order(got)]
        _assert_rows_equal(got, want, banded=True)
        assert _guard_is_intact(r.nominated, r.cap)
        tables.append(got)
    for f in ("slot", "s", "z", "y", "x", "flags", "v", "nbr_max", "band"):
        np.testing.assert_array_equal(tables[0][f], tables[1][f])
    if c.queue:
        i, on = c.plateaus[0]
        rows = tables[0][tables[0]["slot"] == i]
        hit = np.zeros(on.shape, dtype=np.int64)
        np.add.at(hit, (rows["s"], rows["z"], rows["y"], rows["x"]), 1)
        assert int(on.sum()) > H.QUEUE and (hit[on] == 1).all()


@pytest.mark.parametrize("layout", [ROWS, QUADS], ids=["rows", "quads"])
def test_sparse_table_overflow_keeps_counting_and_stays_inside(gpu, layout):
    name = "sparse_ns9"
    want = case(name).table(layout)
    cap = len(want) // 3
    r = _run(gpu, name, layout, "faces", cap=cap)
    assert cap >= 50 and r.count == len(want)
    got = r.nominated[:cap]
    got = got[_order(got)]
    assert len(np.unique(cand_key(got), axis=0)) == cap
    pos = {tuple(k): i for i, k in enumerate(cand_key(want))}
    idx = [pos.get(tuple(k), -1) for k in cand_key(got)]
    assert min(idx) >= 0
    _assert_rows_equal(got, want[idx], banded=True)
    assert _guard_is_intact(r.nominated, cap)


# ---------------------------------------------------------------- 3. the probes
@pytest.mark.parametrize("name,layout", RUNS, ids=RUN_IDS)
def test_expand_probes_appends_exactly_the_reference(gpu, name, layout):
    """``mmx_expand_probes`` on the tables of parts 1 and 2 (unbanded and banded): ``*d_n_cands``, the candidate rows
    untouched, the multiset of probe rows -- place, ``flags == MMX_CAND_PROBE``, ``band`` = the index of their
    candidate -- equal to ``probes_ref``, ``*d_count`` = candidates + probes, every probe inside its cube (candidates at
    4-D corners included)."""
    c = case(name)
    r = _run(gpu, name, layout)
    want_c = c.table(layout)
    want_p = H.probes_ref(want_c, c.shapes, c.ns)
    print(name, _LAYOUTS[layout], "candidates", r.n_cands, "probes", r.total - r.n_cands, "reference", len(want_p))
    assert r.n_cands == r.count == len(want_c)
    assert r.total == r.n_cands + len(want_p) and r.total <= r.cap
    np.testing.assert_array_equal(r.expanded[:r.n_cands].view(np.uint8), r.nominated[:r.n_cands].view(np.uint8))
    probes = r.expanded[r.n_cands:r.total]
    assert (probes["flags"] == H.PROBE).all() and (probes["band"] < r.n_cands).all()
    # the index of a candidate in the device's table -> its index in the reference's (sorted) table
    rank = np.empty(r.n_cands, dtype=np.int64)
    rank[_order(r.nominated[:r.n_cands])] = np.arange(r.n_cands)
    got = np.concatenate([cand_key(probes), rank[probes["band"].astype(np.int64)][:, None]], axis=1)
    np.testing.assert_array_equal(H.sort_rows(got), want_p)
    dims = np.asarray(c.shapes)[probes["slot"]]
    for f, hi in (("s", c.ns), ("z", dims[:, 0]), ("y", dims[:, 1]), ("x", dims[:, 2])):
        assert (probes[f] >= 0).all() and (probes[f] < hi).all()
    if layout is None and c.ns >= 3:
        kinds = np.concatenate([H.face_kind(cube.shape)[t["s"], t["z"], t["y"], t["x"]][t["contested"]]
                                for cube, t in zip(c.cubes, c.reference())])
        assert (kinds == 15).any()                                   # (a contested candidate at a 4-D corner)
    assert _guard_is_intact(r.expanded, r.cap)


@pytest.mark.parametrize("name,layout", [("dense_ns9", None), ("sparse_ns9", QUADS)], ids=["dense", "quads"])
def test_expand_probes_overflow_keeps_counting_and_stays_inside(gpu, name, layout):
    """A capacity between the candidates and candidates + probes: the count keeps counting, the candidates stay as they
    were, what was appended are probes of the reference, the rows behind the table are untouched."""
    c = case(name)
    want_c = c.table(layout)
    want_p = H.probes_ref(want_c, c.shapes, c.ns)
    cap = len(want_c) + len(want_p) // 3
    r = _run(gpu, name, layout, cap=cap)
    assert len(want_p) >= 90 and r.n_cands == len(want_c) and r.total == len(want_c) + len(want_p)
    np.testing.assert_array_equal(r.expanded[:r.n_cands].view(np.uint8), r.nominated[:r.n_cands].view(np.uint8))
    probes = r.expanded[r.n_cands:cap]
    assert (probes["flags"] == H.PROBE).all()
    rank = np.empty(r.n_cands, dtype=np.int64)
    rank[_order(r.nominated[:r.n_cands])] = np.arange(r.n_cands)
    got = np.concatenate([cand_key(probes), rank[probes["band"].astype(np.int64)][:, None]], axis=1)
    assert len(np.unique(got, axis=0)) == len(got)
    assert {tuple(g) for g in got} <= {tuple(w) for w in want_p}
    assert _guard_is_intact(r.expanded, cap)


# ---------------------------------------------------------------- 4. the closed loop
@pytest.mark.parametrize("name,layout", RUNS, ids=RUN_IDS)
def test_nominate_expand_resolve_is_peak_local_max_of_the_exact_cube(gpu, name, layout):
    """an exact cube within eps / 4 of the nominated one -- up to 3 x 2^-16 off, in patterns that
    turn every tie either way, and not off at all (every voxel of a plateau is then a peak) -- whose values fill
    ``v64`` of the device's candidate and probe rows in place of ``mmx_rescore_f64``: ``mmx_host_resolve_peaks`` gives
    per block the oracle's ``peak_mask`` of the exact cube, values and order included, and reports the deviation."""
    from magellanmapper_amd import blob_log as bl
    c = case(name)
    r = _run(gpu, name, layout)
    assert r.total <= r.cap
    n_peaks = 0
    for pattern in (0, 1, -1):
        exact = c.exact(pattern)
        table = r.expanded[:r.total].copy()
        for i in range(len(c.shapes)):
            m = table["slot"] == i
            table["v64"][m] = exact[i][table["s"][m], table["z"][m], table["y"][m], table["x"][m]]
        stats = bl.BatchStats()
        pb = bl._resolve_peaks_native(table, r.n_cands, r.blocks, c.ns, c.thr, stats, c.eps)
        assert stats.max_f32_error == (MAX_DELTA if pattern else 0.0)
        for i in range(len(c.shapes)):
            want_rows, want_vals = H.oracle_peaks(exact[i], c.thr)
            rows, vals = pb.block(i)
            np.testing.assert_array_equal(rows, want_rows)
            np.testing.assert_array_equal(vals, want_vals)
            n_peaks += len(rows)
        if pattern == 0:
            for i, on in c.plateaus:
                rows, _ = pb.block(i)
                hit = np.zeros(on.shape, dtype=bool)
                hit[rows[:, 3], rows[:, 0], rows[:, 1], rows[:, 2]] = True
                assert hit[on].all()
    assert n_peaks >= 100


# ---------------------------------------------------------------- 5. the entries of the real producers
class _Producer:
    """The ragged blocks of the host file (and, for the tiled kernels, the 530 voxels wide one) through
    ``mmx_log_batch_f32`` with entries, scale by scale, under one named mode; ``d_log`` prefilled with a sentinel."""
    SENTINEL = -77.0

    def __init__(self, dev, mode, wide_block, eps):
        from magellanmapper_amd import _native as nat, blob_log as bl, kernels1d as k1
        from test_gpu_wide_rows import _tiled_slot
        L = nat.lib()
        spec = H.RAGGED_BLOCKS + ([H.WIDE_BLOCK] if wide_block else [])
        self.shapes = [s for _, s in spec]
        dvol = bl.DeviceVolume(H.producer_volume())
        self.blocks, slot = bl._make_blocks(dvol, 0, [o for o, _ in spec], self.shapes)
        self.slot = slot = _tiled_slot(self.shapes, 1) if wide_block else slot
        nb, ns = len(spec), len(H.PRODUCER_SIGMAS)
        self.nb, self.ns, self.lo, self.eps = nb, ns, np.float32(np.float32(H.PRODUCER_THR) - np.float32(eps)), eps
        d_blocks = bl._to_device_bytes(self.blocks, dev)
        v32 = dvol.view(0, True)
        work = torch.zeros(4 * nb * slot, dtype=torch.float32, device=dev)
        log = torch.full((ns, nb * slot), self.SENTINEL, dtype=torch.float32, device=dev)
        generic = torch.zeros((ns, nb * slot), dtype=torch.float32, device=dev)
        words = (nb * slot) >> 5
        masks = torch.zeros((ns, words, 2), dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        self.paths, self.layouts, self.bounds = [], [], []
        for i, sg in enumerate(H.PRODUCER_SIGMAS):
            R = k1.kernel_radius(sg)
            w0, w2 = k1.gaussian_half_kernel(sg, 0, R), k1.gaussian_half_kernel(sg, 2, R)
            args = (ctypes.byref(v32), d_blocks.data_ptr(), self.blocks.ctypes.data, nb, slot, nat.as_double_ptr(w0),
                    nat.as_double_ptr(w2), R, sg * sg)
            written, path = ctypes.c_int(-1), ctypes.c_int(-1)
            nat.check(L.mmx_log_batch_f32(*args, log[i].data_ptr(), work.data_ptr(), masks[i].data_ptr(), float(self.lo),
                                          eps, ctypes.byref(written), mode, ctypes.byref(path), stream), "mmx_log_batch_f32")
            nat.check(L.mmx_log_batch_f32_generic(*args, generic[i].data_ptr(), work.data_ptr(), stream), "generic")
            self.paths.append(path.value)
            self.layouts.append(written.value)
            self.bounds.append(L.mmx_tiled_q16_error_bound(nat.as_double_ptr(w0), nat.as_double_ptr(w2), R, sg * sg))
        torch.cuda.synchronize()
        self.log, self.generic = log.cpu().numpy().reshape(ns, nb, slot), generic.cpu().numpy().reshape(ns, nb, slot)
        self.masks = masks.cpu().numpy().view(np.uint64)

    def cube(self, arr, i):
        nz, ny, nx = self.shapes[i]
        px = H.pitch(nx)
        return arr[:, i, :nz * ny * px].reshape(self.ns, nz, ny, px)[..., :nx]

    def entries(self, i, layout):
        nz, ny, nx = self.shapes[i]
        nwords = H.entry_map(nz, nx, layout)[2]
        return self.masks[:, (i * self.slot) >> 5:][:, :ny * nwords].reshape(self.ns, ny, nwords, 2)


def _producers():
    from magellanmapper_amd import _native as nat, blob_log as bl
    return {
        "MMX_ZX_PACKED": (nat.MMX_ZX_PACKED, nat.MMX_ZX_PACKED, ROWS, False, bl.EPS_REL, False),
        "MMX_ZX_TILED": (nat.MMX_ZX_TILED, nat.MMX_ZX_TILED, QUADS, True, bl.EPS_REL, False),
        "MMX_ZX_TILED_Q16": (nat.MMX_ZX_TILED_Q16, nat.MMX_ZX_TILED_Q16, QUADS, True, bl.EPS_REL_Q16, True),
        "MMX_ZX_TILED_Q16|MMX_ZX_Y_VALU": (nat.MMX_ZX_TILED_Q16 | nat.MMX_ZX_Y_VALU, nat.MMX_ZX_TILED_Q16, QUADS, True,
                                           bl.EPS_REL_Q16, True),
        "MMX_ZX_WIDE": (nat.MMX_ZX_WIDE, nat.MMX_ZX_WIDE, ROWS, False, bl.EPS_REL, False),
    }


@pytest.mark.parametrize("producer", ["MMX_ZX_PACKED", "MMX_ZX_TILED", "MMX_ZX_TILED_Q16", "MMX_ZX_TILED_Q16|MMX_ZX_Y_VALU",
                                      "MMX_ZX_WIDE"])
def test_entries_of_a_real_producer_keep_the_contract_of_the_header(gpu, producer):
    """Each kernel that writes NMS entries, by name, on ragged blocks (rows below 16 and no multiple of 16, planes no
    multiple of 4, columns no multiple of 16; for the tiled kernels also a block 530 wide and 26 deep), three scales.
    From the device's own output: the path and layout asked for; word 0 within word 1 and no bit past the block; in
    stored segments word 1 is ``d_log > nms_lo`` to the bit; unstored segments still hold the sentinel; word 0 holds
    every candidate of the brute-force reference on the stored cube; nothing the generic passes put above ``nms_lo`` by
    more than the path's stated error is missing from word 1.  A block with fewer than 20 stored or 20 unstored
    segments or 10 candidates fails: the case would be too easy."""
    from magellanmapper_amd import blob_log as bl
    mode, path, layout, wide_block, eps, q16 = _producers()[producer]
    p = _Producer(gpu, mode, wide_block, eps)
    print(producer, "paths", p.paths, "layouts", p.layouts, "q16 bounds", p.bounds)
    assert p.paths == [path] * p.ns and p.layouts == [layout] * p.ns
    # the path's own stated error against the float32 generic passes: the 16-bit tiles' bound x the value range (1 for
    # uint16 voxels), the band the product grants the float32 paths x the value scale (1)
    tol = max(p.bounds) * 1.0 if q16 else bl.EPS_REL * 1.0
    assert 0 < tol <= eps
    sentinel = np.float32(p.SENTINEL)
    for i, (nz, ny, nx) in enumerate(p.shapes):
        ent = p.entries(i, layout)
        w0, w1 = ent[..., 0], ent[..., 1]
        assert not (w0 & ~w1).any()
        bits1 = H.bits_of(w1, nz, nx, layout)
        np.testing.assert_array_equal(H.words_of(bits1, layout), w1)                     # (no bit beyond nx / nz)
        stored = H.stored_of(w1, nz, nx, layout)
        log, generic = p.cube(p.log, i), p.cube(p.generic, i)
        np.testing.assert_array_equal(bits1[stored], log[stored] > p.lo)
        assert (log[~stored] == sentinel).all() and not (log[stored] == sentinel).any()
        ref = H.nominate_ref(log, stored, H.PRODUCER_THR, eps)
        bits0 = H.bits_of(w0, nz, nx, layout)
        assert not (ref["mask"] & ~bits0).any()
        seg = w1 != 0
        print("  block %s: %d stored / %d unstored segments, %d word-0 bits, %d candidates, |producer - generic| %.3g" % (
            (nz, ny, nx), seg.sum(), (~seg).sum(), bits0.sum(), len(ref["v"]), np.abs(log[stored] - generic[stored]).max()))
        assert seg.sum() >= H.PRODUCER_MIN["stored"] and (~seg).sum() >= H.PRODUCER_MIN["unstored"]
        assert len(ref["v"]) >= H.PRODUCER_MIN["candidates"]
        must = generic > p.lo + np.float32(tol)
        assert must.any() and not (must & ~(stored & bits1)).any()
