"""The BASELINE.json configurations at (or near) their real geometry, through the C ABI, against the oracle.

  * two blocks of the benchmark geometry (261 wide, 5 sigmas, kernel radii 12..20, the seed-3 generator):
    per-block tables and the pruned table
  * C2 (configs[1]): 512 x 512 x 256, single sigma, through ``bench.py --config c2``
  * C5-shaped (configs[4]): a 2-channel volume, preprocessing on, intensity co-localisation, the blocks
    sharded over 2 and 3 ranks that share the GPU (gloo), through ``bench.py --config c5``
"""
import json
import multiprocessing as mp
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from gpu_support import gpu  # noqa: F401

pytestmark = pytest.mark.gpu
RES = np.array([[1.0, 1.0, 1.0]])


def _host_volume(shape, seed, channels=1):
    """bench.py's generator on the host (the benchmark's blob field: density, amplitude, background)."""
    import torch
    from magellanmapper_amd import synth
    c0 = synth.make_volume_device(shape, seed, torch.device("cpu")).to(torch.int32)
    if channels == 1:
        return c0.numpy().astype(np.uint16)
    c1 = synth.make_volume_device(shape, seed + 1, torch.device("cpu")).to(torch.int32)
    c1 = torch.maximum(c1, (c0 * 7) // 10)
    return torch.stack((c0, c1), dim=-1).numpy().astype(np.uint16)


def _bench_profile(**over):
    sys.path.insert(0, ROOT)
    import bench
    return dict(bench._BASE_PROFILE, **over)


def _oracle_block(args):
    coord, offset, last, sub, profile = args
    sys.path.insert(0, ROOT)
    from oracle import magmap_oracle as mmo
    return coord, mmo.detect_sub_roi(coord, offset, last, None, sub, None, [profile], RES)


def test_two_blocks_of_the_benchmark_geometry(gpu):
    """Blocks as the 2048^2 x 1024 volume cuts them: 261 voxels wide (256 + the 5 overlap columns, the tail
    producer wave of the fused kernel), 5 sigmas 3..5 (radii 12, 14, 16, 18, 20), uint16 from the seed-3 generator;
    only the depth is cut to 101 planes so that the float64 oracle takes seconds per block."""
    from magellanmapper_amd import blob_log as bl, config, stack_detect
    from oracle import magmap_oracle as mmo
    shape = (101, 261, 517)
    vol = _host_volume(shape, 3)
    profile = _bench_profile()
    config.setup_roi_profiles(None)
    config.resolutions, config.filename = RES, "cfgtest"
    config.roi_profile.update(profile)
    blk = stack_detect.setup_blocks(config.roi_profile, (101, 261, 512))       # tol / overlap as the benchmark's
    slices = np.empty((1, 1, 2), dtype=object)
    slices[0, 0, 0] = (slice(0, 101), slice(0, 261), slice(0, 261))
    slices[0, 0, 1] = (slice(0, 101), slice(0, 261), slice(256, 517))
    offsets = np.zeros((1, 1, 2, 3), dtype=int)
    offsets[0, 0, 1] = (0, 0, 256)
    seg = stack_detect.StackDetector.detect_blobs_sub_rois(None, bl.DeviceVolume(vol), slices, offsets, None, None,
                                                           False, [0])
    assert bl.LAST_ZX_PATH == 7                       # the tiled matrix-core kernels, 16-bit intermediates, took this geometry
    st = stack_detect.StackDetector.last_stats
    assert st.n_blocks == 2 and st.max_f32_error < 0.25 * bl.EPS_REL_Q16
    got, _ = stack_detect.StackPruner.prune_blobs_mp(vol, seg, blk.overlap, blk.tol, slices, offsets, [0],
                                                     blk.overlap_padding)
    last = np.array([0, 0, 1])
    jobs = [(c, offsets[c], last, vol[slices[c]], profile) for c in ((0, 0, 0), (0, 0, 1))]
    want_seg = np.zeros((1, 1, 2), dtype=object)
    with mp.get_context("spawn").Pool(2) as pool:
        for c, tbl in pool.imap_unordered(_oracle_block, jobs):
            want_seg[c] = tbl
    for c in ((0, 0, 0), (0, 0, 1)):
        assert want_seg[c] is not None and len(want_seg[c]) > 200
        np.testing.assert_array_equal(seg[c], want_seg[c])          # per-block tables, row for row
    want, _ = mmo.prune_blobs_mp(shape, want_seg, blk.overlap, blk.tol, slices, offsets, [0], blk.overlap_padding)
    assert len(want) < len(want_seg[0, 0, 0]) + len(want_seg[0, 0, 1])      # the seam had duplicates
    np.testing.assert_array_equal(got, want)


def _run_bench(tmp_path, ranks, *extra, timeout=900, launcher=True):
    """``launcher=False``: plain ``python bench.py --gpus N`` -- the script starts its ranks itself."""
    env = dict(os.environ, MMX_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [os.path.join(ROOT, "bench.py"), "--gpus", str(ranks), "--steps", "1", "--warmup", "0",
           "--no-cpu-baseline", *extra]
    if ranks > 1 and launcher:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks),
               "--master-addr", "127.0.0.1", "--master-port", str(port)] + cmd
    run = subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=timeout, env=env,
                         cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-3000:]
    return json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])


def test_c2_single_sigma_volume_matches_oracle(gpu, tmp_path):
    """BASELINE.json configs[1] at full size: 512 x 512 x 256 uint16, one sigma (3), segment_size 256 -> 4 blocks of
    256 x 261 x 261; the final table of ``bench.py --config c2`` equals the oracle's, and the run reports its roofline."""
    from oracle import magmap_oracle as mmo
    shape = (256, 512, 512)
    vol = _host_volume(shape, 2)
    np.save(tmp_path / "c2.npy", vol)
    line = _run_bench(tmp_path, 1, "--config", "c2", "--volume", str(tmp_path / "c2.npy"), "--dump",
                      str(tmp_path / "c2.npz"), "--full")
    assert line["config"]["blocks_per_rank"] == 4 and line["roofline"]["kernel"] in ("zxpass", "y2pass")
    profile = _bench_profile(min_sigma_factor=3, max_sigma_factor=3, num_sigma=1)
    want, _ = mmo.detect_blobs_blocks(vol, None, [profile], RES)
    got = np.load(tmp_path / "c2.npz")["final"]
    assert len(want) > 3000
    np.testing.assert_array_equal(got, want)


def test_kernel_event_modes_of_the_bench_line(gpu, tmp_path):
    """``bench.py --kernel-events all | dominant | none``: where the per-kernel HIP events are recorded (inside the timed
    region, only the roofline's family there, or in extra steps after it) changes neither the table nor what the line
    reports -- every family has its launches and a time."""
    shape = (96, 200, 210)
    vol = _host_volume(shape, 5)
    np.save(tmp_path / "ke.npy", vol)
    lines = {}
    for mode in ("all", "dominant", "none"):
        lines[mode] = _run_bench(tmp_path, 1, "--config", "c3", "--segment-size", "64", "--volume", str(tmp_path / "ke.npy"),
                                 "--steps", "2", "--warmup", "1", "--kernel-events", mode, "--full")
    ref = lines["all"]
    assert ref["config"]["blocks_per_rank"] > 8 and ref["graph_replay"] is None        # (not the small-volume graph path)
    assert ref["kernel_events"]["in_timed_region"] == "all" and lines["none"]["kernel_events"]["in_timed_region"] == "none"
    timed = lines["dominant"]["kernel_events"]["in_timed_region"]
    from magellanmapper_amd import _native
    # (the warm-up step's longest family -- on these small blocks not necessarily one the later steps launch)
    assert isinstance(timed, list) and len(timed) == 1 and timed[0] in _native.KERNEL_KINDS
    for mode, line in lines.items():
        assert line["table_sha1"] == ref["table_sha1"] and line["blobs"] == ref["blobs"] > 0, mode
        assert line["roofline"]["kernel"] in ref["kernels"], mode          # (tiny kernels here: which one leads is noise)
        assert set(line["kernels"]) == set(ref["kernels"]), mode
        for fam, rec in line["kernels"].items():
            assert rec["launches_per_step"] == ref["kernels"][fam]["launches_per_step"] and rec["ms_per_step"] > 0, (mode, fam)


def test_plain_line_dumps_the_last_steps_outputs(gpu, tmp_path):
    """A plain ``bench.py`` run (no ``--full``) times exactly ``--steps`` steps, measures nothing beside them (no CPU
    baseline, parity sample, sub-records or link rates) and with ``--dump-outputs`` writes the last step's table and
    flags: the ``--dump`` table, and the same files from a second run of the same command."""
    common = ("--config", "c5", "--shape", "56", "150", "160", "--segment-size", "64", "--steps", "3", "--warmup", "1")
    lines = []
    for k in range(2):
        lines.append(_run_bench(tmp_path, 1, *common, "--dump", str(tmp_path / f"c5_{k}.npz"),
                                "--dump-outputs", str(tmp_path / f"out{k}")))
    line = lines[0]
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["step_ms_percentiles"]["max"] > 0
    assert line["cpu_baseline"] is None and line["parity_sample_identical"] is None and "sub_records" not in line
    assert line["h2d"] is None
    dump = np.load(tmp_path / "c5_0.npz")
    final, colocs = np.load(tmp_path / "out0" / "final.npy"), np.load(tmp_path / "out0" / "colocs.npy")
    assert final.dtype == np.float64 and colocs.dtype == np.float32 and len(final) == line["blobs"] > 50
    np.testing.assert_array_equal(final, dump["final"])
    np.testing.assert_array_equal(colocs, dump["colocs"].astype(np.float32))
    assert sorted(os.listdir(tmp_path / "out1")) == ["colocs.npy", "final.npy"]
    for name in ("final.npy", "colocs.npy"):
        np.testing.assert_array_equal(np.load(tmp_path / "out1" / name), np.load(tmp_path / "out0" / name))
    # a volume of one block replays its batch from a captured graph: no kernel events in the timed region, and a plain
    # line takes no extra steps to time the kernels
    small = _run_bench(tmp_path, 1, "--config", "c2", "--shape", "64", "128", "128", "--steps", "3", "--warmup", "3",
                       "--dump-outputs", str(tmp_path / "c2"))
    assert small["steps"] == 3 and small["kernel_events"]["in_timed_region"] == "none" and small["kernels"] == {}
    assert small["roofline"] is None and small["pipeline_roofline"]["frac_kernels"] is None
    assert len(np.load(tmp_path / "c2" / "final.npy")) == small["blobs"]


@pytest.mark.parametrize("ranks", [2, 3])
def test_c5_shaped_two_channel_coloc_over_ranks(gpu, tmp_path, ranks):
    """BASELINE.json configs[4] in small: 2 channels (30 % of channel 1's blobs of its own), per-block preprocessing
    (denoise_size 25), both channels detected, intensity co-localisation, blocks sharded over ranks that share this
    GPU (gloo), gathered and pruned on rank 0: final table and ``colocs`` equal the oracle's."""
    from oracle import magmap_oracle as mmo
    shape = (56, 150, 160)
    vol = _host_volume(shape, 3, channels=2)
    np.save(tmp_path / "c5.npy", vol)
    line = _run_bench(tmp_path, ranks, "--config", "c5", "--segment-size", "64", "--volume", str(tmp_path / "c5.npy"),
                      "--dump", str(tmp_path / "c5.npz"), launcher=ranks != 3)     # (3 ranks: bench.py launches them itself)
    assert line["n_gpus"] == ranks and len(line["ranks"]) == ranks
    assert sum(r["blocks"] for r in line["ranks"]) == 9                 # 1 x 3 x 3 blocks, uneven over 2 ranks
    profile = _bench_profile(denoise_size=25, segment_size=64)
    want, stages = mmo.detect_blobs_blocks(vol, [0, 1], [profile, profile], RES, near_max=[-1.0, -1.0], coloc=True)
    dump = np.load(tmp_path / "c5.npz")
    assert len(want) > 100 and set(np.unique(want[:, 6])) == {0.0, 1.0}
    np.testing.assert_array_equal(dump["final"], want)
    np.testing.assert_array_equal(dump["colocs"], stages["colocs"])


GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
C3_DIGEST = "5fba8ef88362dfa0a7d9fb8caaef869ea416eb85"


def test_full_c3_volume_over_two_ranks_has_the_one_rank_digest(gpu, tmp_path):
    """BASELINE.json configs[3] as far as one GPU goes: the FULL 2048 x 2048 x 1024 volume, its 256 blocks sharded
    over 2 ranks that share this GPU (gloo), every rank pruning its own rows and merging everybody's survivors by key
    (the distributed pruning): same digest and blob count as one rank.  Rank 0 also runs the parity sample by itself
    (``dist.solo``) against the committed oracle table of that sample (tests/golden/make_bench_samples.py).

    Two ranks, not four: THREE or more processes on one MI355X of this pool are time-sliced in quanta of seconds --
    four processes take 262 s to generate their slabs of the synthetic volume instead of 0.6 s with two
    (tools/exp/gen4.py: all four finish at the same moment), the three-rank form of this test 275 s, the four-rank form
    515 s -- a property of the box, not of this code.  The four-rank run returns the same digest
    (profiles/r04_ranks4_gloo.txt) and stays a tool: ``MMX_DIST_BACKEND=gloo python bench.py --gpus 4``."""
    line = _run_bench(tmp_path, 2, "--parity-sample", os.path.join(GOLDEN_DIR, "bench_sample_c3.npz"), timeout=1500)
    assert line["n_gpus"] == 2 and [r["blocks"] for r in line["ranks"]] == [128, 128]
    assert line["table_sha1"] == C3_DIGEST and line["blobs"] == 292044
    assert line["parity_sample_identical"] is True and "committed" in line["parity_sample_source"]
    assert line["scaling"] == "strong" and line["roofline"] is not None


def test_full_size_c5_tile_digests_and_sample_parity(gpu, tmp_path):
    """BASELINE.json configs[4] at bench.py's geometry on one GPU: 2 channels x 2048 x 2048 x 512 uint16, per-block
    preprocessing (denoise_size 25), both channels detected with 5 sigmas, intensity co-localisation, prune.  Too large
    for the float64 oracle, so: the sample of the same workload equals the committed oracle table (final table row for
    row AND the co-localisation flags), and the full-size table / flags are pinned by digest and by size-independent
    properties."""
    line = _run_bench(tmp_path, 1, "--config", "c5", "--parity-sample", os.path.join(GOLDEN_DIR, "bench_sample_c5.npz"),
                      "--dump", str(tmp_path / "c5.npz"), timeout=1500)
    assert line["parity_sample_identical"] is True and "committed" in line["parity_sample_source"]
    assert line["config"]["blocks_per_rank"] == 128 and line["n_gpus"] == 1
    dump = np.load(tmp_path / "c5.npz")
    final, colocs = dump["final"], dump["colocs"]
    assert final.shape == (line["blobs"], 8) and colocs.shape == (line["blobs"], 2) and colocs.dtype == np.uint8
    assert set(np.unique(final[:, 6])) == {0.0, 1.0}
    zyx = final[:, :3]
    assert np.array_equal(zyx, np.round(zyx)) and zyx.min() >= 0 and np.all(zyx.max(axis=0) < (512, 2048, 2048))
    # the reference's off-by-one: column 0 of the flags is uint8(region = -1), column 1 the
    # flag of channel 0 -- set for every blob of channel 0 that passes its own channel's threshold
    assert np.all(colocs[:, 0] == 255) and set(np.unique(colocs[:, 1])) <= {0, 1}
    assert line["table_sha1"] == C5_DIGESTS["table"], line["table_sha1"]
    assert line["colocs_sha1"] == C5_DIGESTS["colocs"], line["colocs_sha1"]
    assert line["blobs"] == C5_DIGESTS["blobs"]


#: first recorded in round 4 (profiles/r04_bench_c5_first.json); the sample check above ties the same code to the oracle
C5_DIGESTS = {"table": "4cea549b4ccf64e812dd75171aaf9505125a5a67", "colocs": "946996fd9817e988835dfcafc0d68fb79af3f543",
              "blobs": 427167}


def test_full_size_c3_volume_properties_and_digest(gpu, tmp_path):
    """BASELINE.json configs[2] at FULL size (2048 x 2048 x 1024, 256 blocks, 5 sigmas) through ``bench.py``: too
    large for the float64 oracle, so the result is pinned by what does not depend on size -- the digest of the final
    table (the same for every kernel path, batch size and rank count since it was first recorded, and equal to the
    oracle on the sample ``bench.py --full`` checks at every run), and properties of a correctly pruned table."""
    from magellanmapper_amd import detector
    line = _run_bench(tmp_path, 1, "--dump", str(tmp_path / "c3.npz"), timeout=1200)
    assert line["config"]["blocks_per_rank"] == 256 and line["n_gpus"] == 1
    assert line["table_sha1"] == C3_DIGEST
    assert line["detector_stats"]["max_f32_error"] < 4.4e-5 and line["detector_stats"]["n_band_retries"] == 0   # Q16 bound
    final = np.load(tmp_path / "c3.npz")["final"]
    assert final.shape == (line["blobs"], 8) and line["blobs"] == 292044
    zyx = final[:, :3]
    assert np.array_equal(zyx, np.round(zyx)) and zyx.min() >= 0
    assert np.all(zyx.max(axis=0) < (1024, 2048, 2048))
    assert set(np.unique(final[:, 3]).round(6)) <= {round(s * 3 ** 0.5, 6) for s in (3.0, 3.5, 4.0, 4.5, 5.0)}
    assert np.all(final[:, 4:6] == -1) and np.all(final[:, 6] == 0) and np.all(final[:, 7] == -1)
    # idempotence: no two surviving blobs within the pruning tolerance of each other across a block seam, i.e.
    # checking the table against itself finds every row only as its own match (remove_close_blobs, tol 5)
    order = np.lexsort((zyx[:, 2], zyx[:, 1], zyx[:, 0]))
    s = zyx[order].astype(np.int64)
    near_seam = np.zeros(len(s), dtype=bool)
    for ax, n in enumerate((1024, 2048, 2048)):
        pos = s[:, ax] % 256
        near_seam |= ((pos <= 10) | (pos >= 246)) & (s[:, ax] > 10) & (s[:, ax] < n - 10)
    cand = s[near_seam]
    pruned, _ = detector.remove_close_blobs(np.hstack((cand, np.zeros((len(cand), 8)))),
                                            np.hstack((cand + [[4096, 0, 0]], np.zeros((len(cand), 8)))), 5)
    assert len(pruned) == len(cand)          # (shifted far away along z: nothing may match)
    cz = cand[np.lexsort((cand[:, 2], cand[:, 1], cand[:, 0]))]
    d = np.abs(np.diff(cz, axis=0))
    assert not np.any(np.all(d == 0, axis=1))           # no exact duplicates left at the seams


def test_tiled_stack_sharded_by_tile_is_a_weak_scaling_line(gpu, tmp_path):
    """``bench.py --config c5 --tiles T --gpus N`` (configs[4] across GPUs, as far as one GPU goes): four small two-channel
    tiles -- as 4 tiles on one rank and as 2 per rank on two gloo ranks sharing this GPU -- give the same table and flags
    per tile (tile g is the same volume whoever detects it), distinct tiles differ, the line says ``weak`` and carries
    per-rank tile times, and the parity sample (rank 0, by itself) equals the oracle run in that process."""
    args = ("--config", "c5", "--shape", "56", "150", "160", "--segment-size", "64", "--cpu-cores", "4")
    env = dict(os.environ, MMX_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", *args, "--tiles", "4",
                          "--full"],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr[-3000:]
    one = json.loads([l for l in run.stdout.splitlines() if l.startswith("{")][-1])
    assert one["parity_sample_identical"] is True and one["cpu_baseline"]["kind"] == "port"
    two = _run_bench(tmp_path, 2, *args, "--tiles", "2", "--steps", "2", "--warmup", "1")
    for line, n in ((one, 1), (two, 2)):
        assert line["scaling"] == "weak" and line["n_gpus"] == n and line["config"]["tiles_total"] == 4
        assert line["config"]["tiles_per_rank"] == 4 // n and [t["tile"] for t in line["tiles"]] == [0, 1, 2, 3]
        assert line["roofline"]["kernel"] in line["kernels"] and line["roofline"]["frac"] > 0
        assert all(t["blobs"] > 50 and t["colocs_sha1"] for t in line["tiles"])
    assert one["tiles"] == two["tiles"]
    assert len({t["table_sha1"] for t in one["tiles"]}) == 4
    assert [r["tiles"] for r in two["ranks"]] == [2.0, 2.0] and all(r["ms_per_tile"] > 0 for r in two["ranks"])
    assert one["value"] > 0 and two["value"] > 0 and two["ms_per_tile"] > 0


def test_share_run_models_a_rank_and_merges_the_whole_stacks_table(gpu, tmp_path):
    """``bench.py --share k/N`` (the strong-scaling MODEL measured on one GPU): one process plays every rank of N twice to
    record what a real run puts on the wire (``dist.Loopback``), then replays rank k -- its share of the blocks, its seam
    rows, the pruning of its rows, the merge of every rank's survivors.  The merged table is the whole stack's: the same
    digest as the plain one-process run, for a middle and an edge rank of 3 and of 8."""
    shape = (96, 192, 240)             # (whole blocks of 48: a regular geometry -- the distributed pruning's domain)
    np.save(tmp_path / "sh.npy", _host_volume(shape, 5))
    common = ("--config", "c3", "--segment-size", "48", "--volume", str(tmp_path / "sh.npy"), "--steps", "2", "--warmup", "1")
    plain = _run_bench(tmp_path, 1, *common)
    assert plain["share"] is None and plain["blobs"] > 100
    for spec in ("1/3", "0/8", "5/8"):
        line = _run_bench(tmp_path, 1, *common, "--share", spec)
        k, n = (int(v) for v in spec.split("/"))
        sh = line["share"]
        assert sh["rank"] == k and sh["of"] == n and sh["blocks"] > 0 and sum(sh["batches"]) == sh["blocks"]
        assert line["table_sha1"] == plain["table_sha1"] and line["blobs"] == plain["blobs"], spec
        assert line["n_gpus"] == 1 and sh["step_ms"] > 0 and sh["prune_and_merge_ms"] > 0
        assert line["config"]["blocks_per_rank"] == sh["blocks"] < plain["config"]["blocks_per_rank"]
