"""The A/B scheme of the measuring tools (``tools/abbench.py``) against a stub worker: the order of the requests, the
summary, a worker that ends mid-run, chatter on a worker's stdout.  No GPU."""
import os
import sys

import pytest

from conftest import ROOT

TOOLS = os.path.join(ROOT, "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import abbench  # noqa: E402

TIMES = [5.0, 3.0, 4.0, 1.0, 2.0, 6.0]

#: answers request n with TIMES[n], after a line of chatter; logs "<cmd> <name>" per request; exits with status 7 instead
#: of answering request number ``die_at``
STUB = """
import sys
sys.path.insert(0, %r)
import abbench
name, log, die_at = sys.argv[1], sys.argv[2], int(sys.argv[3])
times, seen = %r, []

def answer(req):
    if len(seen) == die_at:
        sys.exit(7)
    seen.append(req)
    with open(log, "a") as f:
        f.write("%%s %%s\\n" %% (req["cmd"], name))
    print("chatter of a library, no JSON")
    return dict(ms=times[len(seen) - 1], case=req["case"])

abbench.serve(dict(describe=answer, run=answer))
""" % (TOOLS, TIMES)


@pytest.fixture
def stub(tmp_path):
    script = tmp_path / "stub_worker.py"
    script.write_text(STUB)
    log = tmp_path / "requests.log"
    made = []

    def start(name, die_at=-1):
        made.append(abbench.Worker(str(script), [name, str(log), str(die_at)]))
        return made[-1]
    yield start, log
    for w in made:
        w.close()


def test_requests_alternate_in_the_order_of_the_names(stub):
    start, log = stub
    builds = {"parent": start("parent"), "new": start("new")}
    seen = []
    described, times = abbench.alternate(builds, ["parent", "new"], "c", warmup=2, repeats=3,
                                         check=lambda b, reply, first: seen.append((b, reply["ms"], first["ms"])))
    pair = ["parent", "new"]
    assert log.read_text().split("\n")[:-1] == (["describe %s" % b for b in pair] + ["run %s" % b for b in pair] * (2 + 3))
    # every build answered describe with its first time, the warm-ups with the next two, the repeats with the rest
    assert described == {b: dict(ms=TIMES[0], case="c") for b in pair}
    assert times == {b: TIMES[3:6] for b in pair}
    assert seen == [(b, t, TIMES[0]) for t in TIMES[3:6] for b in pair]


def test_a_subset_of_the_builds_runs_alone(stub):
    start, log = stub
    builds = {"parent": start("parent"), "new": start("new")}
    described, times = abbench.alternate(builds, ["new"], "c", warmup=0, repeats=2)
    assert log.read_text().split() == ["describe", "new", "run", "new", "run", "new"]
    assert list(described) == ["new"] and times == {"new": TIMES[1:3]}


def test_summary_of_an_odd_and_an_even_count():
    odd = abbench.summarise([5.0, 1.0, 4.0])
    assert odd == dict(median_ms=4.0, min_ms=1.0, max_ms=5.0, spread_ms=4.0, repeats=3)
    even = abbench.summarise([5.0, 1.0, 4.0, 2.0])
    assert even == dict(median_ms=3.0, min_ms=1.0, max_ms=5.0, spread_ms=4.0, repeats=4)
    per_voxel = abbench.summarise([2.0, 4.0, 3.0], voxels=1000)
    assert (per_voxel["ns_per_voxel"], per_voxel["ns_per_voxel_max"]) == (3000.0, 4000.0)
    assert set(per_voxel) == set(odd) | {"ns_per_voxel", "ns_per_voxel_max"}


def test_a_worker_that_ends_mid_run_raises_and_the_other_closes(stub):
    start, _ = stub
    builds = {"parent": start("parent"), "new": start("new", die_at=2)}
    with pytest.raises(RuntimeError, match="exit status 7"):
        abbench.alternate(builds, ["parent", "new"], "c", warmup=1, repeats=2)
    builds["parent"].close()
    assert builds["parent"].p.returncode == 0
    builds["new"].close()                       # (closing the dead one is harmless too)


def test_lines_that_are_no_json_are_skipped(stub):
    start, _ = stub
    w = start("only")
    assert w.ask(cmd="run", case="x") == dict(ms=TIMES[0], case="x")
    assert w.ask(cmd="describe", case="y") == dict(ms=TIMES[1], case="y")
