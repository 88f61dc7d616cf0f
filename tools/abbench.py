"""The A/B scheme of the measuring tools, stated once: two worker processes alive for the whole run, one JSON request
per line, ``describe`` then warm-up then ``parent, new, parent, new, ...``, a summary, a digest, JSON out.

A tool's driver starts a :class:`Worker` per build and hands them to :func:`alternate`; its worker side answers through
:func:`serve`.  A worker may run out of another checkout against that checkout's package, so this module imports
nothing of the package (NumPy only inside the digests)."""
import hashlib
import json
import subprocess
import sys


class Worker:
    """``script`` started with ``args`` as a child that answers one JSON line per request line."""

    def __init__(self, script, args=(), env=None, cwd=None):
        self.p = subprocess.Popen([sys.executable, script, *args], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                  env=env, cwd=cwd)

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


def serve(handlers):
    """The worker's loop: a request ``{"cmd": name, ...}`` per line of stdin, answered by ``handlers[name](req)`` as one
    JSON line; ``quit`` (or the end of stdin) ends it."""
    for line in sys.stdin:
        req = json.loads(line)
        if req["cmd"] == "quit":
            break
        sys.stdout.write(json.dumps(handlers[req["cmd"]](req)) + "\n")
        sys.stdout.flush()


def alternate(builds, names, case, warmup, repeats, check=None):
    """One case on the builds ``names`` of ``builds`` (name -> Worker), strictly in that order within every round:
    ``describe`` (also the first warm-up), ``warmup`` rounds of ``run``, ``repeats`` measured rounds.
    ``check(name, reply, described)`` sees every measured reply.  Returns the ``describe`` records and the ``ms`` lists."""
    described = {b: builds[b].ask(cmd="describe", case=case) for b in names}
    for _ in range(warmup):
        for b in names:
            builds[b].ask(cmd="run", case=case)
    times = {b: [] for b in names}
    for _ in range(repeats):
        for b in names:
            reply = builds[b].ask(cmd="run", case=case)
            times[b].append(reply["ms"])
            if check is not None:
                check(b, reply, described[b])
    return described, times


def same_fields(*keys):
    """A ``check`` for :func:`alternate`: every measured reply repeats these fields of the build's ``describe``."""
    def check(build, reply, described):
        for k in keys:
            assert reply[k] == described[k], (build, k, reply[k], described[k])
    return check


def summarise(ms, voxels=None):
    s = sorted(ms)
    n = len(s)
    med = s[n // 2] if n % 2 else 0.5 * (s[n // 2 - 1] + s[n // 2])
    out = dict(median_ms=med, min_ms=s[0], max_ms=s[-1], spread_ms=s[-1] - s[0], repeats=n)
    if voxels is not None:
        out.update(ns_per_voxel=med * 1e6 / voxels, ns_per_voxel_max=s[-1] * 1e6 / voxels)
    return out


def peaks_digest(peaks):
    """``(n, sha1)`` of per-block ``(coords, values)`` as ``blob_log_blocks(return_peaks=True)`` gives them."""
    import numpy as np
    h, n = hashlib.sha1(), 0
    for coords, vals in peaks:
        h.update(np.ascontiguousarray(coords).tobytes())
        h.update(np.ascontiguousarray(vals).tobytes())
        n += len(coords)
    return n, h.hexdigest()


def table_digest(tables):
    """``(rows, sha1)`` of a list of blob tables, as float64 and in the order given."""
    import numpy as np
    h, n = hashlib.sha1(), 0
    for t in tables:
        t = np.ascontiguousarray(t, dtype=np.float64)
        h.update(t.tobytes())
        n += len(t)
    return n, h.hexdigest()


def write_json(path, result):
    if path:
        with open(path, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
