"""The kernel-path rules on the CPU: ``tools/route_check.cpp`` -- the table of routes, the by-name rows of
``tests/golden/route_by_name.txt`` and the sweep over geometries -- built as a stand-alone program under the host
sanitizers (AddressSanitizer + UBSan linked into that program only) and run.  Needs ``hipcc`` (the routing header comes
with the kernels' shared declarations), no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not found")
def test_route_check_passes_under_the_host_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "route_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                            "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-x", "hip",
                            os.path.join(ROOT, "tools", "route_check.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "route_by_name.txt")], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, text=True)
    print(run.stdout[-3000:])
    assert run.returncode == 0, run.stdout[-3000:]
    assert "0 refused by a predicate, 0 disagreements" in run.stdout
