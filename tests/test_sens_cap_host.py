"""The register form of the derivative kernels at the capacities the lane kernels are built with (CAP 5 and 8), which
the host twins (CAP 64) never run: tests/sens_cap_check.cpp is a stand-alone program that walks every row set of a small
pack (n = 6, m = 9, nth = 3, nout = 2, one SOFT row, one duplicated row) and compares sens_point and pack_grad_point
across the capacities, statuses and bits.  It is built with the kernels' floating-point flags and the address and
undefined-behaviour sanitizers and links neither HIP nor the library."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sens_point_and_pack_grad_point_equal_across_capacities(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = tmp_path / "sens_cap_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-mfma", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "sens_cap_check.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sens_cap_check ok" in out.stdout
    # the comparison is not vacuous: every set that fits was compared, and sets of every size a lane kernel finishes
    # at CAP 5 reached SENS_DONE
    cmp5, cmp8 = map(int, re.search(r"compared at CAP 5: (\d+) sets, at CAP 8: (\d+) sets", out.stdout).groups())
    assert cmp5 == sum(c for c in (1, 9, 36, 84, 126, 126)) and cmp8 == 2 ** 9 - 1
    done = [int(v) for v in re.search(r"done by size:((?: \d+)+)", out.stdout).group(1).split()]
    assert len(done) == 10 and all(done[k] >= 1 for k in range(6)), done
