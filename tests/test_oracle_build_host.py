"""oracle.ldp.build() with several processes arriving at once (no GPU).  The workers of tests/test_distributed_cpu.py are
the first users of the oracle in a test run; where the library is older than its sources they all rebuild it, and one that
loaded the file while another was still writing it ended with "file too short".  Here: a copy of oracle/ in a scratch
directory, its sources made newer than the library, eight processes loading it at the same time, twice."""
import os
import shutil
import subprocess
import sys

from conftest import ROOT


def test_concurrent_first_use_of_a_stale_oracle(tmp_path):
    shutil.copytree(os.path.join(ROOT, "oracle"), tmp_path / "oracle", ignore=shutil.ignore_patterns("_build", "_ref", "__pycache__"))
    code = "import sys; sys.path.insert(0, %r); from oracle import ldp; ldp.lib(); print(ldp.default_settings().iter_limit)" % str(tmp_path)
    for rnd in range(2):                                     # (no library yet; then one older than a source)
        os.utime(tmp_path / "oracle" / "daqp_avi_oracle.c")
        ps = [subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
              for _ in range(8)]
        outs = [p.communicate(timeout=120) for p in ps]
        assert [o.strip() for o, e in outs] == ["10000"] * 8, (rnd, [e[-300:] for o, e in outs if o.strip() != "10000"])
    left = sorted(os.listdir(tmp_path / "oracle" / "_build"))
    assert [f for f in left if not f.startswith(".")] == ["liboracle.so"], left
