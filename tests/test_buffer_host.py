"""The handle's owning buffer type, the group rule, the scratch reset and the launch-record ring
(linearmpc.jl_amd/csrc/lmpc_buffer.hpp), checked on the host: tests/buffer_check.cpp is a stand-alone program with a
malloc-backed allocator that counts live blocks and can fail the k-th allocation.  It is built with the address and
undefined-behaviour sanitizers (LeakSanitizer reports at exit) and links neither HIP nor the library."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buffer_group_scratch_and_ring_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = tmp_path / "buffer_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "buffer_check.cpp"), "-o", str(exe)],
                   check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "buffer_check ok" in out.stdout
