"""The one-launch kernel's generic fallback (lane_loop, called out of line from fast_kernel) and the register budget
that moving it out of line buys the kernel: four wavefronts per SIMD."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import load_golden, oracle_ldp_from

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
LIB = os.path.join(ROOT, "linearmpc.jl_amd", "lib", "liblmpc_hip.so")
LLVM_BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def _tool(name):
    path = os.path.join(LLVM_BIN, name)
    return path if os.path.exists(path) else shutil.which(name)


def _gfx950_code_objects(lib, tmp):
    """The gfx950 code objects of `lib`: its .hip_fatbin section is one clang offload bundle per translation unit
    ("__CLANG_OFFLOAD_BUNDLE__", entry count, then (offset, size, triple length, triple) per entry)."""
    objcopy = _tool("llvm-objcopy")
    if objcopy is None:
        pytest.skip("llvm-objcopy not found")
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([objcopy, "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "stripped")], check=True,
                   capture_output=True)
    with open(fat, "rb") as fh:
        data = fh.read()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    out = []
    start = data.find(magic)
    while start >= 0:
        pos = start + len(magic)
        (nent,) = struct.unpack_from("<Q", data, pos)
        pos += 8
        for _ in range(nent):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            pos += 24
            triple = data[pos:pos + tlen].decode()
            pos += tlen
            if triple.endswith("gfx950") and size > 0:
                co = os.path.join(tmp, f"co{len(out)}.o")
                with open(co, "wb") as fh:
                    fh.write(data[start + off:start + off + size])
                out.append(co)
        start = data.find(magic, pos)
    return out


def _kernel_vgprs(lib, symbol_re):
    """{kernel symbol: .vgpr_count} from the AMDGPU metadata notes of the gfx950 code objects embedded in `lib`."""
    readelf = _tool("llvm-readelf")
    if readelf is None:
        pytest.skip("llvm-readelf not found")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in _gfx950_code_objects(lib, tmp):
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            if not re.search(symbol_re, notes):
                continue
            # the metadata lists one map per kernel; .name and .vgpr_count are keys of the same map
            for block in re.split(r"\n\s*- \.", notes):
                name = re.search(r"\.?name:\s+(\S+)", block)
                vg = re.search(r"\.?vgpr_count:\s+(\d+)", block)
                if name and vg and re.search(symbol_re, name.group(1)):
                    out[name.group(1)] = int(vg.group(1))
    return out


def test_fast_kernel_headline_instantiation_fits_four_waves_per_simd():
    # fast_kernel<8, 7, 5, false> (the pendulum batch) and its several-batches form: at most 128 VGPRs -- 512 / 128 =
    # four wavefronts per SIMD, i.e. four workgroups of four wavefronts per CU
    assert os.path.exists(LIB), "build the library first"
    vg = _kernel_vgprs(LIB, r"fast_kernel(_multi)?ILi8ELi7ELi5E(Lb0E)?E")
    assert any("fast_kernelILi8ELi7ELi5ELb0E" in k for k in vg), sorted(vg)
    assert any("fast_kernel_multiILi8ELi7ELi5E" in k for k in vg), sorted(vg)
    for k, v in vg.items():
        assert v <= 128, (k, v)


def _hard_theta(n, seed):
    # the pendulum example's +-20 parameter range: most points iterate, and rows leave the working set again -- the
    # lanes the straight-line tiers cannot finish
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.hstack([rng.uniform(-20, 20, (n, 4)), rng.uniform(-20, 20, (n, 1)), np.zeros((n, 1)),
                                           rng.uniform(-2, 2, (n, 1))]))


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [3, 1])
def test_fast_fallback_many_lanes_match_oracle(in_flight):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import linearmpc_jl_amd as lmpc
    from oracle import ldp as oldp
    g = load_golden("pendulum")
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
    qp.set_option("in_flight", in_flight)
    assert qp.kernel_name.startswith("fast<5>")
    L = oracle_ldp_from(qp.ldp())
    for N in (64 * 4096 + 17, 1_000_000):
        theta = _hard_theta(N, 20 + N % 7)
        x, ef, it, act = qp.solve(theta)
        sel = np.arange(N) if N < 300_000 else np.random.default_rng(3).choice(N, 250_000, replace=False)
        xo, efo, ito, acto = oldp.solve_batch(L, theta[sel])
        assert np.array_equal(x[sel], xo) and np.array_equal(ef[sel], efo)
        assert np.array_equal(it[sel], ito) and np.array_equal(act[sel], acto)
        # lanes that removed a row again (more iterations than adds) were solved by the generic loop: a few dozen
        # of the ~250 000 checked here
        nact = np.array([bin(int(a)).count("1") for a in act[sel].view(np.uint64).ravel()])
        assert (it[sel] > nact + 1).sum() >= 10
        # the device-resident call writes the same bits
        th_d = torch.from_numpy(theta).cuda()
        xd, efd = qp.solve_device(th_d)
        torch.cuda.synchronize()
        assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(efd.cpu().numpy(), ef)
    qp.check()
