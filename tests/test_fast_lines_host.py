"""The staged write-out's kernels (fast_staged_kernel, fast_staged_kernel_multi of lmpc_fast_kernel.hpp) in the built
library, from its AMDGPU metadata notes (kernel names and register counts; no code is read): they exist for exactly
the (NTHMAX, NT, N) triples of tests/fast_cases.py, and the headline pair keeps four wavefronts per SIMD."""
import re

import fast_cases as fc
from test_fast_fallback import LIB, _kernel_vgprs


def test_staged_kernels_cover_the_case_table():
    names = _kernel_vgprs(LIB, r"fast_staged_kernel(_multi)?ILi\d+E")
    got = {False: set(), True: set()}
    for k in names:
        m = re.search(r"fast_staged_kernel(_multi)?ILi(\d+)ELi(\d+)ELi(\d+)EE", k)
        assert m, k
        got[m.group(1) is not None].add(tuple(int(v) for v in m.groups()[1:]))
    assert got[False] == fc.instantiations() and got[True] == fc.instantiations()


def test_staged_headline_kernels_fit_four_waves_per_simd():
    vg = _kernel_vgprs(LIB, r"fast_staged_kernel(_multi)?ILi8ELi7ELi5EE")
    assert len(vg) == 2, sorted(vg)
    assert all(v <= 128 for v in vg.values()), vg
