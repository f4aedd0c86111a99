#!/usr/bin/env python3
"""Host time per call of the plain entry points on the three handle kinds (the measures of
profiles/dispatch_refactor.md): lmpc_solve_one latency, and lmpc_solve_batch_device at N = 1 and N = 512 as enqueue
rate (2000 calls without draining the queue) and as call + synchronise (300 calls).  Lane handle: pendulum; wavefront
handle with the screening pass in front: pendulum_N50; tiers-pass handle: mass_spring.  One JSON line, microseconds."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import linearmpc_jl_amd as lmpc
from linearmpc_jl_amd._cabi import lib

vp = ctypes.c_void_p
out = {}
for name in ("pendulum", "pendulum_N50", "mass_spring"):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")))
    qp = lmpc.BatchedQP.from_mpqp(g["H"], g["f"], g["f_theta"], g["A"], g["bu"], g["bl"], g["W"], g["senses"], nout=1)
    out[name + " kernel"] = qp.kernel_name
    th1 = np.ascontiguousarray(g["theta"][0])
    x1 = np.zeros(1)
    for _ in range(50):
        lib().lmpc_solve_one(qp._h, vp(th1.ctypes.data), vp(x1.ctypes.data))
    t0 = time.perf_counter()
    for _ in range(300):
        lib().lmpc_solve_one(qp._h, vp(th1.ctypes.data), vp(x1.ctypes.data))
    out[name + " solve_one us"] = round(1e6 * (time.perf_counter() - t0) / 300, 2)
    dev = torch.device("cuda", 0)
    st = vp(torch.cuda.current_stream(dev).cuda_stream)
    for N in (1, 512):
        th = torch.from_numpy(np.ascontiguousarray(g["theta"][:N])).to(dev)
        assert th.shape[0] == N
        x = torch.empty((N, 1), dtype=torch.float64, device=dev)
        ef = torch.empty(N, dtype=torch.int32, device=dev)
        call = lambda: lib().lmpc_solve_batch_device(qp._h, N, vp(th.data_ptr()), vp(x.data_ptr()), vp(ef.data_ptr()), None, None,
                                                     None, st)
        for _ in range(50):
            assert call() == 1
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(2000):
            call()
        t1 = time.perf_counter()
        torch.cuda.synchronize(dev)
        out[f"{name} N={N} enqueue us"] = round(1e6 * (t1 - t0) / 2000, 2)
        t0 = time.perf_counter()
        for _ in range(300):
            call()
            torch.cuda.synchronize(dev)
        out[f"{name} N={N} call+sync us"] = round(1e6 * (time.perf_counter() - t0) / 300, 2)
    qp.check()
    qp.close()
print(json.dumps(out))
