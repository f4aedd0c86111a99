#!/usr/bin/env python3
"""Launch-shape sweep of the one-launch kernel for one library build (LMPC_HIP_LIB selects it; cold HBM): three 1e6
batches in flight (us/step, medians of three runs of 900 steps) and one call at a time (HIP-event call time, medians
of three runs of 200 calls).  A shape is "default" or a comma list of lmpc_set_option NAME=VALUE.

usage: LMPC_HIP_LIB=path/to/lib.so python tools/fast_shapes.py "default;fast_nstr=3,fast_tiles=28,fast_dma=0" "default;fast_tiles=16"
"""
import os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
import torch
import linearmpc_jl_amd as lmpc

tag = os.path.basename(os.environ.get("LMPC_HIP_LIB", "in-tree"))
shapes3 = [s for s in sys.argv[1].split(";") if s] if len(sys.argv) > 1 else []
shapes1 = [s for s in sys.argv[2].split(";") if s] if len(sys.argv) > 2 else []
dev = torch.device("cuda", 0)
W3 = bench.Workload(torch, lmpc, "pendulum", bench.BATCH, dev, 0, 0, 3, options={"lane_block": 64, "in_flight": 3})
W1 = bench.Workload(torch, lmpc, "pendulum", bench.BATCH, dev, 0, 0, 1, options={})


def setopts(W, s):
    kv = dict(x.split("=") for x in s.split(",")) if s != "default" else {}
    for q in W.qps:
        if s == "default":
            q.set_option("in_flight", 3 if W is W3 else 1)
            q.set_option("fast_dma", -1)
        for k, v in kv.items():
            q.set_option(k, int(v))


for s in shapes3:
    setopts(W3, s)
    W3.timed(300, 10, False)
    r = [1e6 * W3.timed(900, 10, False) / 900 for _ in range(3)]
    print(f"{tag:16s} 3inflight {s:32s} us/step med {statistics.median(r):6.2f} runs {' '.join('%.2f' % x for x in r)}", flush=True)
for s in shapes1:
    setopts(W1, s)
    W1.timed(300, 10, False)
    r = [1e3 * W1.single_launch(200, False)[1] for _ in range(3)]
    print(f"{tag:16s} single    {s:32s} us/call med {statistics.median(r):6.2f} runs {' '.join('%.2f' % x for x in r)}", flush=True)
