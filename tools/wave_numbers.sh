#!/bin/bash
# wave-kernel workloads, one line each (general path: one QP per wavefront)
run() { python bench.py --full --no-cpu-baseline "$@" > /dev/null 2>&1; python -c "
import json,sys; d=json.load(open('bench_full.json')); c=d['config']
print(' '.join(sys.argv[1:]), '| %s | %.3e solves/s | mean it %.2f | %.3e it/s' % (c['kernel'], d['value'], c['mean_iterations'], d['value']*c['mean_iterations']))" "$@"; }
run --workload mass_spring_3in --steps 5 --warmup 1 --batch 100000
run --workload soft_doc --steps 10 --warmup 2 --batch 200000
run --workload mass_spring --wave --steps 10 --warmup 2 --batch 200000
run --workload pendulum_hard --wave --steps 10 --warmup 2
run --workload mass_spring_3in --steps 5 --warmup 1 --batch 100000 --f32
run --workload soft_doc --steps 10 --warmup 2 --batch 200000 --f32
run --workload hybrid --steps 3 --warmup 1 --batch 20000
run --workload hybrid --steps 3 --warmup 1 --batch 20000 --f32
