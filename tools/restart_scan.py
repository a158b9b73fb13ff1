"""What seeded random restarts buy and what they cost (run on the GPU, bench.py is not touched).

For a square int8 matrix (default_rng(seed).integers(-128, 128), the benchmark's recipe) as ONE greedy chain (`decompose_dc=-1`,
`search_all_decompose_dc=False`):
  * R restarts of the matrix in one call (da4ml_amd.cmvm.solve_restarts): wall time of the call, distribution of adders and cost
    over the restarts (min, median, max) against restart 0, which is the deterministic solve;
  * beside it the same call with R unseeded chains of R DISTINCT matrices -- the benchmark's own C3 workload at 256x256 --: the
    difference is what the seeded instantiation costs per lockstep step.
Each call is made twice and the second is reported (the first pays for arena growth).  One JSON line per size, tie order and mode.
`--orders`: the seeded tie orders to scan ('random', 'newest'); `--modes`: 'wmc' (the single wmc chain above), 'wmc-dc' (a single wmc-dc chain)
or 'search' (the default search of solve(): every decompose_dc candidate of every restart); `--no-distinct` leaves the unseeded comparison call out.

    python tools/restart_scan.py [--sizes 256 64 128] [--restarts 64] [--seed 1] [--orders random] [--modes wmc] [--no-distinct] [--out FILE]"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import restart_seeds  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
MODES = {'wmc': SINGLE, 'wmc-dc': dict(SINGLE, method0='wmc-dc', method1='wmc-dc'), 'search': {}}


def matrix(seed, n):
    return np.random.default_rng(seed).integers(-128, 128, (n, n)).astype(np.float32)


def timed(fn):
    fn()
    hip.timings(reset=True)
    t0 = time.perf_counter()
    res = fn()
    dt = time.perf_counter() - t0
    tm = hip.timings(reset=True)
    return res, dt, tm


def dist(v):
    return dict(min=min(v), median=statistics.median(v), max=max(v))


def scan(n, restarts, seed, order='random', mode='wmc', with_distinct=True):
    k = matrix(0, n)
    seeds = restart_seeds(restarts, seed)
    opts = MODES[mode]
    pipes, t_restarts, tm_r = timed(lambda: hip.solve_many([k] * restarts, seeds=seeds, tie_order=order, **opts))
    distinct = [matrix(i, n) for i in range(restarts)]
    if with_distinct:
        plain, t_plain, tm_p = timed(lambda: hip.solve_many(distinct, **opts))
    else:
        t_plain, tm_p = None, dict(loop_ms=None, lockstep_iters=0)
    adders = [p.n_adders for p in pipes]
    costs = [pipeline_cost_f32(p) for p in pipes]
    best = min(range(restarts), key=lambda i: (costs[i], i))
    per_step = lambda tm: 1e3 * tm['loop_ms'] / max(tm['lockstep_iters'], 1) if tm['loop_ms'] is not None else None  # noqa: E731
    return dict(
        size=n, restarts=restarts, seed=seed, order=order, mode=mode, valid=all(bool(np.all(p.kernel == k)) for p in pipes[:: max(1, restarts // 4)]),
        restarts_call_s=t_restarts, restarts_loop_ms=tm_r['loop_ms'], restarts_us_per_lockstep_step=per_step(tm_r), restarts_lockstep_steps=tm_r['lockstep_iters'],
        distinct_unseeded_call_s=t_plain, distinct_unseeded_loop_ms=tm_p['loop_ms'], distinct_unseeded_us_per_lockstep_step=per_step(tm_p), distinct_unseeded_lockstep_steps=tm_p['lockstep_iters'],
        deterministic=dict(adders=adders[0], cost=costs[0]), best=dict(restart=best, adders=adders[best], cost=costs[best]),
        adders=dist(adders), cost=dist(costs), distinct_results=len(set(costs)), restarts_cheaper_than_deterministic=sum(c < costs[0] for c in costs),
    )  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 64, 128])
    ap.add_argument('--restarts', type=int, default=64)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', help='append the JSON lines to this file as well')
    ap.add_argument('--orders', nargs='+', default=['random'], choices=sorted(hip.TIE_ORDERS))
    ap.add_argument('--modes', nargs='+', default=['wmc'], choices=sorted(MODES))
    ap.add_argument('--no-distinct', action='store_true', help='skip the call with unseeded chains of distinct matrices')
    args = ap.parse_args()
    for n in args.sizes:
        for mode in args.modes:
            for order in args.orders:
                line = json.dumps(scan(n, args.restarts, args.seed, order, mode, not args.no_distinct))
                print(line, flush=True)
                if args.out:
                    with open(args.out, 'a') as f:
                        f.write(line + '\n')


if __name__ == '__main__':
    main()
