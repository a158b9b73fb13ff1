"""What a sweep of the latency-penalty weight buys and what it costs (run on the GPU, bench.py is not touched).

For a square int8 matrix (default_rng(0).integers(-128, 128), the benchmark's recipe) with `decompose_dc=-1, search_all_decompose_dc=False`:
da4ml_amd.cmvm.solve_tradeoff with its default weights and methods -- 19 solves in one call --: adders, cost and latency of every point, the
Pareto front, the wall time of the call (the second of two calls: the first pays for arena growth).  `--search N`: the default search of the
N x N matrix (point 0 = solve(kernel) with all its candidates) as a line of its own.  One JSON line per size.

    python tools/dc_weight_scan.py [--sizes 64 128 256] [--search 256] [--out FILE]"""

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import solve_tradeoff  # noqa: E402

ONE_CHAIN = dict(decompose_dc=-1, search_all_decompose_dc=False)


def matrix(seed, n):
    return np.random.default_rng(seed).integers(-128, 128, (n, n)).astype(np.float32)


def scan(n, opts, label):
    k = matrix(0, n)
    solve_tradeoff(k, **opts)
    hip.timings(reset=True)
    t0 = time.perf_counter()
    front, pts = solve_tradeoff(k, return_all=True, **opts)
    dt = time.perf_counter() - t0
    tm = hip.timings(reset=True)
    row = lambda p: dict(method=p.method0, dc_weight=p.dc_weight, adders=p.pipeline.n_adders, cost=p.cost, latency=p.latency)  # noqa: E731
    return dict(size=n, options=label, call_s=dt, loop_ms=tm['loop_ms'], chains=tm['chains'], lockstep_steps=tm['lockstep_iters'],
                valid=all(bool(np.all(p.pipeline.kernel == k)) for p in front), points=[row(p) for p in pts], front=[row(p) for p in front])  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='*', default=[64, 128, 256])
    ap.add_argument('--search', type=int, nargs='*', default=[])
    ap.add_argument('--out', help='append the JSON lines to this file as well')
    args = ap.parse_args()
    for n, opts, label in [(n, ONE_CHAIN, 'decompose_dc=-1, search_all_decompose_dc=False') for n in args.sizes] + [(n, {}, 'default search') for n in args.search]:
        line = json.dumps(scan(n, opts, label))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
