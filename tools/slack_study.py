"""What a score slack buys and what it costs (run on the GPU, bench.py is not touched).

For b-bit square matrices (default_rng(seed).integers(-2^(b-1), 2^(b-1))) as ONE wmc chain (`method0 = method1 = 'wmc'`, `decompose_dc=-1`,
`search_all_decompose_dc=False`), one line per (bits, size, matrix seed, tie order, slack) with
  * the adders of solve (restart 0 of every call);
  * best and median of the restarts r >= 1 of solve_restarts(kernel, R, seed=1, order=, slack=), and how many of them are cheaper than solve;
  * the wall time of the call (the first call of a size also pays for arena growth).
Slack 0 is the yardstick: the tie-order restarts of the same order, seeds and count.  Sizes go up in the outermost loop; `--budget` seconds
after the start no new configuration is begun and those left are listed as not reached.

`--timing N`: after the study, a call of R restarts of the seed-0 N x N 8-bit matrix with `--timing-slack` against the same call without it,
two warm-ups and seven rounds with the variants alternating; median [min, max] seconds of each.

    python tools/slack_study.py [--bits 8 4] [--sizes 64 128 256] [--seeds 0 1 2] [--slacks 0 2 4 8 16 32] [--orders random newest] [--restarts 64]
                                [--budget 600] [--timing 256] [--timing-slack 4] [--out FILE]"""

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from da4ml_amd.cmvm import solve_restarts  # noqa: E402

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
HEADER = f'{"bits":>4} {"size":>5} {"seed":>4} {"order":>6} {"slack":>5} | {"solve":>7} {"best":>7} {"best %":>7} {"median":>8} {"cheaper":>7} of {"R-1":>3} | {"seconds":>7}'


def matrix(bits, n, mseed):
    return np.random.default_rng(mseed).integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, n)).astype(np.float32)


def study(bits, n, mseed, order, slack, restarts):
    k = matrix(bits, n, mseed)
    t0 = time.perf_counter()
    _, pipes, _ = solve_restarts(k, restarts, seed=1, return_all=True, order=order, slack=slack, **SINGLE)
    dt = time.perf_counter() - t0
    assert np.array_equal(pipes[0].kernel, k) and np.array_equal(pipes[-1].kernel, k)
    plain, rest = pipes[0].n_adders, [p.n_adders for p in pipes[1:]]
    return (f'{bits:>4} {n:>5} {mseed:>4} {order:>6} {slack:>5} | {plain:>7} {min(rest):>7} {100.0 * (min(rest) - plain) / plain:>+7.2f} {statistics.median(rest):>8.1f} '
            f'{sum(a < plain for a in rest):>7} of {len(rest):>3} | {dt:>7.3f}')  # fmt: skip


def timing(n, slack, restarts, emit):
    k = matrix(8, n, 0)
    times = {0: [], slack: []}
    for rnd in range(9):  # two warm-ups, seven rounds
        for s in ((0, slack) if rnd % 2 == 0 else (slack, 0)):
            t0 = time.perf_counter()
            solve_restarts(k, restarts, seed=1, order='newest', slack=s, **SINGLE)
            if rnd >= 2:
                times[s].append(time.perf_counter() - t0)
    emit(f'timing: {restarts} newest-order restarts of the seed-0 {n}x{n} 8-bit matrix, one call, seconds, median [min, max] of 7 alternating rounds after 2 warm-ups')
    for s, v in times.items():
        emit(f'  slack {s:>3}: {statistics.median(v):.3f} [{min(v):.3f}, {max(v):.3f}]')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bits', type=int, nargs='+', default=[8, 4])
    ap.add_argument('--sizes', type=int, nargs='+', default=[64, 128, 256])
    ap.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    ap.add_argument('--slacks', type=int, nargs='+', default=[0, 2, 4, 8, 16, 32])
    ap.add_argument('--orders', nargs='+', default=['random', 'newest'], choices=['random', 'newest'])
    ap.add_argument('--restarts', type=int, default=64)
    ap.add_argument('--budget', type=float, default=600.0, help='seconds after which no new configuration is begun')
    ap.add_argument('--timing', type=int, default=0, help='size of the timed matrix (0: no timing)')
    ap.add_argument('--timing-slack', type=int, default=4)
    ap.add_argument('--out', help='append the lines to this file as well')
    args = ap.parse_args()

    def emit(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    t0 = time.perf_counter()
    emit(HEADER)
    skipped = []
    for n in args.sizes:
        for bits in args.bits:
            for mseed in args.seeds:
                for order in args.orders:
                    for slack in args.slacks:
                        if time.perf_counter() - t0 > args.budget:
                            skipped.append((bits, n, mseed, order, slack))
                            continue
                        emit(study(bits, n, mseed, order, slack, args.restarts))
    for bits, n, mseed, order, slack in skipped:
        emit(f'{bits:>4} {n:>5} {mseed:>4} {order:>6} {slack:>5} | not reached within the budget of {args.budget:.0f} s')
    if args.timing:
        timing(args.timing, args.timing_slack, args.restarts, emit)


if __name__ == '__main__':
    main()
