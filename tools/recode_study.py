"""What the digit recodings buy and what they cost (run on the GPU, bench.py is not touched).

For b-bit square matrices (default_rng(seed).integers(-2^(b-1), 2^(b-1))), both as ONE wmc chain (`method0 = method1 = 'wmc'`,
`decompose_dc=-1`, `search_all_decompose_dc=False`) and under the default search of solve(), one line per (bits, size, matrix seed, mode) with
  * the adders of solve;
  * the adders of the COMPACT digits;
  * the best and the median of 16 SEEDED points;
  * the best of 16 tie-seeded restarts in the newest order, from the CSD digits and with recode='compact' (restart 0 is solve under both);
  * the wall time of each of the five calls (the first call of a size also pays for arena growth).
Sizes go up in the outermost loop; `--budget` seconds after the start no new configuration is begun and those left are listed as not reached.

    python tools/recode_study.py [--bits 3 4 6 8] [--sizes 16 32 64 128 256] [--seeds 0 1 2] [--modes wmc search] [--points 16] [--budget 600] [--out FILE]"""

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import restart_seeds, solve_restarts  # noqa: E402

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
MODES = {'wmc': SINGLE, 'search': {}}
HEADER = f'{"bits":>4} {"size":>5} {"seed":>4} {"mode":>6} | {"solve":>7} {"compact":>7} {"seeded best":>11} {"median":>8} {"newest16":>8} {"+compact":>8} | {"seconds: solve":>14} {"compact":>7} {"seeded16":>8} {"newest16":>8} {"+compact":>8}'


def timed(fn):
    t0 = time.perf_counter()
    res = fn()
    return res, time.perf_counter() - t0


def study(bits, n, mseed, mode, points):
    k = np.random.default_rng(mseed).integers(-(1 << (bits - 1)), 1 << (bits - 1), (n, n)).astype(np.float32)
    opts = MODES[mode]
    (plain,), t_plain = timed(lambda: hip.solve_each([k], [dict(opts)]))
    (compact,), t_compact = timed(lambda: hip.solve_each([k], [dict(opts, recode='compact')]))
    seeds = restart_seeds(points + 1, 1)[1:]
    seeded, t_seeded = timed(lambda: hip.solve_each([k] * points, [dict(opts, recode='seeded', recode_seed=s) for s in seeds]))
    (_, newest, _), t_newest = timed(lambda: solve_restarts(k, points, seed=1, return_all=True, order='newest', **opts))
    (_, both, _), t_both = timed(lambda: solve_restarts(k, points, seed=1, return_all=True, order='newest', recode='compact', **opts))
    for p in (plain, compact, seeded[0], newest[-1], both[-1]):
        assert np.array_equal(p.kernel, k)
    sa = [p.n_adders for p in seeded]
    return (f'{bits:>4} {n:>5} {mseed:>4} {mode:>6} | {plain.n_adders:>7} {compact.n_adders:>7} {min(sa):>11} {statistics.median(sa):>8.1f} {min(p.n_adders for p in newest):>8} '
            f'{min(p.n_adders for p in both):>8} | {t_plain:>14.3f} {t_compact:>7.3f} {t_seeded:>8.3f} {t_newest:>8.3f} {t_both:>8.3f}')  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bits', type=int, nargs='+', default=[3, 4, 6, 8])
    ap.add_argument('--sizes', type=int, nargs='+', default=[16, 32, 64, 128, 256])
    ap.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    ap.add_argument('--modes', nargs='+', default=['wmc', 'search'], choices=sorted(MODES))
    ap.add_argument('--points', type=int, default=16)
    ap.add_argument('--budget', type=float, default=600.0, help='seconds after which no new configuration is begun')
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
        for mode in args.modes:
            for bits in args.bits:
                for mseed in args.seeds:
                    if time.perf_counter() - t0 > args.budget:
                        skipped.append((bits, n, mseed, mode))
                        continue
                    emit(study(bits, n, mseed, mode, args.points))
    for bits, n, mseed, mode in skipped:
        emit(f'{bits:>4} {n:>5} {mseed:>4} {mode:>6} | not reached within the budget of {args.budget:.0f} s')


if __name__ == '__main__':
    main()
