"""Chains of DAIS programs for the compiled executables (da4ml_amd._binary.dais_compile, C ABI da_dais_compile), shared by
tests/test_dais_exec.py (host modes), tests/emu/dais_exec_worker.py (kernel k_dais_exec on the emulated device) and
tests/test_zz_dais_exec_gpu.py (the same kernel on the GPU).  The programs come from tests/dais_cases.py unchanged; the reference
of every chain is the stage-by-stage composition on the host block executor, `compose`."""

import numpy as np
from dais_cases import random_program


def compose(programs, x):
    """for p in programs: x = dais_interp_run(p, x) -- what an executable must reproduce bit for bit"""
    from da4ml_amd._binary import dais_interp_run

    for p in programs:
        x = dais_interp_run(p, x, n_threads=1)
    return x


def random_chain(seed, n_stages=2, n_ops=None, n_samples=24):
    """`n_stages` random programs whose sizes fit; samples inside the declared input formats (first half) and far outside (second
    half: every input statement wraps)"""
    rng = np.random.default_rng(10_000 + seed)
    widths = [int(v) for v in rng.integers(2, 8, n_stages + 1)]
    progs, x = [], None
    for s in range(n_stages):
        n = int(n_ops if n_ops is not None else rng.integers(30, 181))
        n = max(n, widths[s] + 1)
        p, xs = random_program(100 * seed + s, n_in=widths[s], n_ops=n, n_out=widths[s + 1], n_samples=n_samples)
        progs.append(p)
        x = xs if s == 0 else x
    far = x * rng.choice([64.0, 1024.0, -4096.0, 1e6], (1, widths[0])) + rng.integers(-5, 6, x.shape)
    return progs, np.concatenate([x[: (n_samples + 1) // 2], far[(n_samples + 1) // 2 :]])


def with_absent_output(prog, j):
    """a copy of `prog` whose output j is absent (index -1)"""
    p = prog.copy()
    p[6 + int(p[2]) + j] = -1
    return p


def faulting_stage(n_in):
    """A valid program of `n_in` inputs and one output whose lookup statement is out of bounds for EVERY sample: the table's operand is a
    constant add in a 15-bit format (index = value + 1000 + 2**14), the table has four entries"""
    ops = [[-1, j, -1, 0, 0, 1, 4, 0] for j in range(n_in)] + [[4, 0, -1, 1000, 0, 1, 14, 0], [8, n_in, -1, 0, 0, 1, 9, 0]]
    head = [1, 0, n_in, 1, len(ops), 1] + [0] * n_in + [len(ops) - 1] + [0] + [0]
    return np.asarray(head + [w for op in ops for w in op] + [4] + [7, 8, 9, 10], dtype=np.int32)


def pipeline_programs(pipe):
    return [s.to_binary() for s in pipe.solutions]


def samples_for(comb, rng, n, spread=1):
    """integer multiples of every input's step over `spread` times its declared interval"""
    cols = []
    for q in comb.inp_qint:
        lo, hi = round(q.min / q.step), round(q.max / q.step)
        mid, half = (lo + hi) // 2, (hi - lo) // 2  # (spread 1: mid - half >= lo and mid + half <= hi)
        if spread > 1:
            half = spread * max(half, 1)
        cols.append(rng.integers(mid - half, mid + half + 1, n) * q.step)
    return np.stack(cols, axis=1).astype(np.float64)
