"""Seeded inputs shared by the CPU and GPU parity tests (no unseeded randomness, unlike the reference's tests)."""

import numpy as np


def int_matrix(seed, n_in, n_out, lo, hi):
    return np.random.default_rng(seed).integers(lo, hi, (n_in, n_out)).astype(np.float32)


def array_digest(*arrays):
    """sha256 over the shapes and float64 values of arrays: equal for arrays that np.array_equal calls equal (-0.0 counts as 0.0)"""
    import hashlib

    h = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a, np.float64) + 0.0
        h.update(repr(a.shape).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def reference_style_kernel(seed, n, bits):
    """The generator of the reference's tests/test_cmvm.py:17-20, seeded."""
    r = np.random.default_rng(seed)
    return np.round((r.random((n, n)) - 0.5) * 2 ** (bits + 1)).astype(np.float32)


METHODS = ('mc', 'mc-dc', 'mc-pdc', 'wmc', 'wmc-dc', 'wmc-pdc')


def random_case(seed):
    """A random small matrix with a random option set, covering every method / cost-model / search combination."""
    rng = np.random.default_rng(seed)
    n_in, n_out = (int(v) for v in rng.integers(1, 13, 2))
    b = int(rng.integers(1, 10))
    k = (rng.random((n_in, n_out)).astype(np.float32) * 2**b - 2 ** (b - 1)).round()
    if seed % 5 == 0:
        k *= 2.0 ** int(rng.integers(-3, 3))
    if seed % 7 == 0:
        k[rng.integers(0, n_in)] = 0
    if seed % 11 == 0:
        k[:, rng.integers(0, n_out)] = 0
    k = np.ascontiguousarray(k, dtype=np.float32)
    opts = dict(
        method0=str(rng.choice(['mc', 'wmc', 'mc-dc', 'wmc-dc', 'mc-pdc', 'wmc-pdc'])),
        method1=str(rng.choice(['auto', 'mc', 'wmc', 'wmc-dc', 'mc-pdc'])),
        hard_dc=int(rng.choice([-1, 0, 1, 2, 3])),
        decompose_dc=int(rng.choice([-2, -1, 0, 1, 2])),
        adder_size=int(rng.choice([-1, 1, 4])),
        carry_size=int(rng.choice([-1, 2, 8])),
        search_all_decompose_dc=bool(rng.integers(0, 2)),
    )
    zero_input = False
    if seed % 3 == 0:
        lo = rng.integers(-64, 1, n_in)
        hi = lo + rng.integers(0, 200, n_in)
        st = 2.0 ** rng.integers(-3, 2, n_in)
        opts['qintervals'] = [(float(a * s), float(c * s), float(s)) for a, c, s in zip(lo, hi, st)]
        opts['latencies'] = [float(v) for v in rng.integers(0, 4, n_in)]
        if seed % 6 == 0:
            opts['qintervals'][0] = (0.0, 0.0, 1.0)
            zero_input = True
    return k, opts, zero_input


def odd_step_case(seed):
    """Input intervals whose quantisation steps are NOT powers of two (what the tracer's `variable * 3` produces, reference
    trace/fixed_variable.py:594): steps m * 2^k with up to five different mantissas per matrix, every cost model that looks at
    the steps, every method.  The latency model then needs -log2f(step) of the host libm for them (StepLog2, cmvm_core.h)."""
    rng = np.random.default_rng(50_000 + seed)
    n_in, n_out = (int(v) for v in rng.integers(2, 11, 2))
    k = rng.integers(-64, 64, (n_in, n_out)).astype(np.float32)
    mants = rng.choice(np.array([1.0, 3.0, 5.0, 0.3, 1.7, 6.25, 0.1], np.float32), size=int(rng.integers(1, 6)), replace=False)
    st = (rng.choice(mants, n_in) * 2.0 ** rng.integers(-4, 3, n_in)).astype(np.float32)
    lo = rng.integers(-40, 1, n_in)
    hi = lo + rng.integers(1, 120, n_in)
    opts = dict(
        method0=str(rng.choice(METHODS)),
        method1=str(rng.choice(['auto', 'wmc', 'mc-dc', 'wmc-pdc'])),
        hard_dc=int(rng.choice([-1, 0, 2])),
        decompose_dc=int(rng.choice([-2, -1, 0, 1])),
        adder_size=int(rng.choice([1, 4, -1])),
        carry_size=int(rng.choice([2, 8, -1])),
        search_all_decompose_dc=bool(rng.integers(0, 2)),
        qintervals=[(float(np.float32(a) * s), float(np.float32(c) * s), float(s)) for a, c, s in zip(lo, hi, st)],
        latencies=[float(v) for v in rng.integers(0, 3, n_in)],
    )
    if opts['adder_size'] < 0 and opts['carry_size'] < 0:
        opts['carry_size'] = 8  # at least one of the two, or the steps are never looked at
    return k, opts


TEST_CMVM_GRID = [
    dict(hard_dc=h, method0=m0, method1=m1, decompose_dc=d, search_all_decompose_dc=s, adder_size=1, carry_size=-1)
    for h in (0, 2, -1)
    for m0 in ('mc', 'wmc')
    for m1 in ('mc', 'wmc')
    for d in (0, -1, -2)
    for s in (False, True)
]


COST_MODELS = ((-1, -1), (1, -1), (4, 8))


def _method_grid():
    """(name, int_matrix arguments, options): every selector x hard_dc x cost model at 32x32 and 64x64 int8 with the default
    decomposition choice (search off: the `decompose_dc--` retry runs), and every selector as ONE 64x64 chain."""
    grid = []
    for n, seed in ((32, 5), (64, 6)):
        for m in METHODS:
            for h in (-1, 0, 2):
                for a, c in COST_MODELS:
                    opts = dict(method0=m, method1='auto', hard_dc=h, decompose_dc=-2, adder_size=a, carry_size=c, search_all_decompose_dc=False)
                    grid.append((f'{n}x{n} {m} hard_dc={h} adder={a} carry={c}', (seed, n, n, -128, 128), opts))
    for m in METHODS:
        for a, c in COST_MODELS:
            opts = dict(method0=m, method1=m, hard_dc=-1, decompose_dc=-1, adder_size=a, carry_size=c, search_all_decompose_dc=False)
            grid.append((f'64x64 single chain {m} adder={a} carry={c}', (7, 64, 64, -128, 128), opts))
    return grid


METHOD_GRID = _method_grid()


# ---- structured matrices: what quantised layer weights look like (ties across the whole pair table, duplicate rows / columns, sparsity) ----
# name -> (medium shape: the GPU size, small twin: the emulated device's size)
_STRUCTURED_SHAPES = {
    'ones': ((64, 64), (12, 12)),
    'ones_wide': ((8, 300), (4, 260)),  # more than 256 columns: wide layout, every column substituted in every step
    'full85': ((48, 48), (12, 12)),
    'full85_signs': ((48, 48), (12, 12)),
    'full_m128': ((24, 20), (12, 10)),
    'full_127': ((24, 20), (12, 10)),
    'full_0x555': ((12, 12), (6, 6)),
    'full_8191': ((12, 12), (6, 6)),
    'frac85': ((24, 24), (12, 12)),
    'diag': ((48, 48), (12, 12)),
    'rank1': ((64, 64), (12, 12)),
    'dup_rows': ((64, 48), (12, 12)),
    'dup_cols': ((48, 64), (12, 12)),
    'neg_cols': ((48, 48), (12, 12)),
    'ternary_sparse': ((128, 128), (16, 16)),
    'ternary_dense': ((64, 64), (12, 12)),
    'pow2': ((64, 64), (12, 12)),
    'toeplitz': ((64, 64), (12, 12)),
    'checker_zero': ((32, 32), (12, 12)),
    'one_hot_rows': ((40, 16), (12, 8)),
}
STRUCTURED = tuple(_STRUCTURED_SHAPES)

SINGLE_CHAIN = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
# the option sets every structured family is recorded under (tests/golden/structured_golden.json.gz)
STRUCTURED_OPTS = {
    'single': SINGLE_CHAIN,
    'default': {},
    'mc_latency': dict(method0='mc', method1='mc-pdc', adder_size=1, carry_size=-1),
    'wmc_dc_hard0': dict(method0='wmc-dc', method1='auto', hard_dc=0, adder_size=4, carry_size=8),
    'mc_dc_hard2': dict(method0='mc-dc', method1='wmc-pdc', decompose_dc=0, hard_dc=2, search_all_decompose_dc=False),
}


def structured_matrix(name, small=False, shape=None):
    """One matrix of a structured family: seeded, float32, C-contiguous.  `small`: the twin for the emulated device;
    `shape`: any other size of the same construction (the seed depends on the family only)."""
    n_in, n_out = shape or _STRUCTURED_SHAPES[name][1 if small else 0]
    rng = np.random.default_rng(70_000 + STRUCTURED.index(name))
    i, j = np.indices((n_in, n_out))
    if name in ('ones', 'ones_wide'):
        k = np.ones((n_in, n_out))
    elif name == 'full85':  # 0b1010101: chained occurrences of one row pair at shifts 2, 4 and 6 that share digits
        k = np.full((n_in, n_out), 85.0)
    elif name == 'full85_signs':
        k = 85.0 * (1 - 2 * ((i + j) % 2))
    elif name == 'full_m128':
        k = np.full((n_in, n_out), -128.0)
    elif name == 'full_127':
        k = np.full((n_in, n_out), 127.0)
    elif name == 'full_0x555':  # 11 overlapping digits, narrow layout
        k = np.full((n_in, n_out), float(0x555))
    elif name == 'full_8191':  # digit 13: wide layout
        k = np.full((n_in, n_out), 8191.0)
    elif name == 'frac85':
        k = np.full((n_in, n_out), 85.0 / 64.0)
    elif name == 'diag':
        k = 37.0 * (i == j)
    elif name == 'rank1':
        k = np.outer(rng.integers(-8, 8, n_in), rng.integers(-8, 8, n_out))
    elif name == 'dup_rows':
        assert n_in % 4 == 0
        k = np.tile(rng.integers(-64, 64, (4, n_out)), (n_in // 4, 1))
    elif name == 'dup_cols':
        assert n_out % 4 == 0
        k = np.tile(rng.integers(-64, 64, (n_in, 4)), (1, n_out // 4))
    elif name == 'neg_cols':
        assert n_out % 3 == 0
        a = rng.integers(-64, 64, (n_in, n_out // 3))
        k = np.concatenate([a, -a, 2 * a], axis=1)
    elif name == 'ternary_sparse':
        k = rng.choice([-1, 0, 1], size=(n_in, n_out), p=[0.05, 0.9, 0.05])
    elif name == 'ternary_dense':
        k = rng.choice([-1, 1], size=(n_in, n_out))
    elif name == 'pow2':  # one digit per cell: no pair inside a cell, all pairs across rows
        k = rng.choice([-1, 1], size=(n_in, n_out)) * 2.0 ** rng.integers(0, 7, (n_in, n_out))
    elif name == 'toeplitz':
        k = 21.0 * (((i - j) % 7) - 3)
    elif name == 'checker_zero':
        k = 51.0 * ((i + j) % 2 == 0)
    elif name == 'one_hot_rows':
        v = rng.integers(1, 64, n_in) * rng.choice([-1, 1], size=n_in)
        k = np.zeros((n_in, n_out))
        k[np.arange(n_in), rng.integers(0, n_out, n_in)] = v
    else:
        raise KeyError(name)
    return np.ascontiguousarray(k + 0.0, dtype=np.float32)


def samples_inside(stage, rng, n):
    """n sample vectors on the grid of a stage's declared input intervals: the executor multiplies input i by 2^inp_shifts[i] and
    wraps the product into the format of the input op's interval, so the samples are drawn in that frame and shifted back"""
    cols = []
    for q, sh in zip(stage.inp_qint, stage.inp_shifts):
        if q.min == q.max == 0:  # an input nothing reads (a zero row; a zero column of stage 0): interval [0, 0], step inf
            cols.append(np.zeros(n))
            continue
        cols.append(rng.integers(round(q.min / q.step), round(q.max / q.step) + 1, n) * q.step * 2.0**-sh)
    return np.stack(cols, axis=1).astype(np.float64)
