"""The newest-row-first tie order on the GPU (solve_restarts(order='newest'), 'tie_order' of solve_each): the SEEDED instantiations of
k_init_pairs, k_iter_select2 and k_iter_update reading the chain's order, at the smallest shapes at which each of them runs, against
tests/golden/newest_golden.json.  The reference has no seeded order: the records come from a patched copy of the restatement
(tests/golden/make_newest_golden.py), which shares the word function of cmvm_core.h with the product and nothing else; restart 0 of every case is
the reference's result and is compared with the reference build, live."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import int_matrix
from newest_cases import CASES, SINGLE, digest, mixed_batch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'newest_golden.json').read_text())
OLD = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


def check_against_golden(name, pipes, costs, best):
    g = GOLDEN['cases'][name]
    assert [digest(p) for p in pipes] == g['digests']
    assert costs == g['costs'] and best == g['best'] and [p.n_adders for p in pipes] == g['adders']
    assert costs[best] <= costs[0]


@pytest.mark.parametrize('name', ['small16', 'small32', 'search32', 'mc16', 'wmcdc16'])
def test_restarts_in_the_newest_order(hip, oracle, name):
    """16x16 and 32x32 int8 as one wmc chain (eight restarts), the default search with hard_dc=2 on 32x32, one mc and one wmc-dc chain at 16x16
    (four restarts): the seeded kernels beside the unseeded restart 0"""
    from da4ml_amd.cmvm import solve_restarts
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    mat, opts, n, seed = CASES[name]
    k = int_matrix(*mat)
    best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, order='newest', **opts)
    check_against_golden(name, pipes, costs, best)
    ref = oracle.solve(k, **opts)
    assert pipes[0] == ref
    assert costs[best] <= pipeline_cost_f32(ref)
    for p in pipes:
        assert np.all(p.kernel == k)
    assert solve_restarts(k, n, seed=seed, order='newest', **opts) == pipes[best]


WIDE_SUB = (
    "import sys, json\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom newest_cases import CASES, digest\nfrom da4ml_amd import _binary as hip\nfrom da4ml_amd.cmvm import solve_restarts\n"
    "mat, opts, n, seed = CASES['wide300']\nk = int_matrix(*mat)\n"
    "best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, order='newest', **opts)\n"
    "print(json.dumps(dict(best=best, costs=costs, digests=[digest(p) for p in pipes], kernel_ok=all(bool((p.kernel == k).all()) for p in pipes), "
    "manycol=hip.timings()['manycol_chains'], chains=hip.timings()['chains'])))\n"
)


@pytest.mark.parametrize('manycol', [False, True])
def test_wide_and_many_column(oracle, manycol):
    """4x300 int4 (wide entries: the uint64_t instantiations), four restarts; the same under DA4ML_HIP_MANYCOL_FROM=1 (many-column x seeded).  A fresh
    process each: the knob is read when the backend is created"""
    e = {k: v for k, v in os.environ.items() if k != 'DA4ML_HIP_MANYCOL_FROM'}
    if manycol:
        e['DA4ML_HIP_MANYCOL_FROM'] = '1'
    out = subprocess.run([sys.executable, '-c', WIDE_SUB], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    g = GOLDEN['cases']['wide300']
    assert r['digests'] == g['digests'] and r['costs'] == g['costs'] and r['best'] == g['best'] and r['kernel_ok']
    assert r['manycol'] == (r['chains'] if manycol else 0)
    mat, opts, _, _ = CASES['wide300']
    assert r['digests'][0] == digest(oracle.solve(int_matrix(*mat), **opts))  # restart 0 against the reference build, live


def test_mixed_call(hip, oracle):
    """one solve_each call: unseeded, random-seeded, newest-seeded and one weighted newest chain, three widths (both entry layouts), scrambled --
    all of them advance in the same lockstep; every result equals its record and the same problem solved alone"""
    batch = mixed_batch()
    assert {label.split(':')[0] for label, _, _ in batch} == {'plain', 'random', 'newest', 'newest-w'}
    ks = [int_matrix(*mat) for _, mat, _ in batch]
    got = hip.solve_each(ks, [o for _, _, o in batch])
    for (label, _, _), p, k in zip(batch, got, ks):
        kind, mat, *rest = label.split(':')
        assert np.all(p.kernel == k)
        if kind == 'plain':
            assert p == oracle.solve(k, **SINGLE), label
        elif kind == 'random':
            assert digest(p) == OLD[mat]['digests'][int(rest[0])], label
        else:
            assert digest(p) == GOLDEN['mixed'][label]['digest'] and p.n_adders == GOLDEN['mixed'][label]['adders'], label
    alone = [hip.solve_each([k], [o])[0] for k, (_, _, o) in zip(ks, batch)]
    assert alone == got


def test_entry_points_and_errors(hip):
    from da4ml_amd.cmvm import restart_seeds, solve_restarts

    mat, opts, n, seed = CASES['small16']
    k = int_matrix(*mat)
    g = GOLDEN['cases']['small16']['digests']
    assert [digest(p) for p in hip.solve_many([k] * 3, seeds=restart_seeds(3, seed), tie_order='newest', **opts)] == g[:3]
    assert [digest(p) for p in solve_restarts(k, 3, seed=seed, return_all=True, **opts)[1]] == OLD['small16']['digests'][:3]  # the default stays 'random'
    assert hip.solve_each([k], [dict(opts, tie_order='newest')])[0] == hip.solve(k, **opts)  # seed 0: the reference whatever the order says
    with pytest.raises(ValueError):
        solve_restarts(k, 2, order='oldest', **opts)
    with pytest.raises(ValueError):
        hip.solve_each([k], [dict(opts, seed=1, tie_order=2)])
