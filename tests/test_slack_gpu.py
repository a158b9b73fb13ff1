"""The score slack on the GPU (slack= of da4ml_amd.cmvm.solve_restarts, 'slack' of solve_each, da_solve_batch_search): the SLACK instantiations of
k_init_pairs and k_iter_update at the smallest shapes that reach each code path, against tests/golden/slack_golden.json.  The reference has no
such option: the records come from a patched copy of the restatement (tests/golden/make_slack_golden.py), which shares entry_rank_slack,
slack_byte and tie_word of cmvm_core.h with the product and nothing else; restart 0 of every case is the reference's result and is compared with
the reference build, live."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import int_matrix
from slack_cases import CASES, SINGLE, digest, mixed_batch, restart_options

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'slack_golden.json').read_text())


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


@pytest.mark.parametrize('name', ['small16', 'small32', 'search32', 'mc16', 'wmcdc16', 'wmcdcw16', 'newest16', 'compact16'])
def test_restarts_with_a_slack(hip, oracle, name):
    """16x16 and 32x32 int8 as one wmc chain, the default search with hard_dc=2 on 32x32 (both stages, every candidate, the retries), one mc chain,
    one wmc-dc chain on its constant and one with dc_weight=3.3, the newest-first order, the compact digits: restart 0 and the slack restarts in one call"""
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    mat, opts, n, _, _, _ = CASES[name]
    k = int_matrix(*mat)
    pipes = hip.solve_each([k] * n, restart_options(name))
    g = GOLDEN['cases'][name]
    assert [digest(p) for p in pipes] == g['digests']
    assert [pipeline_cost_f32(p) for p in pipes] == g['costs'] and [p.n_adders for p in pipes] == g['adders']
    if 'dc_weight' not in opts:  # (the reference has the constants only)
        assert pipes[0] == oracle.solve(k, **opts) and pipes[0] == hip.solve(k, **opts)
    for p in pipes:
        assert np.array_equal(p.kernel, k)


WIDE_SUB = (
    "import sys, json\nimport numpy as np\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom slack_cases import CASES, digest, restart_options\nfrom da4ml_amd import _binary as hip\nfrom da4ml_amd.multi_gpu import pipeline_cost_f32\n"
    "mat, opts, n = CASES['wide300'][:3]\nk = int_matrix(*mat)\n"
    "pipes = hip.solve_each([k] * n, restart_options('wide300'))\n"
    "print(json.dumps(dict(costs=[pipeline_cost_f32(p) for p in pipes], digests=[digest(p) for p in pipes], kernel_ok=all(bool(np.array_equal(p.kernel, k)) for p in pipes), "
    "manycol=hip.timings()['manycol_chains'], chains=hip.timings()['chains'])))\n"
)


@pytest.mark.parametrize('manycol', [False, True])
def test_wide_and_many_column(oracle, manycol):
    """4x300 int4 (wide entries), four restarts; the same under DA4ML_HIP_MANYCOL_FROM=1.  A fresh process each: the knob is read when the backend
    is created"""
    e = {k: v for k, v in os.environ.items() if k != 'DA4ML_HIP_MANYCOL_FROM'}
    if manycol:
        e['DA4ML_HIP_MANYCOL_FROM'] = '1'
    out = subprocess.run([sys.executable, '-c', WIDE_SUB], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    g = GOLDEN['cases']['wide300']
    assert r['digests'] == g['digests'] and r['costs'] == g['costs'] and r['kernel_ok']
    assert r['manycol'] == (r['chains'] if manycol else 0)
    mat, opts = CASES['wide300'][:2]
    assert r['digests'][0] == digest(oracle.solve(int_matrix(*mat), **opts))  # restart 0 against the reference build, live


def test_mixed_call(hip, oracle):
    """one solve_each call: unseeded chains, seeded chains without a slack, slack chains at two slacks and a weighted newest-order one, three widths
    (both entry layouts), scrambled -- the descriptors of the call are sorted by kernel variant; every result equals its record and the same
    problem solved alone"""
    batch = mixed_batch()
    assert {label.split(':')[0] for label, _, _ in batch} == {'plain', 'seeded', 'slack5', 'slack16', 'slack16-newest-w'}
    ks = [int_matrix(*mat) for _, mat, _ in batch]
    got = hip.solve_each(ks, [o for _, _, o in batch])
    for (label, _, _), p, k in zip(batch, got, ks):
        assert np.array_equal(p.kernel, k)
        assert digest(p) == GOLDEN['mixed'][label]['digest'] and p.n_adders == GOLDEN['mixed'][label]['adders'], label
        if label.startswith('plain'):
            assert p == oracle.solve(k, **SINGLE), label
    alone = [hip.solve_each([k], [o])[0] for k, (_, _, o) in zip(ks, batch)]
    assert alone == got


def test_entry_points_and_errors(hip):
    from da4ml_amd.cmvm import restart_seeds, solve_restarts

    mat, opts, n, seed, slack, _ = CASES['small16']
    k = int_matrix(*mat)
    g = GOLDEN['cases']['small16']
    best, pipes, costs = solve_restarts(k, n, seed=seed, slack=slack, return_all=True, **opts)
    assert [digest(p) for p in pipes] == g['digests'] and best == g['best'] and costs == g['costs'] and costs[best] <= costs[0]
    assert solve_restarts(k, n, seed=seed, slack=slack, **opts) == pipes[best]
    assert hip.solve_many([k] * n, seeds=restart_seeds(n, seed), slack=slack, **opts) == pipes
    assert solve_restarts(k, 3, seed=seed, slack=0, return_all=True, **opts)[1] == solve_restarts(k, 3, seed=seed, return_all=True, **opts)[1]
    for bad in (256, -1, 2.0, '4', None, True):
        with pytest.raises(ValueError):
            solve_restarts(k, 2, slack=bad, **opts)
    with pytest.raises(ValueError):
        hip.solve_each([k], [dict(opts, slack=4)])  # a slack is keyed by the seed
    with pytest.raises(ValueError):
        hip.solve_many([k], seeds=[1], slack=300, **opts)
