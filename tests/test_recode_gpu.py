"""The digit recodings on the GPU (da4ml_amd.cmvm.solve_recoded, 'recode' / 'recode_seed' of solve_each, da_solve_batch_recode): k_init_cells
reading every chain's (mode, seed) from its side array, and every loop kernel on digits that are not non-adjacent, at the smallest shapes that
reach each code path, against tests/golden/recode_golden.json.  The reference always starts from the CSD digits: the records come from a patched
copy of the restatement (tests/golden/make_recode_golden.py), which shares digit_masks of cmvm_core.h with the product and nothing else; point 0
of every case is the reference's result and is compared with the reference build, live."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import int_matrix
from recode_cases import CASES, SINGLE, digest, mixed_batch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'recode_golden.json').read_text())


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


@pytest.mark.parametrize('name', ['small16', 'small32', 'bits8', 'search32', 'mc16', 'wmcdc16'])
def test_points_of_solve_recoded(hip, oracle, name):
    """16x16 3 bit, 32x32 4 bit and 9x12 8 bit as one wmc chain, the default search with hard_dc=2 on 32x32 (both stages, the minimal latency, the
    retries), one mc and one wmc-dc chain: solve, COMPACT and the SEEDED points in one call"""
    from da4ml_amd.cmvm import solve_recoded
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    mat, opts, n, seed = CASES[name]
    k = int_matrix(*mat)
    best, pipes, costs = solve_recoded(k, n, seed=seed, return_all=True, **opts)
    g = GOLDEN['cases'][name]
    assert [digest(p) for p in pipes] == g['digests']
    assert costs == g['costs'] and best == g['best'] and [p.n_adders for p in pipes] == g['adders']
    ref = oracle.solve(k, **opts)
    assert pipes[0] == ref and pipes[0] == hip.solve(k, **opts)
    assert costs[best] <= pipeline_cost_f32(ref)
    for p in pipes:
        assert np.array_equal(p.kernel, k)
    assert solve_recoded(k, n, seed=seed, **opts) == pipes[best]


WIDE_SUB = (
    "import sys, json\nimport numpy as np\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom recode_cases import CASES, digest\nfrom da4ml_amd import _binary as hip\nfrom da4ml_amd.cmvm import solve_recoded\n"
    "mat, opts, n, seed = CASES['wide300']\nk = int_matrix(*mat)\n"
    "best, pipes, costs = solve_recoded(k, n, seed=seed, return_all=True, **opts)\n"
    "print(json.dumps(dict(best=best, costs=costs, digests=[digest(p) for p in pipes], kernel_ok=all(bool(np.array_equal(p.kernel, k)) for p in pipes), "
    "manycol=hip.timings()['manycol_chains'], chains=hip.timings()['chains'])))\n"
)


@pytest.mark.parametrize('manycol', [False, True])
def test_wide_and_many_column(oracle, manycol):
    """4x300 int4 (wide entries: k_init_cells<uint64_t>), four points; the same under DA4ML_HIP_MANYCOL_FROM=1.  A fresh process each: the knob is
    read when the backend is created"""
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
    assert r['digests'][0] == digest(oracle.solve(int_matrix(*mat), **opts))  # point 0 against the reference build, live


def test_mixed_call(hip, oracle):
    """one solve_each call: plain, COMPACT, SEEDED, a SEEDED chain with a tie seed in the newest order and a weighted COMPACT chain, three widths
    (both entry layouts), scrambled -- the descriptors of the call are sorted by kernel variant, the side array with them; every result equals its
    record and the same problem solved alone"""
    batch = mixed_batch()
    assert {label.split(':')[0] for label, _, _ in batch} == {'plain', 'compact', 'seeded', 'seeded-newest', 'compact-w'}
    ks = [int_matrix(*mat) for _, mat, _ in batch]
    got = hip.solve_each(ks, [o for _, _, o in batch])
    for (label, _, _), p, k in zip(batch, got, ks):
        assert np.array_equal(p.kernel, k)
        assert digest(p) == GOLDEN['mixed'][label]['digest'] and p.n_adders == GOLDEN['mixed'][label]['adders'], label
        if label.startswith('plain'):
            assert p == oracle.solve(k, **SINGLE), label
    alone = [hip.solve_each([k], [o])[0] for k, (_, _, o) in zip(ks, batch)]
    assert alone == got


def test_solve_recoded_is_never_dearer_than_solve(hip):
    """32x32 3 bit under the default search: the sizes the compact digits were measured to win at"""
    from da4ml_amd.cmvm import solve_recoded
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    k = int_matrix(0, 32, 32, -4, 4)
    best, pipes, costs = solve_recoded(k, return_all=True)
    plain = hip.solve(k)
    assert len(pipes) == 8 and pipes[0] == plain and costs[0] == pipeline_cost_f32(plain)
    assert costs[best] <= costs[0] and costs[best] == min(costs)
    print('solve_recoded 32x32 3 bit: costs', costs, 'best', best)
    for p in pipes:
        assert np.array_equal(p.kernel, k)


def test_entry_points_and_errors(hip):
    from da4ml_amd.cmvm import restart_seeds, solve_restarts

    mat, opts, n, seed = CASES['bits8']
    k = int_matrix(*mat)
    g = GOLDEN['cases']['bits8']['digests']
    assert digest(hip.solve_each([k], [dict(opts, recode='compact', recode_seed=5)])[0]) == g[1]  # COMPACT reads no seed
    assert hip.solve_each([k], [dict(opts, recode='csd', recode_seed=5)])[0] == hip.solve(k, **opts)
    s = restart_seeds(3, seed)
    want = hip.solve_each([k] * 3, [dict(opts, seed=v, recode='compact') if v else dict(opts) for v in s])
    assert solve_restarts(k, 3, seed=seed, return_all=True, recode='compact', **opts)[1] == want
    assert solve_restarts(k, 3, seed=seed, return_all=True, recode='csd', **opts)[1] == solve_restarts(k, 3, seed=seed, return_all=True, **opts)[1]
    with pytest.raises(ValueError):
        solve_restarts(k, 2, recode='naf', **opts)
    with pytest.raises(ValueError):
        hip.solve_each([k], [dict(opts, recode=2)])
