"""Seeded random restarts of the greedy search on the GPU: the SEEDED instantiations of k_init_pairs, k_iter_select2 and k_iter_update at the
smallest shapes at which each of them runs, against tests/golden/restarts_golden.json.  The reference has no restarts: the records come from the
same kernels on the emulated device (tests/golden/make_restarts_golden.py), where candidate lists of two entries make most steps find their
pick the long way; restart 0 of every case is the reference's result and is compared with the reference build, live."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import int_matrix
from restart_cases import CASES, MIXED, SINGLE, digest, mixed_batch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


def check_against_golden(name, pipes, costs, best):
    g = GOLDEN[name]
    assert [digest(p) for p in pipes] == g['digests']
    assert costs == g['costs'] and best == g['best']


@pytest.mark.parametrize('name', ['small16', 'small32'])
def test_small_matrices(hip, oracle, name):
    """16x16 and 32x32 int8, one wmc chain, eight restarts: k_init_pairs / k_iter_select2 / k_iter_update <uint32_t, ..., SEEDED> beside the unseeded restart 0"""
    from da4ml_amd.cmvm import solve_restarts
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    mat, opts, n, seed = CASES[name]
    k = int_matrix(*mat)
    best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, **opts)
    check_against_golden(name, pipes, costs, best)
    ref = oracle.solve(k, **opts)
    assert pipes[0] == ref
    assert costs[best] <= pipeline_cost_f32(ref)
    for p in pipes:
        assert np.all(p.kernel == k)
    assert solve_restarts(k, n, seed=seed, **opts) == pipes[best]


WIDE_SUB = (
    "import sys, json\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom restart_cases import CASES, digest\nfrom da4ml_amd import _binary as hip\nfrom da4ml_amd.cmvm import solve_restarts\n"
    "mat, opts, n, seed = CASES['wide300']\nk = int_matrix(*mat)\n"
    "best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, **opts)\n"
    "print(json.dumps(dict(best=best, costs=costs, digests=[digest(p) for p in pipes], kernel_ok=all(bool((p.kernel == k).all()) for p in pipes), "
    "manycol=hip.timings()['manycol_chains'], chains=hip.timings()['chains'])))\n"
)


@pytest.mark.parametrize('manycol', [False, True])
def test_wide_and_many_column(manycol):
    """4x300 int4 (wide entries: the uint64_t instantiations), four restarts; the same under DA4ML_HIP_MANYCOL_FROM=1 (many-column x seeded).  A fresh
    process each: the knob is read when the backend is created"""
    e = {k: v for k, v in os.environ.items() if k != 'DA4ML_HIP_MANYCOL_FROM'}
    if manycol:
        e['DA4ML_HIP_MANYCOL_FROM'] = '1'
    out = subprocess.run([sys.executable, '-c', WIDE_SUB], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    g = GOLDEN['wide300']
    assert r['digests'] == g['digests'] and r['costs'] == g['costs'] and r['best'] == g['best'] and r['kernel_ok']
    assert r['manycol'] == (r['chains'] if manycol else 0)


def test_mixed_batch(hip):
    """one solve_many call of 24 problems: three matrices of different widths (both entry layouts), seeds {0, s1 .. s7} each, interleaved -- seeded
    and unseeded ranges of both layouts advance in the same lockstep; every result equals its record and the same problem solved alone"""
    from da4ml_amd.cmvm import restart_seeds

    order = mixed_batch()
    assert len(order) == 24
    mats = {name: int_matrix(*MIXED[name][0]) for name in MIXED}
    seeds = {name: restart_seeds(MIXED[name][2], MIXED[name][3]) for name in MIXED}
    got = hip.solve_many([mats[name] for name, _ in order], seeds=[seeds[name][r] for name, r in order], **SINGLE)
    for (name, r), p in zip(order, got):
        assert digest(p) == GOLDEN[name]['digests'][r], (name, r)
        assert np.all(p.kernel == mats[name])
    alone = [hip.solve_many([mats[name]], seeds=[seeds[name][r]], **SINGLE)[0] for name, r in order]
    assert alone == got


def test_default_search(hip):
    """search_all_decompose_dc=True, hard_dc=2 on 32x32, four restarts: the minimal-latency probe (no seed), the latency retries and every
    decompose_dc candidate of every restart carry the restart's seed through both stages"""
    from da4ml_amd.cmvm import solve_restarts

    mat, opts, n, seed = CASES['search32']
    k = int_matrix(*mat)
    best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, **opts)
    check_against_golden('search32', pipes, costs, best)
    for p in pipes:
        assert np.all(p.kernel == k)


def test_determinism(hip):
    """30 repetitions of one seeded 32x32 solve"""
    from da4ml_amd.cmvm import restart_seeds

    mat, opts, n, seed = CASES['small32']
    k, s = int_matrix(*mat), restart_seeds(n, seed)[1]
    assert s != 0
    digests = {digest(hip.solve_many([k], seeds=[s], **opts)[0]) for _ in range(30)}
    assert digests == {GOLDEN['small32']['digests'][1]}


def test_one_restart_is_solve(hip):
    from da4ml_amd.cmvm import solve_restarts

    k = int_matrix(3, 24, 20, -128, 128)
    assert solve_restarts(k, 1, seed=12345) == hip.solve(k)
    assert hip.solve_many([k], seeds=[0])[0] == hip.solve(k)
