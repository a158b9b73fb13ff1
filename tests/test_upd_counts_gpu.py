"""k_iter_update counts the digit pairs of a partner row once and reads the losses of A's and B's blocks through the inverse key map (upd_loss,
cmvm_engine.hip): the cases of tests/upd_diet_cases.py on the GPU, whole Pipeline against the oracle; the seeded and the weighted instantiations
against the records of tests/golden.  The same cases run on the emulated device in tests/test_upd_counts_emulated.py."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import int_matrix
from upd_diet_cases import GROUPS, SINGLE, TIGHT_TABLE_SCALE, self_pairs

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


def child(*groups, **env):
    """the worker of the emulated test in a fresh process on the GPU: the library reads its environment once"""
    e = {k: v for k, v in os.environ.items() if k != 'DA4ML_HIP_LIB'}
    out = subprocess.run([sys.executable, str(ROOT / 'tests' / 'emu' / 'upd_diet_worker.py'), *groups], env=dict(e, **env), capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('group', ['same_row', 'shifts', 'long_rows', 'wide_cells'])
def test_group(hip, oracle, group):
    """picks of a row with itself, mirrored partners, shifted B-role keys, partner rows of more than 32 and 64 entries, 64-bit cells"""
    add = sub = 0
    for mat in GROUPS[group]:
        k = int_matrix(*mat)
        got, want = hip.solve(k, **SINGLE), oracle.solve(k, **SINGLE)
        assert got == want, mat
        assert np.all(got.kernel == k)
        a, s = self_pairs(want)
        add, sub = add + a, sub + s
    if group == 'same_row':
        assert add >= 1 and sub >= 1  # the cases do hold picks of a row with itself, of either sign


def test_several_passes_per_wavefront():
    """48x16 with two update blocks per chain: 32 partner rows per pass, 94 per step on average"""
    r = child('passes', DA4ML_HIP_UPD_BLOCKS='2')
    assert r['bad'] == [] and r['partners_per_step'] > 64


def test_blocks_beyond_their_home_bucket():
    """the same chain with the tightest table that completes without the capacity retry on the emulated device"""
    r = child('passes', DA4ML_HIP_UPD_BLOCKS='2', DA4ML_HIP_TABLE_SCALE=TIGHT_TABLE_SCALE)
    assert r['bad'] == []


def test_seeded_instantiation(hip):
    """k_iter_update<uint32_t, ..., SEEDED>: the eight restarts of the 16x16 case of tests/restart_cases.py against their record"""
    from restart_cases import CASES, digest

    from da4ml_amd.cmvm import solve_restarts

    golden = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']['small16']
    mat, opts, n, seed = CASES['small16']
    best, pipes, costs = solve_restarts(int_matrix(*mat), n, seed=seed, return_all=True, **opts)
    assert [digest(p) for p in pipes] == golden['digests'] and costs == golden['costs'] and best == golden['best']


@pytest.mark.parametrize('name', ['narrow16', 'mc12'])
def test_weighted_instantiation(hip, name):
    """k_iter_update<uint32_t, ..., WEIGHTED>: every method and weight of the small cases of tests/dc_weight_cases.py against their records"""
    from dc_weight_cases import CASES, digest, points, wkey

    golden = json.loads((ROOT / 'tests' / 'golden' / 'dc_weight_golden.json').read_text())['cases'][name]['points']
    k = int_matrix(*CASES[name][0])
    pts = points(name)
    pipes = hip.solve_each([k] * len(pts), [p[2] for p in pts])
    for (m, w, *_), p in zip(pts, pipes):
        assert digest(p) == golden[str(m)][wkey(w)]['digest'], (m, w)
        assert np.all(p.kernel == k)
