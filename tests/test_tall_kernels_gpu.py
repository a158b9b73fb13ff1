"""Kernels with more input rows than the pair-table heuristic can size (768 to 2048 rows): tables of more than 2^25 slots are capped by
the row pairs the chain can hold (da4ml_amd/csrc/cmvm_geometry.h), groups of 2^15 slots and more run through the selection's tail loops.
Checked against the reference's own sources (live, or the records of tests/golden/large_chain_golden.json / tall_golden.json)."""

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from cases import int_matrix

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / 'golden'
SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


def digest(p):
    dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))
    return hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest()


SUB = (
    "import sys, json, hashlib, time\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom da4ml_amd import _binary as hip\n"
    "args, opts = json.loads(sys.argv[1]), json.loads(sys.argv[2])\nk = int_matrix(*args)\n"
    "t = time.perf_counter()\np = hip.solve(k, **opts)\ndt = time.perf_counter() - t\ntm = hip.timings()\n"
    "dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))\n"
    "print(json.dumps({'cost': p.cost, 'n_ops': [len(s.ops) for s in p.solutions], 'seconds': dt, 'kernel_ok': bool((p.kernel == k).all()),\n"
    "                  'sha256': hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest(),\n"
    "                  **{n: tm[n] for n in ('retries', 'table_bytes', 'arena_bytes', 'iterations', 'loop_ms')}}))\n"
)


def solve_in_subprocess(args, opts, **env):
    """one solve in a fresh process: the table and row scales are read when the backend is created"""
    e = dict(os.environ, **{k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, '-c', SUB, json.dumps(args), json.dumps(opts)], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(args, opts, env, {k: v for k, v in r.items() if k != 'sha256'})
    return r


def table_slots(r):
    """slots of the pair table from table_bytes = C x (key 8 + rank 4 + a payload line of 2^k bytes): C is the power of two that divides it so"""
    tb = int(r['table_bytes'])
    for log2c in range(8, 31):
        c = 1 << log2c
        if tb % c == 0 and tb // c > 12 and ((tb // c - 12) & (tb // c - 13)) == 0:
            return c
    raise AssertionError(f'table_bytes {tb} is not C x (12 + 2^k)')


@pytest.mark.parametrize('name,scale,gs_log2', [('128x128_seed0', 200, 15), ('128x128_seed0', 400, 16), ('256x256_seed0', 25, 15), ('256x256_seed0', 50, 16)])
def test_recorded_matrix_through_large_groups(name, scale, gs_log2):
    """the records of the reference build, solved with tables forced to 2048 groups of 2^15 / 2^16 slots (the selection's tail loops read
    groups beyond the 1024 slots it holds in registers)"""
    rec = json.loads((GOLDEN / 'large_chain_golden.json').read_text())[name + '_single_chain_ref']
    n, seed = int(name.split('x')[0]), int(name.split('seed')[1])
    r = solve_in_subprocess([seed, n, n, -128, 128], rec['opts'], DA4ML_HIP_TABLE_SCALE=scale)
    assert r['retries'] == 0
    assert table_slots(r) == 2048 << gs_log2
    assert r['arena_bytes'] < 40e9
    assert r['cost'] == rec['cost'] and r['n_ops'] == rec['n_ops'] and r['sha256'] == rec['sha256']


@pytest.mark.parametrize('shape', [(1, 768, 1, -128, 128), (1, 1024, 4, -8, 8), (1, 1024, 8, -8, 8)])
def test_tall_kernel_single_chain_against_oracle(hip, oracle, shape):
    k = int_matrix(*shape)
    got = hip.solve(k, **SINGLE)
    assert got == oracle.solve(k, **SINGLE)
    assert (got.kernel == k).all()


@pytest.mark.parametrize('shape', [(1, 768, 1, -128, 128), (1, 1024, 4, -8, 8)])
def test_tall_kernel_default_search_against_oracle(hip, oracle, shape):
    k = int_matrix(*shape)
    got = hip.solve(k)
    assert got == oracle.solve(k)
    assert (got.kernel == k).all()


@pytest.mark.parametrize('name', ['1024x16_int4_seed1_single_chain', '1024x16_int4_seed1_default'])
def test_1024x16_against_reference_record(hip, name):
    """1024x16 int4: minutes on the CPU oracle, so against the record of the reference build (tests/golden/make_tall_golden.py)"""
    rec = json.loads((GOLDEN / 'tall_golden.json').read_text())[name]
    k = int_matrix(*rec['matrix'])
    p = hip.solve(k, **rec['opts'])
    assert (p.kernel == k).all()
    assert p.cost == rec['cost'] and [len(s.ops) for s in p.solutions] == rec['n_ops'] and digest(p) == rec['sha256']


def test_dropin_solve_of_a_tall_kernel(hip, oracle):
    """through install_as_da4ml() and da4ml.cmvm.solve, as a converted flatten -> dense layer would call it"""
    import da4ml_amd

    before = {k for k in sys.modules if k == 'da4ml' or k.startswith('da4ml.')}
    da4ml_amd.install_as_da4ml()
    try:
        from da4ml.cmvm import solve

        k = int_matrix(2, 768, 2, -128, 128)
        sol = solve(k)
        assert (sol.kernel == k).all()
        assert sol == oracle.solve(k)
    finally:
        for name in [m for m in sys.modules if (m == 'da4ml' or m.startswith('da4ml.')) and m not in before]:
            del sys.modules[name]


def test_dense_1024x64_int8_single_chain():
    """too slow for the CPU oracle: the kernel is reproduced, and the result does not depend on the table size or on the run"""
    args = [3, 1024, 64, -128, 128]
    a = solve_in_subprocess(args, SINGLE)
    b = solve_in_subprocess(args, SINGLE, DA4ML_HIP_TABLE_SCALE=0.5)
    c = solve_in_subprocess(args, SINGLE)
    assert a['kernel_ok'] and b['kernel_ok'] and c['kernel_ok']
    assert a['table_bytes'] != b['table_bytes']
    assert a['sha256'] == b['sha256'] == c['sha256']
    assert max(a['arena_bytes'], b['arena_bytes']) < 40e9


def test_mixed_batch_of_small_and_tall_kernels(hip):
    ks = [int_matrix(4, 64, 64, -128, 128), int_matrix(5, 1024, 8, -8, 8), int_matrix(6, 64, 64, -8, 8)]
    batch = hip.solve_many(ks, **SINGLE)
    for k, p in zip(ks, batch):
        assert p == hip.solve(k, **SINGLE)
        assert (p.kernel == k).all()


def test_column_sharded_tall_kernel():
    """one rank, the sharded phases forced: equal to the unsharded solve"""
    code = (
        "import os, sys, json\nos.environ['DA4ML_SHARD_FORCE'] = '1'\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
        "from cases import int_matrix\nfrom da4ml_amd import _binary as hip\n"
        "k = int_matrix(7, 768, 4, -8, 8)\nopts = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)\n"
        "p, st = hip.solve_sharded(k, rank=0, world=1, **opts)\nq = hip.solve(k, **opts)\n"
        "print(json.dumps({'same': bool(p == q), 'kernel_ok': bool((p.kernel == k).all()), 'stats': st}))\n"
    )
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(r)
    assert r['same'] and r['kernel_ok'] and r['stats']['sharded_chains'] >= 1
