"""The tunable latency-penalty weight of the -dc / -pdc selectors on the GPU: the WEIGHTED instantiations of k_init_pairs and k_iter_update at the
smallest shapes at which each site that forms a rank and each entry layout runs, against tests/golden/dc_weight_golden.json (a patched copy of the
restatement, tests/golden/make_dc_weight_golden.py).  Results at the methods' own weights are compared with the reference build, live."""

import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import int_matrix
from dc_weight_cases import CASES, digest, latency_of, matrix_args, mixed_call, points, wkey

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
RECORDS = json.loads((ROOT / 'tests' / 'golden' / 'dc_weight_golden.json').read_text())
GOLDEN = RECORDS['cases']


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


def solve_abi(hip, k, options, qintervals=None, latencies=None):
    """every point of a case in ONE da_solve_batch_opts call, the structs filled here (not by solve_each)"""
    n = len(options)
    opts = (hip.SolveOpts * n)()
    for i, o in enumerate(options):
        w = o.get('dc_weight')
        opts[i] = hip.SolveOpts(C.sizeof(hip.SolveOpts), o.get('method0', 'wmc').encode(), o.get('method1', 'auto').encode(), o.get('hard_dc', -1), o.get('decompose_dc', -2),
                                o.get('adder_size', -1), o.get('carry_size', -1), int(o.get('search_all_decompose_dc', True)), hip.DC_WEIGHT_DEFAULT if w is None else w, o.get('seed', 0))  # fmt: skip
    q = None if qintervals is None else np.ascontiguousarray(np.asarray(qintervals, np.float32).reshape(-1, 3))
    l = None if latencies is None else np.ascontiguousarray(np.asarray(latencies, np.float32))
    res = (C.c_void_p * n)()
    rc = hip.lib().da_solve_batch_opts(n, (C.c_void_p * n)(*[k.ctypes.data] * n), np.full(n, k.shape[0], np.int64), np.full(n, k.shape[1], np.int64), C.cast(opts, C.c_void_p),
                                       None if q is None else (C.c_void_p * n)(*[q.ctypes.data] * n), None if l is None else (C.c_void_p * n)(*[l.ctypes.data] * n), res)  # fmt: skip
    assert rc == 0, hip.lib().da_last_error().decode()
    return [hip._collect(res[i]) for i in range(n)]


def record_of(p):
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    return dict(digest=digest(p), cost=pipeline_cost_f32(p), latency=latency_of(p), adders=p.n_adders)


@pytest.mark.parametrize('name', ['narrow16', 'mc12', 'lat16', 'search32'])
def test_records_through_the_c_abi(hip, name):
    k = int_matrix(*CASES[name][0])
    pts = points(name)
    pipes = solve_abi(hip, k, [p[2] for p in pts], pts[0][3], pts[0][4])
    for (m, w, *_), p in zip(pts, pipes):
        assert record_of(p) == GOLDEN[name]['points'][str(m)][wkey(w)], (m, w)
        assert np.all(p.kernel == k)


WIDE_SUB = (
    "import sys, json\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom dc_weight_cases import CASES, points, wkey\nimport test_dc_weight_gpu as t\nfrom da4ml_amd import _binary as hip\n"
    "k = int_matrix(*CASES['wide300'][0])\npts = points('wide300')\npipes = t.solve_abi(hip, k, [p[2] for p in pts])\n"
    "print(json.dumps(dict(points={wkey(w): t.record_of(p) for (m, w, *_), p in zip(pts, pipes)}, kernel_ok=all(bool((p.kernel == k).all()) for p in pipes), "
    "manycol=hip.timings()['manycol_chains'], chains=hip.timings()['chains'])))\n"
)


@pytest.mark.parametrize('manycol', [False, True])
def test_wide_entries_and_the_many_column_carve(manycol):
    """4x300 (wide entries: the uint64_t instantiations) at two weights; the same under DA4ML_HIP_MANYCOL_FROM=1.  A fresh process each: the knob is
    read when the backend is created"""
    e = {k: v for k, v in os.environ.items() if k != 'DA4ML_HIP_MANYCOL_FROM'}
    if manycol:
        e['DA4ML_HIP_MANYCOL_FROM'] = '1'
    out = subprocess.run([sys.executable, '-c', WIDE_SUB], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r['points'] == GOLDEN['wide300']['points']['wmc-dc'] and r['kernel_ok']
    assert r['manycol'] == (r['chains'] if manycol else 0)


def test_one_call_with_mixed_options(hip):
    """methods, weights, a seed, both entry layouts and a searching solve in one solve_each call: weighted and unweighted ranges of both layouts
    advance in the same lockstep; every result equals the same problem solved alone; positions 1 and 4 differ in their weight only; in either
    layout a larger problem at its method's own weight runs beside smaller weighted ones, which launch the same selection kernel"""
    call = mixed_call()
    mats = {name: int_matrix(*matrix_args(name)) for name, _ in call}
    got = hip.solve_each([mats[name] for name, _ in call], [o for _, o in call])
    alone = [hip.solve_each([mats[name]], [o])[0] for name, o in call]
    assert got == alone
    for (name, _), p in zip(call, got):
        assert np.all(p.kernel == mats[name])
    assert digest(got[1]) == GOLDEN['narrow16']['points']['wmc-pdc']['1.0']['digest'] == digest(got[9])
    assert digest(got[4]) == GOLDEN['narrow16']['points']['wmc-pdc']['4.0']['digest'] != digest(got[1])
    assert digest(got[0]) == GOLDEN['wide300']['points']['wmc-dc']['0.3']['digest']
    assert digest(got[2]) == GOLDEN['mc12']['points']['mc-pdc']['2.5']['digest']


def test_a_large_problem_at_its_own_weight_beside_a_small_weighted_one(hip):
    """2x2000 int4 (wide entries; its selection blocks ask for more than 64 KB of dynamic LDS, which a kernel gets only after its limit was raised) at
    the constant of wmc-dc, and the 4x300 matrix at weight 0.3: both ranges launch the same k_iter_select2 instantiation, whose limit must cover the
    larger.  Each result equals the problem solved alone, in either order"""
    big, small = int_matrix(25, 2, 2000, -8, 8), int_matrix(*CASES['wide300'][0])
    one = dict(decompose_dc=-1, search_all_decompose_dc=False, method0='wmc-dc', method1='wmc-dc')
    alone = [hip.solve_each([big], [one])[0], hip.solve_each([small], [dict(one, dc_weight=0.3)])[0]]
    assert digest(alone[1]) == GOLDEN['wide300']['points']['wmc-dc']['0.3']['digest']
    assert hip.solve_each([big, small], [one, dict(one, dc_weight=0.3)]) == alone
    assert hip.solve_each([small, big], [dict(one, dc_weight=0.3), one]) == alone[::-1]
    assert np.all(alone[0].kernel == big)


@pytest.mark.parametrize('name', ['narrow16', 'mc12', 'lat16'])
def test_the_methods_own_weights_against_the_reference_build(hip, reference_oracle, name):
    """unset, and the constant spelled out (256 resp. 1e9): the reference's result"""
    mat, opts, methods, _ = CASES[name]
    k = int_matrix(*mat)
    per = {key: v for key, v in opts.items() if key not in ('qintervals', 'latencies')}
    kw = {key: [opts[key]] * 2 for key in ('qintervals', 'latencies') if key in opts}
    for m in methods:
        ref = reference_oracle.solve(k, **dict(opts, method0=m, method1=m))
        got = hip.solve_each([k] * 2, [dict(per, method0=m, method1=m), dict(per, method0=m, method1=m, dc_weight=1e9 if m.startswith('mc') else 256.0)], **kw)
        assert got[0] == ref and got[1] == ref, m
        assert hip.solve(k, **dict(opts, method0=m, method1=m)) == ref


def test_solve_tradeoff_gives_the_front_of_the_emulated_device(hip):
    from da4ml_amd.cmvm import cheapest_within, solve_tradeoff
    from da4ml_amd.multi_gpu import pipeline_cost_f32

    k, opts = int_matrix(*CASES['narrow16'][0]), CASES['narrow16'][1]
    front, pts = solve_tradeoff(k, return_all=True, **opts)
    assert solve_tradeoff(k, **opts) == front
    row = lambda p: [p.cost, p.latency, p.method0, p.method1, p.dc_weight, digest(p.pipeline)]  # noqa: E731
    want = RECORDS['tradeoff_narrow16']
    assert [row(p) for p in pts] == want['points']
    assert [row(p) for p in front] == want['front']
    plain = hip.solve(k, **opts)
    assert pts[0].pipeline == plain
    assert cheapest_within(front, pts[0].latency).cost <= pipeline_cost_f32(plain)
    with pytest.raises(ValueError, match='smallest latency available'):
        cheapest_within(front, front[0].latency - 1)


def test_errors(hip):
    k = int_matrix(*CASES['mc12'][0])
    for w in (-0.5, float('nan'), float('inf'), -1.0):  # (None, not -1, spells "unset" in Python)
        with pytest.raises(ValueError, match='dc_weight must be a finite number >= 0'):
            hip.solve_each([k], [dict(dc_weight=w)])
    with pytest.raises(ValueError):
        hip.solve_each([k, k], [{}])
