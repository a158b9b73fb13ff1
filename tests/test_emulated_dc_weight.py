"""The tunable latency-penalty weight of the -dc / -pdc selectors (_binary.solve_each, da_solve_batch_opts, da4ml_amd.cmvm.solve_tradeoff) with the
product's kernels on the emulated device of tests/test_emulated_device.py, through tests/emu/dc_weight_worker.py.

A weight changes the rank of a table entry and nothing else.  Ranks are formed in one place, the block evaluator of cmvm_engine.hip, which four
paths write blocks through (table_insert, table_update, and in k_iter_update the side-by-side re-evaluation and the block creation): a path left
on the method's constant would still give valid adder graphs, but which pick wins would depend on where a block lies in the table and on which
path wrote it last.  So every case and weight is compared with the records of
tests/golden/dc_weight_golden.json -- a patched copy of the restatement, tests/golden/make_dc_weight_golden.py --, the ends of the weight axis
with the unpatched restatement, and the narrow chains must not move when the table's geometry does."""

import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import pytest

from dc_weight_cases import CASES, mixed_call

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'dc_weight_worker.py'
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'dc_weight_golden.json').read_text())['cases']


@pytest.fixture(scope='module')
def emu():
    r = subprocess.run(['make', '-s', '-C', str(EMU_DIR)], capture_output=True, text=True)
    assert r.returncode == 0 and EMU_LIB.exists(), r.stdout[-2000:] + r.stderr[-2000:]

    def run(*args, env=None, timeout=1800):
        e = dict(os.environ, DA4ML_HIP_LIB=str(EMU_LIB), DA4ML_HIP_UPD_BLOCKS='8', **(env or {}))
        out = subprocess.run([sys.executable, str(WORKER), *map(str, args)], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=timeout)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    return run


GEOMETRIES = {'plain': None, '4': dict(DA4ML_HIP_TABLE_SCALE='4'), '0.5': dict(DA4ML_HIP_TABLE_SCALE='0.5'), 'retry': dict(DA4ML_HIP_TABLE_SCALE='0.02', DA4ML_HIP_ROW_SCALE='0.05')}


@pytest.fixture(scope='module')
def runs(emu):
    """every worker run of this file, each in a process of its own, eight side by side: the records of every case (wide300 a second time under the
    many-column carve), the narrow16 chains under four table geometries, and the five single checks"""
    jobs = {('records', name, False): (('records', name), None) for name in CASES}
    jobs[('records', 'wide300', True)] = (('records', 'wide300'), dict(DA4ML_HIP_MANYCOL_FROM='1'))
    jobs.update({('narrow', g): (('narrow',), env) for g, env in GEOMETRIES.items()})
    jobs.update({(what,): ((what,), None) for what in ('pins', 'equivalence', 'mixed', 'errors', 'tradeoff')})
    with ThreadPoolExecutor(8) as pool:
        got = list(pool.map(lambda j: emu(*j[0], env=j[1]), jobs.values()))
    return dict(zip(jobs, got))


@pytest.fixture(scope='module')
def replayed(runs):
    return {(k[1], k[2]): r for k, r in runs.items() if k[0] == 'records'}


@pytest.mark.parametrize('name', list(CASES))
def test_every_case_and_weight_equals_its_record(replayed, name):
    r = replayed[(name, False)]
    assert r['points'] == GOLDEN[name]['points']
    assert r['kernel_ok'] and r['manycol'] == 0 and r['retries'] == 0


def test_wide_entries_under_the_many_column_carve(replayed):
    r = replayed[('wide300', True)]
    assert r['points'] == GOLDEN['wide300']['points'] and r['kernel_ok']
    assert r['manycol'] == r['chains'] > 0


def test_the_records_cover_what_they_should():
    assert GOLDEN['narrow16']['distinct_op_lists'] >= 2
    for name, (_, _, methods, weights) in CASES.items():
        assert set(GOLDEN[name]['points']) == {str(m) for m in methods}
        for m in methods:
            assert len(GOLDEN[name]['points'][str(m)]) == len(weights)
    costs = {p['cost'] for p in GOLDEN['narrow16']['points']['wmc-pdc'].values()}
    assert len(costs) >= 3  # the weight moves the result, not monotonically: 376, 375, 379, 388 when recorded


def test_the_ends_of_the_weight_axis_need_no_patched_oracle(runs):
    """mc-pdc and mc-dc at weight 0 give the op list of mc, wmc-pdc at weight 0 (default intervals) that of wmc, mc-dc at weight 1e6 that of
    mc-dc: all against the restatement as it is committed"""
    pins = runs[('pins',)]['pins']
    assert len(pins) >= 4 and all(pins.values()), pins


def test_the_constant_spelled_out_is_unset_is_solve(runs):
    assert runs[('equivalence',)]['bad'] == []


@pytest.fixture(scope='module')
def narrow_plain(runs):
    return runs[('narrow', 'plain')]


@pytest.mark.parametrize('scale', ['4', '0.5'])
def test_picks_do_not_depend_on_the_table_geometry(runs, narrow_plain, scale):
    """the narrow16 chains with a table four times / half the size: other slots, other groups, blocks created and re-evaluated by other paths --
    the op lists must not move.  A rank formed with the constant at one site shows here"""
    r = runs[('narrow', scale)]
    assert r['op_lists'] == narrow_plain['op_lists'] and r['kernel_ok'] and r['retries'] == 0
    assert narrow_plain['distinct'] >= 2


def test_the_weight_survives_a_capacity_retry(runs, narrow_plain):
    r = runs[('narrow', 'retry')]
    assert r['retries'] >= 1 and r['op_lists'] == narrow_plain['op_lists'] and r['kernel_ok']


def test_one_call_with_mixed_options(runs):
    """methods, weights, a seed, both entry layouts and a searching solve in one solve_each call; positions 1 and 4 differ in their weight ONLY: a
    weight missing from the de-duplication of equal problems would hand one of them the other's result.  Positions 10 and 11 are larger problems
    at their method's own weight beside smaller weighted ones of the same layout"""
    r = runs[('mixed',)]
    assert len(r['equal']) == len(mixed_call()) and all(r['equal']) and all(r['kernel_ok'])
    assert r['weight_matters'] and r['digests'][1] == r['digests'][9]
    assert r['digests'][1] == GOLDEN['narrow16']['points']['wmc-pdc']['1.0']['digest']
    assert r['digests'][4] == GOLDEN['narrow16']['points']['wmc-pdc']['4.0']['digest']


def test_errors(runs):
    r = runs[('errors',)]
    for label in ('-0.5', 'nan', 'inf', '-1'):  # (None, not -1, spells "unset" in Python)
        assert r[label].startswith('ValueError') and 'dc_weight must be a finite number >= 0' in r[label], (label, r[label])
    for label in ('-0.5', 'nan', 'inf'):
        assert r['abi ' + label] == [-2, 'dc_weight must be a finite number >= 0']  # DA_ERR_VALUE from the library itself
    assert r['length'].startswith('ValueError')


def test_solve_tradeoff(runs):
    r = runs[('tradeoff',)]
    front, pts = r['front'], r['points']
    assert r['calls'] == [1 + 2 * (1 + 8)] and len(pts) == 19 and r['kernel_ok']  # ONE da_solve_batch_opts call with every point
    assert r['point0_is_solve'] and pts[0][0] == r['solve_cost'] and pts[0][2:5] == [None, None, None]
    assert r['front_only_ok']
    # ordered and non-dominated: ascending latency, strictly decreasing cost; every point is on the front or dominated by a member
    assert all(a[1] < b[1] and a[0] > b[0] for a, b in zip(front, front[1:]))
    assert all(p in pts for p in front)
    for p in pts:
        assert p in front or any(f[0] <= p[0] and f[1] <= p[1] for f in front)
    # point 0 is on the front, or strictly dominated (an equal never displaces it)
    assert pts[0] in front or any((f[0] <= pts[0][0] and f[1] <= pts[0][1]) and (f[0] < pts[0][0] or f[1] < pts[0][1]) for f in front)
    assert r['within'][0] <= r['solve_cost'] and r['within'][1] <= pts[0][1]
    assert 'smallest latency available' in r['below'] and str(front[0][1]) in r['below']
    # the labels: each method at its own weight, then the eight default weights
    assert [p[2:5] for p in pts[1:10]] == [['wmc-pdc', 'wmc-pdc', w] for w in (None, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)]
    assert [p[2:5] for p in pts[10:]] == [['wmc-dc', 'wmc-dc', w] for w in (None, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0)]


def test_front_rules_on_made_up_points():
    """ascending latency, strictly decreasing cost; of equal (cost, latency) the earliest stays; cheapest_within names the smallest latency"""
    from da4ml_amd.cmvm import TradeoffPoint, cheapest_within, pareto_front

    pt = lambda i, cost, lat: TradeoffPoint(float(cost), float(lat), None, None, None, i)  # noqa: E731
    pts = [pt(0, 100, 9), pt(1, 110, 8), pt(2, 100, 9), pt(3, 105, 8), pt(4, 105, 8), pt(5, 120, 7), pt(6, 99, 10), pt(7, 130, 7), pt(8, 101, 9)]
    front = pareto_front(pts)
    assert [p.pipeline for p in front] == [5, 3, 0, 6]
    assert cheapest_within(front, 9).pipeline == 0 and cheapest_within(front, 8.5).pipeline == 3 and cheapest_within(front, 1000).pipeline == 6
    with pytest.raises(ValueError, match='smallest latency available is 7.0'):
        cheapest_within(front, 6.9)


def test_solve_tradeoff_takes_solve_s_keywords_only():
    from da4ml_amd.cmvm import solve_tradeoff

    for key in ('seed', 'dc_weight'):
        with pytest.raises(TypeError, match=key):
            solve_tradeoff(None, **{key: 1})
