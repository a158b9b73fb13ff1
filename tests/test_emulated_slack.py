"""The score slack (slack= of da4ml_amd.cmvm.solve_restarts, 'slack' of _binary.solve_each, da_solve_batch_search) with the product's kernels on
the emulated device of tests/test_emulated_device.py, through tests/emu/slack_worker.py, against tests/golden/slack_golden.json -- records of a
patched copy of the restatement (tests/golden/make_slack_golden.py), which shares entry_rank_slack, slack_byte and tie_word of cmvm_core.h with
the product and nothing else.

What a mistake looks like here: a rank formed past the block evaluator, or with the rows of another block, gives valid graphs whose picks depend on
where a block lies in the table -- they move with the table's size; a descriptor of the sorted batch read at the job's index gives a chain the
slack of its neighbour, which shows in the mixed call and nowhere else."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'tests'))

from slack_cases import CASES, MANYCOL, NARROW  # noqa: E402

EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'slack_worker.py'
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'slack_golden.json').read_text())
OLD = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']
NEWEST = json.loads((ROOT / 'tests' / 'golden' / 'newest_golden.json').read_text())['cases']


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


@pytest.fixture(scope='module')
def plain_runs(emu):
    """every case once under the default geometry, side by side"""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(len(CASES)) as pool:
        return dict(zip(CASES, pool.map(lambda name: emu('case', name), CASES)))


def check_case(r, name):
    g = GOLDEN['cases'][name]
    assert r['kernel_ok']  # every graph implements the matrix
    assert r['digests'] == g['digests'], [a == b for a, b in zip(r['digests'], g['digests'])]
    assert r['costs'] == g['costs'] and r['adders'] == g['adders'] and r['best'] == g['best']
    if 'dc_weight' not in CASES[name][1]:
        assert r['digests'][0] == r['plain']  # restart 0 is solve
    assert r['costs'][r['best']] <= r['costs'][0]


@pytest.mark.parametrize('name', list(CASES))
def test_restarts_with_a_slack_are_the_records(plain_runs, name):
    """16x16 and 32x32 narrow, 4x300 wide, the searching 32x32 with hard_dc=2, mc, wmc-dc on its constant and on another weight, the newest-first
    order, a recoding: each as one call with restart 0"""
    r = plain_runs[name]
    check_case(r, name)
    assert r['retries'] == 0 and r['manycol'] == 0
    assert any(GOLDEN['cases'][name]['moved']) and len(set(r['digests'])) > 1  # (the records do differ from the slack-0 restarts)


def test_many_column_carve(emu):
    """4x300 again under DA4ML_HIP_MANYCOL_FROM=1"""
    r = emu('case', MANYCOL, env=dict(DA4ML_HIP_MANYCOL_FROM='1'))
    check_case(r, MANYCOL)
    assert r['manycol'] > 0


@pytest.mark.parametrize('scale', ['4', '0.5'])
@pytest.mark.parametrize('name', NARROW)
def test_graphs_do_not_depend_on_the_table_geometry(emu, plain_runs, name, scale):
    """the narrow chains with a table four times / half the size: a rank is a function of the entry, not of where its block lies"""
    r = emu('case', name, env=dict(DA4ML_HIP_TABLE_SCALE=scale))
    assert r['ops'] == plain_runs[name]['ops']
    check_case(r, name)


@pytest.mark.parametrize('name', NARROW)
def test_the_slack_survives_a_capacity_retry(emu, plain_runs, name):
    r = emu('case', name, env=dict(DA4ML_HIP_TABLE_SCALE='0.02', DA4ML_HIP_ROW_SCALE='0.05'))
    assert r['retries'] >= 1 and r['ops'] == plain_runs[name]['ops']
    check_case(r, name)


def test_one_call_mixes_unseeded_seeded_and_two_slacks(emu):
    """three widths (16x16, 9x12 narrow; 4x300 wide), scrambled: every result equals its result alone, and its record"""
    r = emu('mixed')
    assert r['kernel_ok']
    assert {label.split(':')[0] for label in r['labels']} == {'plain', 'seeded', 'slack5', 'slack16', 'slack16-newest-w'}
    assert r['together'] == r['alone']
    assert set(GOLDEN['mixed']) == set(r['labels'])
    for label, d, cost, adders in zip(r['labels'], r['together'], r['costs'], r['adders']):
        g = GOLDEN['mixed'][label]
        assert (d, cost, adders) == (g['digest'], g['cost'], g['adders']), label
        if label.startswith('plain'):
            assert d == r['plain'][label], label
    by = dict(zip(r['labels'], r['together']))
    assert len({by['seeded:mix300'], by['slack16:mix300'], by['plain:mix300']}) == 3  # one seed: the slack is what differs


def test_nothing_recorded_before_moves(emu):
    r = emu('old')
    for name in ('small16', 'wide300'):
        assert r[f'random:{name}'] == r[f'random:{name}:slack0'] == OLD[name]['digests'], name
    for name in ('small16', 'wmcdc16'):
        assert r[f'newest:{name}'] == r[f'newest:{name}:slack0'] == NEWEST[name]['digests'], name


def test_c_abi_contract(emu):
    r = emu('abi')
    g = GOLDEN['cases']['small16']
    assert (r['size'], r['opts_size'], r['recode_size']) == (8, 64, 16)  # the two older structs have not grown
    assert r['recode'][0] == 0 and r['null'] == r['recode'] and r['zero'] == r['recode']  # NULL and slack 0: da_solve_batch_recode
    assert r['recode'][1] == OLD['small16']['digests'][1:3]
    assert r['slack'] == [0, g['digests'][1:3]] and r['slack_again'] == r['slack']
    assert r['one'] == [0, [r['recode'][1][0], g['digests'][2]]]  # per problem
    assert r['half'] == [0, [g['digests'][0], g['digests'][2]]]
    assert r['255'][0] == 0 and r['255'][1] != r['slack'][1]
    for key in ('slack 256', 'slack 1000', 'slack 4294967295'):
        assert r[key] == [-2, 'slack must lie in 0 .. 255'], key  # DA_ERR_VALUE
    for key in [k for k in r if k.startswith('size ')]:
        assert r[key][0] == -2 and 'struct_size' in r[key][1], key
    assert r['no seed'][0] == -2 and 'seed' in r['no seed'][1]
    # beside a recoding: NULL is still da_solve_batch_recode, and the slack goes into the recoded chains too
    assert r['compact_recode'][0] == 0 and r['compact_null'] == r['compact_recode']
    assert r['compact_slack'][0] == 0 and all(a != b for a, b in zip(r['compact_slack'][1], r['compact_recode'][1])) and r['compact_slack'][1] != r['slack'][1]


def test_column_sharded_chains_take_no_slack(emu):
    r = emu('shard', env=dict(DA4ML_SHARD_FORCE='1'))
    assert r['0'][0] == r['plain'] and r['0'][1] > 0  # sharded chains ran, and slack 0 is the plain solve
    assert r['16'][0] == 'ValueError' and 'column-sharded' in r['16'][1] and r['16'][2] == -2, r['16']  # DA_ERR_VALUE


def test_header_states_the_contract():
    h = (ROOT / 'include' / 'da4ml_hip.h').read_text()
    assert 'uint32_t tie_order;\n} da_solve_opts;' in h and '    uint64_t seed;\n} da_recode_opts;' in h  # untouched
    doc = h[h.index('da_solve_batch_recode with a score slack') : h.index('} da_search_opts;')]
    for words in ('no reference counterpart', 'search == NULL, or slack 0, is da_solve_batch_recode bit for bit', 'slack > 255', 'DA_ERR_VALUE', 'seed == 0',
                  'whatever else the batch holds', 'on every run', 'never a', 'restart dimension'):  # fmt: skip
        assert words in doc, words


def test_python_entry_points(emu):
    r = emu('python_api')
    for name in ('small16', 'newest16', 'compact16'):
        g = GOLDEN['cases'][name]
        assert r[name] == r[name + ' many'] == g['digests'], name
        assert r[name + ' best'] == g['best'] and r[name + ' winner'] == g['digests'][g['best']] and r[name + ' never dearer'], name
        assert r[name][0] == r['plain']  # restart 0 stays solve
    assert r['slack0'] == r['default'] == OLD['small16']['digests']
    assert r['numpy int'] == GOLDEN['cases']['small16']['digests'][:2]
    want = {'error ' + k: 'ValueError' for k in ('restarts 256', 'restarts -1', 'restarts float', 'restarts str', 'restarts None', 'restarts bool', 'many', 'each', 'each no seed')}
    want['error recoded'] = 'TypeError'
    assert {k: v for k, v in r.items() if k.startswith('error')} == want


def test_restarts_sharded_takes_the_slack(emu):
    r = emu('sharded', env=dict(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29623', DA4ML_PIN_RANKS='0'))
    assert r['slack'] == r['real'] == r['want_slack'] and r['flat'] == r['zero'] == r['want_flat'] and r['error'] == 'ValueError'
    assert r['saw_slack'] == [True, False, False]  # the solver sees the option only when it is not 0
