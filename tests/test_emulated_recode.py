"""The digit recodings (da4ml_amd.cmvm.solve_recoded, 'recode' / 'recode_seed' of _binary.solve_each, da_solve_batch_recode) with the product's
kernels on the emulated device of tests/test_emulated_device.py, through tests/emu/recode_worker.py, against tests/golden/recode_golden.json --
records of a patched copy of the restatement (tests/golden/make_recode_golden.py), which shares digit_masks of cmvm_core.h with the product and
nothing else.

What a mistake looks like here: a chain that starts from other digits than its mode's gives a valid graph of the matrix -- but not the record's;
a side array read at the wrong index (the descriptors of a batch are sorted by kernel variant, the jobs are not) gives a chain the digits of
its neighbour, which shows in the mixed call and nowhere else."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'tests'))

from recode_cases import CASES, MANYCOL, NARROW  # noqa: E402

EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'recode_worker.py'
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'recode_golden.json').read_text())
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
    assert r['kernel_ok'] and r['cost_ok']  # every graph implements the matrix; the cost is the float32 sum of its ops
    assert r['digests'] == g['digests'], [a == b for a, b in zip(r['digests'], g['digests'])]
    assert r['costs'] == g['costs'] and r['adders'] == g['adders'] and r['best'] == g['best']
    assert r['digests'][0] == r['plain']  # point 0 is solve
    assert r['winner'] == r['digests'][r['best']]
    assert r['costs'][r['best']] <= r['costs'][0] and r['best'] == min(range(len(r['costs'])), key=lambda i: (r['costs'][i], i))


@pytest.mark.parametrize('name', list(CASES))
def test_points_of_solve_recoded_are_the_records(plain_runs, name):
    """3 and 4 bit narrow, 8 bit, 4x300 wide, the searching 32x32 with hard_dc=2, one mc and one wmc-dc chain: each as one call with point 0"""
    r = plain_runs[name]
    check_case(r, name)
    assert r['retries'] == 0 and r['manycol'] == 0
    assert r['digests'][1] != r['digests'][0]  # the compact digits are other digits


def test_many_column_carve(emu):
    """4x300 again under DA4ML_HIP_MANYCOL_FROM=1"""
    r = emu('case', MANYCOL, env=dict(DA4ML_HIP_MANYCOL_FROM='1'))
    check_case(r, MANYCOL)
    assert r['manycol'] > 0


@pytest.mark.parametrize('scale', ['4', '0.5'])
@pytest.mark.parametrize('name', NARROW)
def test_graphs_do_not_depend_on_the_table_geometry(emu, plain_runs, name, scale):
    """the narrow chains with a table four times / half the size: the engine assumes non-adjacent digits nowhere, so the op lists must not move"""
    r = emu('case', name, env=dict(DA4ML_HIP_TABLE_SCALE=scale))
    assert r['ops'] == plain_runs[name]['ops']
    check_case(r, name)


@pytest.mark.parametrize('name', NARROW)
def test_the_recoding_survives_a_capacity_retry(emu, plain_runs, name):
    r = emu('case', name, env=dict(DA4ML_HIP_TABLE_SCALE='0.02', DA4ML_HIP_ROW_SCALE='0.05'))
    assert r['retries'] >= 1 and r['ops'] == plain_runs[name]['ops']
    check_case(r, name)


def test_one_call_mixes_plain_compact_seeded_a_newest_order_and_a_weighted_chain(emu):
    """three widths (16x16, 9x12 narrow; 4x300 wide), scrambled: every result equals its result alone, and its record"""
    r = emu('mixed')
    assert r['kernel_ok']
    assert {label.split(':')[0] for label in r['labels']} == {'plain', 'compact', 'seeded', 'seeded-newest', 'compact-w'}
    assert r['together'] == r['alone']
    assert set(GOLDEN['mixed']) == set(r['labels'])
    for label, d, cost, adders in zip(r['labels'], r['together'], r['costs'], r['adders']):
        g = GOLDEN['mixed'][label]
        assert (d, cost, adders) == (g['digest'], g['cost'], g['adders']), label
        if label.startswith('plain'):
            assert d == r['plain'][label], label  # mode CSD, with or without a seed: solve itself


def test_c_abi_contract(emu):
    r = emu('abi')
    g = GOLDEN['cases']['bits8']
    assert (r['size'], r['opts_size']) == (16, 64)  # da_solve_opts has not grown
    assert r['opts'][0] == 0 and r['null'] == r['opts'] and r['csd'] == r['opts']  # NULL and CSD: da_solve_batch_opts
    assert r['opts'][1] == [g['digests'][0]] * 2
    assert r['compact'] == [0, [g['digests'][1]] * 2] and r['compact_seed_ignored'] == r['compact']  # COMPACT reads no seed
    assert r['seeded'] == [0, g['digests'][2:4]] and r['seeded_again'] == r['seeded']
    # with a tie seed in the second problem: CSD is still da_solve_batch_opts, and the recoding goes into the seeded chain too
    assert r['tied_opts'][0] == 0 and r['tied_csd'] == r['tied_opts'] and r['tied_opts'][1][1] != g['digests'][0]
    assert r['tied_compact'][1][0] == g['digests'][1] and r['tied_compact'][1][1] not in (g['digests'][1], r['tied_opts'][1][1])
    assert r['each_tied_compact'] == r['tied_compact'][1]
    for key in ('mode 3', 'mode 4', 'mode 4294967295'):
        assert r[key] == [-2, 'recode mode must be DA_RECODE_CSD, DA_RECODE_COMPACT or DA_RECODE_SEEDED'], key  # DA_ERR_VALUE
    for key in [k for k in r if k.startswith('size ')]:
        assert r[key][0] == -2 and 'struct_size' in r[key][1], key


def test_column_sharded_chains_take_csd_only(emu):
    r = emu('shard', env=dict(DA4ML_SHARD_FORCE='1'))
    assert r['0'][0] == r['plain'] and r['0'][1] > 0  # sharded chains ran, and mode CSD is the plain solve
    for mode in ('1', '2'):
        assert r[mode][0] == 'ValueError' and 'column-sharded' in r[mode][1] and r[mode][2] == -2, r[mode]  # DA_ERR_VALUE


def test_header_states_the_contract():
    h = (ROOT / 'include' / 'da4ml_hip.h').read_text()
    assert '#define DA_RECODE_CSD 0u' in h and '#define DA_RECODE_COMPACT 1u' in h and '#define DA_RECODE_SEEDED 2u' in h
    assert 'uint32_t tie_order;\n} da_solve_opts;' in h  # untouched
    doc = h[h.index('da_solve_batch_opts with a digit recoding') : h.index('#define DA_RECODE_CSD')]
    for words in ('no reference counterpart', 'recode == NULL, or mode DA_RECODE_CSD, is da_solve_batch_opts bit for bit', 'DA_ERR_VALUE', 'whatever else the batch holds', 'on every run'):
        assert words in doc, words


def test_python_entry_points(emu):
    r = emu('python_api')
    assert r['default'] == r['csd'] == OLD['small16']['digests'][:4]  # recode='csd' is today's solve_restarts
    assert r['csd_newest'] == r['newest'] == NEWEST['small16']['digests'][:4]
    for mode in ('compact', 'seeded'):
        assert r[mode][0] == r['plain'] and r[mode] == r[mode + '_each'] == r[mode + '_many']  # restart 0 stays solve; restarts >= 1 run the mode with their seed
        assert all(a != b for a, b in zip(r[mode][1:], r['csd'][1:]))
    assert r['compact'][1:] != r['seeded'][1:]
    g = GOLDEN['cases']['bits8']['digests']
    assert r['recoded'] == r['recoded_each'] == g and r['recoded'][0] == r['recoded_plain'] == r['recoded_one']
    assert {k: v for k, v in r.items() if k.startswith('error')} == {'error restarts': 'ValueError', 'error restarts None': 'ValueError', 'error many': 'ValueError',
                                                                      'error each': 'ValueError', 'error recoded seed': 'TypeError', 'error recoded n': 'ValueError'}  # fmt: skip


def test_restarts_sharded_takes_the_recoding(emu):
    r = emu('sharded', env=dict(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29619', DA4ML_PIN_RANKS='0'))
    assert r['compact'] == r['want_compact'] and r['csd'] == r['want_csd'] and r['error'] == 'ValueError'
