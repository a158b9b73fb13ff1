"""The newest-row-first tie order (order='newest' of da4ml_amd.cmvm.solve_restarts, 'tie_order' of _binary.solve_each, da_solve_opts.tie_order)
with the product's kernels on the emulated device of tests/test_emulated_device.py, through tests/emu/newest_worker.py, against
tests/golden/newest_golden.json -- records of a patched copy of the restatement (tests/golden/make_newest_golden.py), which shares the word
function of cmvm_core.h with the product and nothing else.

What a mistake in the kernels looks like here: a site that forms or takes apart the word of the other order (or the reference's) in a
newest-order chain gives picks that are still valid graphs -- but not the records', and which pick wins then depends on where a block lies in the
table and on which of the two ways a step finds its pick.  The emulated build runs candidate lists of two entries, so both ways run all the
time; the geometry tests move every block."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'tests'))

from newest_cases import CASES, MANYCOL, NARROW  # noqa: E402

EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'newest_worker.py'
GOLDEN = json.loads((ROOT / 'tests' / 'golden' / 'newest_golden.json').read_text())
OLD = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']


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
    assert r['costs'][r['best']] <= r['costs'][0] and r['best'] == min(range(len(r['costs'])), key=lambda i: (r['costs'][i], i))


@pytest.mark.parametrize('name', list(CASES))
def test_restarts_in_the_newest_order_are_the_records(plain_runs, name):
    """16x16 and 32x32 narrow, 4x300 wide, the searching 32x32 with hard_dc=2, one mc and one wmc-dc chain: each as a batch with restart 0"""
    r = plain_runs[name]
    check_case(r, name)
    assert r['retries'] == 0 and r['manycol'] == 0
    assert len(set(r['digests'])) > 1  # the seeds matter


def test_restart_0_is_the_reference_order_and_the_newest_order_is_not_the_random_one(plain_runs):
    for name in ('small16', 'small32', 'wide300', 'search32'):  # the cases tests/restart_cases.py has too, with the same seeds
        assert plain_runs[name]['digests'][0] == OLD[name]['digests'][0], name
        n = len(plain_runs[name]['digests'])
        assert plain_runs[name]['digests'][1:] != OLD[name]['digests'][1:n], name


def test_many_column_carve(emu):
    """4x300 again under DA4ML_HIP_MANYCOL_FROM=1: k_iter_select2<Cell, false, MANYCOL, SEEDED>"""
    r = emu('case', MANYCOL, env=dict(DA4ML_HIP_MANYCOL_FROM='1'))
    check_case(r, MANYCOL)
    assert r['manycol'] > 0


@pytest.mark.parametrize('scale', ['4', '0.5'])
@pytest.mark.parametrize('name', NARROW)
def test_picks_are_maximal_whatever_the_table_geometry(emu, plain_runs, name, scale):
    """the narrow chains with a table four times / half the size: other slots, other groups, blocks met in another order -- the op lists must not
    move.  This is the test that catches a site left on another word"""
    r = emu('case', name, env=dict(DA4ML_HIP_TABLE_SCALE=scale))
    assert r['ops'] == plain_runs[name]['ops']
    assert r['retries'] == 0 or (name, scale) == ('small32', '0.5')  # (half a table does not hold the 32x32 chains: they are run again in a larger one, the same op lists)
    check_case(r, name)


@pytest.mark.parametrize('name', NARROW)
def test_the_order_survives_a_capacity_retry(emu, plain_runs, name):
    r = emu('case', name, env=dict(DA4ML_HIP_TABLE_SCALE='0.02', DA4ML_HIP_ROW_SCALE='0.05'))
    assert r['retries'] >= 1 and r['ops'] == plain_runs[name]['ops']
    check_case(r, name)


def test_one_call_mixes_unseeded_random_newest_and_a_weighted_newest_chain(emu):
    """three widths (16x16, 9x12 narrow; 4x300 wide), scrambled: every result equals its result alone, and its record"""
    r = emu('mixed')
    assert r['kernel_ok']
    kinds = {label.split(':')[0] for label in r['labels']}
    assert kinds == {'plain', 'random', 'newest', 'newest-w'}
    assert r['together'] == r['alone']
    for label, d, cost, adders in zip(r['labels'], r['together'], r['costs'], r['adders']):
        kind, mat, *rest = label.split(':')
        if kind == 'plain':
            assert d == r['plain'][label] == OLD[mat]['digests'][0], label  # tie_order='newest' with seed 0: solve itself
        elif kind == 'random':
            assert d == OLD[mat]['digests'][int(rest[0])], label  # tests/golden/restarts_golden.json: nothing that was has moved
        else:
            g = GOLDEN['mixed'][label]
            assert (d, cost, adders) == (g['digest'], g['cost'], g['adders']), label
    assert set(GOLDEN['mixed']) == {label for label in r['labels'] if label.startswith('newest')}


def test_c_abi_struct_sizes_and_orders(emu):
    r = emu('abi')
    g = GOLDEN['cases']['small16']
    assert (r['size_v1'], r['size'], r['last_field']) == (56, 64, 'tie_order')
    # the previous struct_size (an array of the previous struct): accepted, the random order -- what da_solve_batch_seeded gives
    assert r['v1'] == [0, OLD['small16']['digests'][1:3]] and r['seeded_api'] == OLD['small16']['digests'][1:3]
    assert r['new_random'] == r['v1']
    assert r['new_newest'] == [0, g['digests'][1:3]]
    assert r['seed0_newest'] == [0, [r['plain']]] and r['plain'] == g['digests'][0]
    for key in [k for k in r if k.startswith('size ')] + ['mixed sizes']:
        assert r[key][0] == -2 and 'struct_size' in r[key][1], key  # DA_ERR_VALUE
    for key in ('order 2', 'order 3', 'order 4294967295'):
        assert r[key] == [-2, 'tie_order must be DA_TIE_RANDOM or DA_TIE_NEWEST'], key
    assert r['order 2 seed 0'] == -2


def test_header_states_the_contract():
    h = (ROOT / 'include' / 'da4ml_hip.h').read_text()
    assert '#define DA_TIE_RANDOM 0u' in h and '#define DA_TIE_NEWEST 1u' in h
    assert 'uint32_t tie_order;\n} da_solve_opts;' in h  # the last field
    assert 'no reference counterpart' in h[h.index('tie_order (addition') : h.index('#define DA_TIE_RANDOM')]


def test_python_entry_points(emu):
    r = emu('python_api')
    g = GOLDEN['cases']['small16']['digests'][:4]
    assert r['default'] == r['random'] == OLD['small16']['digests'][:4]  # the default stays 'random'
    assert r['newest'] == r['many_newest'] == g
    assert r['many_newest_no_seeds'] == [r['plain']] and r['newest'][0] == r['plain']
    assert {k: v for k, v in r.items() if k.startswith('error')} == {'error restarts': 'ValueError', 'error restarts None': 'ValueError', 'error many': 'ValueError', 'error each': 'ValueError'}


def test_restarts_sharded_takes_the_order(emu):
    r = emu('sharded', env=dict(RANK='0', WORLD_SIZE='1', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT='29617', DA4ML_PIN_RANKS='0'))
    assert r['newest'] == r['want_newest'] != r['random'] and r['random'] == r['want_random'] and r['error'] == 'ValueError'
