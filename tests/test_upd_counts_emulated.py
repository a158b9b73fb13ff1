"""k_iter_update counts the digit pairs of a partner row once and reads the losses of A's and B's blocks through the inverse key map (upd_loss,
cmvm_engine.hip): the cases of tests/upd_diet_cases.py on the emulated device (tests/emu: the product's kernels on the CPU), whole Pipeline against the
oracle; the seeded and the weighted instantiations against the records of tests/golden.  The same cases run on the GPU in tests/test_upd_counts_gpu.py."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
from upd_diet_cases import GROUPS, TIGHT_TABLE_SCALE

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'


@pytest.fixture(scope='module')
def emu():
    r = subprocess.run(['make', '-s', '-C', str(EMU_DIR)], capture_output=True, text=True)
    assert r.returncode == 0 and EMU_LIB.exists(), r.stdout[-2000:] + r.stderr[-2000:]

    def run(worker, *args, env=None):
        e = {**os.environ, 'DA4ML_HIP_LIB': str(EMU_LIB), 'DA4ML_HIP_UPD_BLOCKS': '8', **(env or {})}
        out = subprocess.run([sys.executable, str(EMU_DIR / worker), *map(str, args)], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    return run


def test_self_pairs_mirrored_partners_and_shifted_keys(emu):
    """12x10, 16x16 and 8x8 int8: picks of a row with itself (both loss vectors in A's block), adding and subtracting, partners on both sides of A
    and B, B-role keys at both ends of the count vector"""
    r = emu('upd_diet_worker.py', 'same_row', 'shifts')
    assert r['bad'] == [] and r['n'] == len(GROUPS['same_row']) + len(GROUPS['shifts'])
    assert r['self_add'] >= 1 and r['self_sub'] >= 1  # the cases do hold picks of a row with itself, of either sign


def test_long_partner_rows_and_wide_cells(emu):
    """partner rows of more than 32 and 64 list entries (6x40, 4x64, 3x96); 64-bit cells (8x8 of 15 bits, 2x300)"""
    r = emu('upd_diet_worker.py', 'long_rows', 'wide_cells')
    assert r['bad'] == [] and r['n'] == len(GROUPS['long_rows']) + len(GROUPS['wide_cells'])


def test_several_passes_per_wavefront(emu):
    """48x16 with two update blocks per chain: 32 partner rows per pass, 94 per step on average -- the counters are zeroed and re-read pass after pass"""
    r = emu('upd_diet_worker.py', 'passes', env=dict(DA4ML_HIP_UPD_BLOCKS='2'))
    assert r['bad'] == [] and r['retries'] == 0 and r['partners_per_step'] > 64


def test_blocks_beyond_their_home_bucket(emu):
    """the same chain with the tightest table that completes without the capacity retry: look-ups beyond the first bucket and creations into a
    full bucket take the wave-wide path, whose loss lambdas read the same counters through the same map"""
    r = emu('upd_diet_worker.py', 'passes', env=dict(DA4ML_HIP_UPD_BLOCKS='2', DA4ML_HIP_TABLE_SCALE=TIGHT_TABLE_SCALE))
    assert r['bad'] == [] and r['retries'] == 0


def test_seeded_instantiation(emu):
    """k_iter_update<uint32_t, ..., SEEDED>: the eight restarts of the 16x16 case of tests/restart_cases.py against their record"""
    golden = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']['small16']
    r = emu('restart_worker.py', 'fixed', 8, 1)
    assert r['digests'] == golden['digests'] and r['costs'] == golden['costs'] and r['kernel_ok']


@pytest.mark.parametrize('name', ['narrow16', 'mc12'])
def test_weighted_instantiation(emu, name):
    """k_iter_update<uint32_t, ..., WEIGHTED>: every method and weight of the small cases of tests/dc_weight_cases.py against their records"""
    golden = json.loads((ROOT / 'tests' / 'golden' / 'dc_weight_golden.json').read_text())['cases'][name]
    r = emu('dc_weight_worker.py', 'records', name)
    assert r['points'] == golden['points'] and r['kernel_ok']
