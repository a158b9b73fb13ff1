"""The many-column form of the selection kernel's substitution block (k_iter_select2<Cell, false, MANYCOL>: B's list worked on where it lies
in memory, 16-bit per-column arrays, no copy of the column lengths) on the emulated device of tests/test_emulated_device.py.  The host takes
it for chains whose regular carve does not fit beside the kernel's static LDS (from about 3300 columns on the real device);
DA4ML_HIP_MANYCOL_FROM=1 forces it for every chain, so that the small problems of tests/emu/worker.py -- unchanged -- run through it, in both
entry layouts and in batches.  What this cannot check: that pass 2 of the block sees what pass 1 wrote to memory from other wavefronts
(nothing runs concurrently here); the `-m gpu` tests of tests/test_wide_kernels_gpu.py do."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
LDS_LIMIT = 160 * 1024 - 256  # the emulated device's LDS per workgroup less the reserve of sel2_lds_budget


@pytest.fixture(scope='module')
def emu():
    r = subprocess.run(['make', '-s', '-C', str(EMU_DIR)], capture_output=True, text=True)
    assert r.returncode == 0 and EMU_LIB.exists(), r.stdout[-2000:] + r.stderr[-2000:]

    def run(*args, env=None, timeout=900):
        e = dict(os.environ, DA4ML_HIP_LIB=str(EMU_LIB), DA4ML_HIP_UPD_BLOCKS='8', **(env or {}))
        out = subprocess.run([sys.executable, str(EMU_DIR / 'worker.py'), *map(str, args)], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=timeout)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    return run


FORCED = dict(DA4ML_HIP_MANYCOL_FROM='1')


@pytest.mark.parametrize('block', range(3))
def test_random_option_sets_forced_manycol(emu, block):
    assert emu('random', block * 40, block * 40 + 40, env=FORCED) == {'bad': [], 'n': 40}


def test_entry_layouts_forced_manycol(emu):
    """narrow and wide entries (the 16-bit arrays hold columns up to 256 here), 256 / 257 columns, one row, one column, zeros"""
    assert emu('layouts', env=FORCED)['bad'] == []


def test_structured_matrices_forced_manycol(emu):
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(2) as pool:
        res = list(pool.map(lambda part: emu('structured', part, 2, env=FORCED), range(2)))
    assert [r['bad'] for r in res] == [[], []]
    assert sum(r['n'] for r in res) == res[0]['total'] == 52


def test_batched_chains_forced_manycol(emu):
    r = emu('batch', env=FORCED)
    assert r['bad'] == [] and r['chains'] >= 13


def test_knob_threshold_mixes_both_carves_in_a_batch(emu):
    """from 8 columns on: the batch of worker.batch() holds chains of 4 to 10 columns in both layouts, so all four kernel variants
    (narrow / wide x regular / many-column) run side by side, each over its own range of the sorted descriptors"""
    r = emu('batch', env=dict(DA4ML_HIP_MANYCOL_FROM='8'))
    assert r['bad'] == [] and r['chains'] >= 13


def test_host_takes_manycol_when_only_its_carve_fits(emu):
    """no knob.  The 12-column chains of worker.lds_budget() need 976 bytes of dynamic LDS with the regular carve (B's list 48, six count
    vectors, five int arrays of 12 and one more word) and 800 with the many-column one (976 - 48 - 2 x 12 x 4 - 3 x 12 x 2, rounded up to 16):
    with 900 bytes left beside the static arrays the regular carve is refused (as the parent refuses the chain) and the many-column one runs;
    with 700 bytes neither fits, and the message names the many-column carve's size"""
    only_manycol = emu('lds_budget', env=dict(HIPEMU_STATIC_LDS=str(LDS_LIMIT - 900)))
    none = emu('lds_budget', env=dict(HIPEMU_STATIC_LDS=str(LDS_LIMIT - 700)))
    assert only_manycol == {'ok': True, 'bad': [], 'message': ''}
    assert not none['ok'] and 'needs 800 bytes of dynamic LDS' in none['message'] and 'n_out too large' in none['message']


UPD_SUB = (
    "import sys, json\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from cases import int_matrix\nfrom da4ml_amd import _binary as hip\n"
    "try:\n    hip.solve(int_matrix(1, 2, 3000, -8, 8), method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)\n    print(json.dumps({'message': ''}))\n"
    "except RuntimeError as e:\n    print(json.dumps({'message': str(e)}))\n"
)


def test_update_kernel_refuses_what_the_device_cannot_hold():
    """a 3000-column chain: k_iter_update asks for 22 x 3000 + 3328 = 69 328 bytes of dynamic LDS, more than 64 KB, so the sum with its static
    arrays is checked against the 160 KB of a workgroup.  With 100 000 bytes reported as static the selection still fits (many-column carve:
    30 KB of the 63 KB left) and the update kernel does not: the call fails with both sizes in the message, not with a raw launch error"""
    r = subprocess.run(['make', '-s', '-C', str(EMU_DIR)], capture_output=True, text=True)
    assert r.returncode == 0 and EMU_LIB.exists(), r.stdout[-2000:] + r.stderr[-2000:]
    e = dict(os.environ, DA4ML_HIP_LIB=str(EMU_LIB), DA4ML_HIP_UPD_BLOCKS='8', HIPEMU_STATIC_LDS='100000')
    out = subprocess.run([sys.executable, '-c', UPD_SUB], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    msg = json.loads(out.stdout.strip().splitlines()[-1])['message']
    assert 'update kernel needs 69328 bytes of dynamic LDS beside 100000' in msg and '163840' in msg and 'n_out too large' in msg
