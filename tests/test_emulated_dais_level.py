"""Kernel k_dais_exec_level of the compiled DAIS executables (csrc/dais_gpu.hip) on the emulated device of tests/test_emulated_device.py,
through tests/emu/dais_level_worker.py: mode='level' with the value file in LDS and in global memory, tiles of every fill, levels wider
than the block and of one statement, strides, element types, the golden vectors, the table fault -- all bit for bit the host
composition.  The emulation checks indexing and logic of the kernel and of the host code around it, not its speed."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'dais_level_worker.py'
KNOBS = ('DA4ML_DAIS_MODE', 'DA4ML_DAIS_LEVEL_LDS', 'DA4ML_DAIS_LEVEL_S', 'DA4ML_DAIS_LEVEL_TPB', 'DA4ML_DAIS_TILE')


@pytest.fixture(scope='module')
def emu():
    r = subprocess.run(['make', '-s', '-C', str(EMU_DIR)], capture_output=True, text=True)
    assert r.returncode == 0 and EMU_LIB.exists(), r.stdout[-2000:] + r.stderr[-2000:]

    def run(what):
        env = {k: v for k, v in os.environ.items() if k not in KNOBS}
        env['DA4ML_HIP_LIB'] = str(EMU_LIB)
        out = subprocess.run([sys.executable, str(WORKER), what], env=env, capture_output=True, text=True, cwd=str(ROOT), timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    return run


def test_chains_in_both_value_files(emu):
    """9 random chains of 1, 2 and 3 stages, 700 samples, LDS file and global file; the library's own S (three workgroups: the largest
    tile, 16 samples, and a last tile of 12)"""
    r = emu('chains')
    assert r['bad'] == [] and r['n'] == 18 and r['s'] == [16]


def test_sample_counts_strides_and_types(emu):
    """1, 2, S - 1, S, S + 1 and 700 samples at S = 8, one sample in a tile of 16; an absent output at the boundary; rows inside wider
    arrays; the four element type pairs; a second run of a handle allocates nothing"""
    r = emu('counts')
    assert r['bad'] == [] and r['n'] == 12


def test_levels_wider_than_the_block_and_of_one_statement(emu):
    r = emu('wide')
    assert r['bad'] == [] and r['widths'] == [[2, 2500], [120, 1]]


def test_golden_vectors_and_table_fault(emu):
    r = emu('golden')
    assert r['bad'] == [] and r['n'] > 80
    assert len(r['faults']) == 4 and all(f.startswith('Logic lookup index out of bounds: index=') and f.endswith('table_size=4') for f in r['faults']), r['faults']
