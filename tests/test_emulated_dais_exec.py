"""Kernel k_dais_exec of the compiled DAIS executables (csrc/dais_gpu.hip) on the emulated device of tests/test_emulated_device.py,
through tests/emu/dais_exec_worker.py: the chains of tests/test_dais_exec.py, several tiles, partial blocks.  The emulation checks indexing and logic of the kernel and
of the host code around it (tiles, staging with strides, scratch re-use), not its speed."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'dais_exec_worker.py'


@pytest.fixture(scope='module')
def emu():
    r = subprocess.run(['make', '-s', '-C', str(EMU_DIR)], capture_output=True, text=True)
    assert r.returncode == 0 and EMU_LIB.exists(), r.stdout[-2000:] + r.stderr[-2000:]

    def run(what):
        env = dict(os.environ, DA4ML_HIP_LIB=str(EMU_LIB))
        out = subprocess.run([sys.executable, str(WORKER), what], env=env, capture_output=True, text=True, cwd=str(ROOT), timeout=900)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(out.stdout.strip().splitlines()[-1])

    return run


def test_chains_in_tiles_of_256(emu):
    """12 random chains of 2 and 3 stages, 700 samples in tiles of 256 (two whole tiles, a partial one whose last block is partial); the
    register-file scratch is slots x tile x 8 bytes"""
    r = emu('chains')
    assert r['bad'] == [] and r['n'] == 12


def test_sample_counts_strides_and_types(emu):
    """1, 63, 64, 65 and 130 samples (less than, exactly and more than a wavefront); an absent output at the boundary; rows inside wider
    arrays; float32 in and out; a second run of a handle allocates nothing"""
    r = emu('counts')
    assert r['bad'] == [] and r['n'] == 5


def test_golden_vectors_and_table_fault(emu):
    r = emu('golden')
    assert r['bad'] == [] and r['n'] > 40
    assert len(r['faults']) == 2 and all(f.startswith('Logic lookup index out of bounds: index=') and f.endswith('table_size=4') for f in r['faults']), r['faults']
