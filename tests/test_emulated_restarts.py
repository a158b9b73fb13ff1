"""Seeded random restarts of the greedy search (da4ml_amd.cmvm.solve_restarts, `seeds=` of _binary.solve_many, da_solve_batch_seeded) with the
product's kernels on the emulated device of tests/test_emulated_device.py, through tests/emu/restart_worker.py.

A restart changes the tie word of a chain and nothing else, so every restart is a greedy run of the reference's method: it must give a graph
that implements the matrix, restart 0 (seed 0) must be the reference's result, and the same seed must give the same graph whatever else runs
beside it.  What a mistake in the kernels looks like here: a site that forms a tie word the reference's way in a seeded chain gives picks that are
still valid graphs -- but which pick wins then depends on where a block lies in the table and on which of the two ways a step finds its pick.  The
emulated build runs candidate lists of two entries, so both ways run all the time, and the `maximal picks` test moves every block by changing the
table's size."""

import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EMU_DIR = ROOT / 'tests' / 'emu'
EMU_LIB = EMU_DIR / 'libda4ml_emu.so'
WORKER = EMU_DIR / 'restart_worker.py'


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
def validity(emu):
    """the 40 option sets, R = 4 each, in four worker processes side by side"""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(4) as pool:
        return list(pool.map(lambda b: emu('validity', 10 * b, 10 * b + 10), range(4)))


def test_every_restart_is_a_valid_graph_and_restart_0_the_reference_result(validity):
    """40 random option sets (cases.random_case; every fourth one without intervals of its own on a matrix of up to 16x16), four restarts each:
    every restart's Pipeline.kernel equals the matrix, its cost the float32 sum of its ops in op order, restart 0 equals the oracle's result, the
    winner is the first strict minimum and costs no more than the oracle's"""
    assert [r['bad'] for r in validity] == [[], [], [], []]
    assert sum(r['n'] for r in validity) == 40


def test_the_option_sets_cover_what_they_should(validity):
    assert set().union(*(r['methods'] for r in validity)) == {'mc', 'mc-dc', 'mc-pdc', 'wmc', 'wmc-dc', 'wmc-pdc'}
    assert set().union(*(map(bool, r['cost_models']) for r in validity)) == {False, True}  # adder count only / the latency-aware model
    assert {0, 1, 2, 3} <= set().union(*(r['hard_dc'] for r in validity))
    assert sum(r['custom'] for r in validity) >= 10  # custom intervals and latencies
    assert max(tuple(r['largest']) for r in validity) == (16, 16)
    assert sum(r['differing'] for r in validity) >= 20  # the restarts are not all the same graph


def check_repro(r, manycol):
    for layout in ('narrow', 'wide'):
        assert r['again'][layout] == r['alone'][layout], layout  # the same seeds twice
        assert r['one_by_one'][layout] == r['alone'][layout], layout  # every restart in a call of its own
        assert r['mixed'][layout] == r['alone'][layout], layout  # inside a larger batch: other position, other widths and seeds beside it
        assert len(set(r['alone'][layout])) > 1, layout
    assert [r['alone']['narrow'][0], r['alone']['wide'][0]] == r['plain']  # restart 0 is solve()
    assert (r['manycol'] > 0) == manycol


def test_same_seed_same_result_alone_and_in_a_mixed_batch(emu):
    """narrow entries (9x10) and wide ones (4x260: more than 256 columns); seeded and unseeded chains of both widths in one batch: all four
    of {narrow, wide} x {reference order, seeded} run side by side, each over its own range of the sorted descriptors"""
    check_repro(emu('repro'), manycol=False)


def test_same_seed_same_result_many_column_carve(emu):
    """the same under DA4ML_HIP_MANYCOL_FROM=1: k_iter_select2<Cell, false, MANYCOL, SEEDED>"""
    check_repro(emu('repro', env=dict(DA4ML_HIP_MANYCOL_FROM='1')), manycol=True)


@pytest.fixture(scope='module')
def fixed_plain(emu):
    return emu('fixed', 4, 5)


def test_seeds_matter(emu):
    """the fixed 16x16 int8 wmc matrix (restart_worker.FIXED): eight restarts, eight different op lists on the emulated device"""
    r = emu('fixed', 8, 1)
    assert r['kernel_ok'] and r['distinct_op_lists'] >= 2
    assert r['costs'][r['best']] <= r['costs'][0] and r['best'] == min(range(8), key=lambda i: (r['costs'][i], i))


@pytest.mark.parametrize('scale', ['4', '0.5'])
def test_picks_are_maximal_whatever_the_table_geometry(emu, fixed_plain, scale):
    """the same seeded chains with a table four times / half the size: other slots, other groups, blocks met in another order -- the op lists must
    not move.  A tie word formed inconsistently at one site shows here"""
    r = emu('fixed', 4, 5, env=dict(DA4ML_HIP_TABLE_SCALE=scale))
    assert r['digests'] == fixed_plain['digests'] and r['kernel_ok'] and r['retries'] == 0
    assert len(set(fixed_plain['digests'])) == 4


def test_the_seed_survives_a_capacity_retry(emu, fixed_plain):
    r = emu('fixed', 4, 5, env=dict(DA4ML_HIP_TABLE_SCALE='0.02', DA4ML_HIP_ROW_SCALE='0.05'))
    assert r['retries'] >= 1 and r['digests'] == fixed_plain['digests'] and r['kernel_ok']


@pytest.mark.parametrize('world', [2, 3])
def test_restarts_sharded_over_gloo_ranks(emu, tmp_path, world):
    """multi_gpu.solve_restarts_sharded: restart r on rank r % world, each rank its own emulated device; every rank returns the Pipeline of the
    one-process solve_restarts (a single chain, a default search, the latency-aware cost model; 5, 4 and 7 restarts)"""
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    res = tmp_path / 'rank0.json'
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   DA4ML_HIP_LIB=str(EMU_LIB), DA4ML_HIP_UPD_BLOCKS='8', EMU_OUT=str(res), DA4ML_PIN_RANKS='0')  # fmt: skip
        procs.append(subprocess.Popen([sys.executable, str(WORKER), 'sharded_rank'], env=env, cwd=str(ROOT), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    want = emu('sharded_want')
    for p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    assert json.loads(res.read_text()) == want
