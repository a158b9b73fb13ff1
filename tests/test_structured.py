"""The structured matrices (cases.STRUCTURED: all-ones, one value in every cell, duplicate / negated / doubled rows and columns,
ternary, rank 1, Toeplitz, zero checkerboards, one-hot rows) on the CPU: the records of the reference build
(tests/golden/structured_golden.json.gz, made by tests/golden/make_structured_golden.py with oracle/_ref/libref.so) describe
the families as cases.py builds them, and the restatement reproduces every one of them.  The GPU suite
(tests/test_structured_gpu.py) checks the HIP engine against the same records."""

import gzip
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from cases import STRUCTURED, STRUCTURED_OPTS, structured_matrix
from test_gpu_methods import digest

GOLD = {d['case']: d for d in json.load(gzip.open(Path(__file__).parent / 'golden' / 'structured_golden.json.gz', 'rt'))['digests']}


def test_grid_is_the_recorded_one():
    assert set(GOLD) == {f'{name}/{oname}' for name in STRUCTURED for oname in STRUCTURED_OPTS} and len(GOLD) == 100
    for name in STRUCTURED:
        k = structured_matrix(name)
        for oname, opts in STRUCTURED_OPTS.items():
            rec = GOLD[f'{name}/{oname}']
            assert rec['opts'] == opts and rec['shape'] == list(k.shape), rec['case']
            assert rec['kernel_sha256'] == hashlib.sha256(k.tobytes()).hexdigest(), rec['case']


def test_families_are_what_their_names_say():
    for small in (False, True):
        for name in STRUCTURED:
            k = structured_matrix(name, small)
            assert k.dtype == np.float32 and k.flags['C_CONTIGUOUS'] and np.array_equal(k, structured_matrix(name, small)), name
            assert not np.any(np.signbit(k) & (k == 0)), name  # no -0.0
    k = structured_matrix
    assert np.all(k('ones') == 1) and k('ones').shape == (64, 64) and np.all(k('ones_wide') == 1) and k('ones_wide').shape == (8, 300)
    assert k('ones_wide', small=True).shape[1] > 256  # the twin stays in the wide layout
    assert np.all(k('full85') == 85) and np.all(np.abs(k('full85_signs')) == 85) and k('full85_signs')[0, :2].tolist() == [85, -85]
    assert np.all(k('full_m128') == -128) and np.all(k('full_127') == 127) and np.all(k('full_0x555') == 0x555) and np.all(k('full_8191') == 8191)
    assert np.all(k('frac85') * 64 == 85)
    assert np.array_equal(k('diag'), 37 * np.eye(48, dtype=np.float32))
    assert np.linalg.matrix_rank(k('rank1').astype(np.float64)) == 1 and np.abs(k('rank1')).max() <= 64
    d = k('dup_rows')
    assert d.shape == (64, 48) and np.array_equal(d, np.tile(d[:4], (16, 1))) and len(np.unique(d[:4], axis=0)) == 4
    d = k('dup_cols')
    assert d.shape == (48, 64) and np.array_equal(d, np.tile(d[:, :4], (1, 16))) and len(np.unique(d[:, :4], axis=1).T) == 4
    d = k('neg_cols')
    assert np.array_equal(d[:, 16:32], -d[:, :16]) and np.array_equal(d[:, 32:], 2 * d[:, :16]) and np.abs(d[:, :16]).max() <= 64
    d = k('ternary_sparse')
    assert d.shape == (128, 128) and set(np.unique(d)) == {-1, 0, 1} and 0.87 < np.mean(d == 0) < 0.93
    assert set(np.unique(k('ternary_dense'))) == {-1, 1}
    assert set(np.unique(np.abs(k('pow2')))) == {1, 2, 4, 8, 16, 32, 64} and np.any(k('pow2') < 0)
    d = k('toeplitz')
    assert np.array_equal(d[1:, 1:], d[:-1, :-1]) and set(np.unique(d)) == {21 * v for v in range(-3, 4)}
    d = k('checker_zero')
    assert d[0, 0] == 51 and d[0, 1] == 0 and np.all((d == 51) | (d == 0)) and d.sum() == 51 * 512
    d = k('one_hot_rows')
    assert d.shape == (40, 16) and np.all((d != 0).sum(axis=1) == 1)


@pytest.mark.parametrize('name', STRUCTURED)
def test_restatement_matches_the_reference_records(oracle, name):
    """CPU: the restated oracle reproduces every record (0.01 - 3 s of CPU each)"""
    k = structured_matrix(name)
    for oname, opts in STRUCTURED_OPTS.items():
        rec = GOLD[f'{name}/{oname}']
        p = oracle.solve(k, **opts)
        assert digest(p) == rec['sha256'], rec['case']
        assert p.cost == rec['cost'] and [len(s.ops) for s in p.solutions] == rec['n_ops'], rec['case']
        assert np.all(p.kernel == k), rec['case']
