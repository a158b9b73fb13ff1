"""Stage 1's spanning tree (spanning_tree, da4ml_amd/csrc/cmvm_host.cc) keeps the cheapest edge of every vertex outside the tree -- V^2 edge
costs -- where the reference scans all (outside, inside) pairs in every step and keeps the first strict minimum (V^3 / 6).  It must find the
same edges in the same order also where many edges cost the same and where the depth cap (dc >= 0) blocks edges.  Compared here: the
product's host code behind the sequential model (tests/model, no device) with the oracle's restatement of the reference's scan
(oracle/cmvm_oracle.cc, prim_mst), on matrices made of ties: few distinct values, duplicate, negated, doubled and zero columns."""

import numpy as np
import pytest


def tie_heavy(seed):
    rng = np.random.default_rng(seed)
    n_in, n_out = int(rng.integers(1, 7)), int(rng.integers(2, 41))
    hi = int(rng.choice([1, 2, 4, 64]))
    k = rng.integers(-hi, hi + 1, (n_in, n_out)).astype(np.float32)
    for _ in range(int(rng.integers(0, n_out))):  # columns that equal, negate or double another one: distances 0 and equal distances
        a, b = rng.integers(0, n_out, 2)
        k[:, a] = k[:, b] * float(rng.choice([1, -1, 2]))
    if seed % 3 == 0:
        k[:, rng.integers(0, n_out)] = 0
    return np.ascontiguousarray(k)


@pytest.mark.parametrize('block', range(4))
def test_same_decomposition_as_the_scan_of_all_pairs(oracle, model, block):
    bad = []
    for seed in range(block * 50, block * 50 + 50):
        k = tie_heavy(seed)
        for dc in (-1, 0, 1, 2, 3, 5):
            got, want = model.kernel_decompose(k, dc), oracle.kernel_decompose(k, dc)
            if not all(np.array_equal(g, w) for g, w in zip(got, want)):
                bad.append((seed, dc))
    assert bad == []


def test_a_wide_all_equal_matrix(oracle, model):
    """300 equal columns: every edge costs 0, the order of the vertices decides everything"""
    k = np.ones((2, 300), np.float32)
    for dc in (0, 2):
        got, want = model.kernel_decompose(k, dc), oracle.kernel_decompose(k, dc)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
