"""Geometry of a chain's pair table (da4ml_amd/csrc/cmvm_geometry.h, the one function HipBackend::run_chains and the column-sharded
chain size their tables with), through tests/geometry/libgeometry.so: the shapes that ran before keep their geometry bit for bit, the
tall kernels beyond 748 input rows get one, and the capped tables hold the blocks the sequential engine model counts."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from cases import STRUCTURED, int_matrix, structured_matrix

GEO_DIR = Path(__file__).resolve().parent / 'geometry'
MAX_GROUPS = 2048  # DA_MAX_GROUPS of the product build
M_WMC, M_DUMMY = 3, 6
LOAD_FACTOR = 0.5  # 1 / TABLE_SLOTS_PER_PAIR


def load_geo():
    subprocess.run(['make', '-s', '-C', str(GEO_DIR)], check=True)
    lib = C.CDLL(str(GEO_DIR / 'libgeometry.so'))
    lib.geo_table.argtypes = [C.c_int, C.c_int, C.c_int, C.c_longlong, C.c_longlong, C.c_double, C.c_double, C.c_int, np.ctypeslib.ndpointer(np.int64)]

    def run(n_in, n_out, pairs, digits, table_scale=1.0, row_scale=1.0, method=M_WMC):
        out = np.zeros(4, np.int64)
        lib.geo_table(n_in, n_out, method, pairs, digits, table_scale, row_scale, MAX_GROUPS, out)
        return dict(C=int(out[0]), gs_log2=int(out[1]), n_groups=int(out[2]), rcap=int(out[3]))

    return run


@pytest.fixture(scope='module')
def geo():
    return load_geo()


def naf_weight(x):
    a = np.abs(x.astype(np.int64))
    d = ((3 * a) ^ a) >> 1
    return np.array([bin(int(v)).count('1') for v in d.ravel()]).reshape(x.shape)


def prep(k):
    """k_prepare's digit statistics of an integer matrix: digits, and row pairs of digits per column (centring shifts by powers of two
    leave the NAF weights as they are)"""
    d = naf_weight(k).sum(axis=0)
    return int((d * (d - 1) // 2).sum()), int(d.sum())


def heuristic_geometry(n_in, pairs, digits, table_scale=1.0, method=M_WMC):
    """the sizing rule as it stood for the tables it accepted (at most 2^25 slots)"""
    pairs0 = min(n_in * (n_in + 1) // 2, max(pairs, 1))
    want = max(1024.0, 0.8 * pairs0 * max(4.0, n_in / 5.0) * table_scale)
    if method == M_DUMMY:
        want = 64
    c = 1
    while c < int(want):
        c <<= 1
    gs = 8
    while (c >> gs) > MAX_GROUPS:
        gs += 1
    assert gs <= 14, 'not a shape that ran before'
    c = max(c, 256)
    return dict(C=c, gs_log2=gs, n_groups=c >> gs)


def strip(g):
    return {k: g[k] for k in ('C', 'gs_log2', 'n_groups')}


SQUARE = [(n, lo) for n in (16, 32, 64, 96, 128, 192, 256, 384, 512, 640) for lo in (-8, -128)]
C5 = [(16, 64), (64, 64), (64, 32), (32, 8)]  # bench.py C5_LAYERS


@pytest.mark.parametrize('n,lo', SQUARE)
def test_square_shapes_keep_their_geometry(geo, n, lo):
    k = int_matrix(n, n, n, lo, -lo)
    pairs, digits = prep(k)
    assert strip(geo(n, n, pairs, digits)) == heuristic_geometry(n, pairs, digits)


def test_c3_chain_geometry(geo):
    """BASELINE C3, 256x256 int8: 2^21 slots in groups of 2^10"""
    for seed in range(4):
        pairs, digits = prep(int_matrix(seed, 256, 256, -128, 128))
        assert strip(geo(256, 256, pairs, digits)) == dict(C=1 << 21, gs_log2=10, n_groups=2048)


@pytest.mark.parametrize('shape', C5)
def test_c5_layer_geometry(geo, shape):
    for seed in range(3):
        k = int_matrix(seed, *shape, -8, 8)
        pairs, digits = prep(k)
        for ts in (1.0, 0.02, 4.0, 16.0):
            assert strip(geo(*shape, pairs, digits, table_scale=ts)) == heuristic_geometry(shape[0], pairs, digits, ts)
    assert strip(geo(16, 64, 0, 0, method=M_DUMMY)) == heuristic_geometry(16, 0, 0, method=M_DUMMY)


def test_capacity_retries_of_shapes_that_ran_keep_their_geometry(geo):
    """the retry multiplies both scales by 4: as long as the heuristic stays within 2^25 slots nothing changes"""
    pairs, digits = prep(int_matrix(0, 128, 128, -128, 128))
    for ts in (0.02, 0.08, 0.32, 1.0, 4.0, 16.0, 64.0):
        want = heuristic_geometry(128, pairs, digits, ts)
        assert strip(geo(128, 128, pairs, digits, table_scale=ts, row_scale=ts)) == want


@pytest.mark.parametrize('shape', [(768, 1, -128), (1024, 16, -8), (2048, 64, -128), (1024, 64, -128), (2048, 1, -8), (749, 749, -128)])
def test_tall_kernels_get_a_geometry(geo, shape):
    n_in, n_out, lo = shape
    pairs, digits = prep(int_matrix(1, n_in, n_out, lo, -lo))
    g = geo(n_in, n_out, pairs, digits)
    assert 256 <= g['C'] <= 1 << 30 and g['C'] & (g['C'] - 1) == 0
    assert g['n_groups'] <= MAX_GROUPS and g['C'] == g['n_groups'] << g['gs_log2'] and g['gs_log2'] <= 19
    # rows for every step a chain can take (each removes a digit); never fewer slots than blocks the chain can hold -- row pairs that
    # share a column -- at the load factor, unless the heuristic asked for fewer or the table is at its limit
    assert g['rcap'] == n_in + digits + 1
    blocks = min(g['rcap'] * (g['rcap'] + 1) // 2, pairs + digits)
    assert g['C'] >= min(blocks / LOAD_FACTOR + 2 * g['rcap'], 1 << 30, heuristic_want(n_in, pairs))
    # retries grow it, up to 2^30 slots, and never raise
    for ts in (4.0, 16.0, 64.0, 256.0):
        h = geo(n_in, n_out, pairs, digits, table_scale=ts, row_scale=ts)
        assert g['C'] <= h['C'] <= 1 << 30


def heuristic_want(n_in, pairs, table_scale=1.0):
    pairs0 = min(n_in * (n_in + 1) // 2, max(pairs, 1))
    return max(1024.0, 0.8 * pairs0 * max(4.0, n_in / 5.0) * table_scale)


def test_tall_narrow_tables_are_capped(geo):
    """1024x1 int4: ~1M blocks at most against the heuristic's 2^27 slots"""
    pairs, digits = prep(int_matrix(1, 1024, 1, -8, 8))
    assert heuristic_want(1024, pairs) > 1 << 26
    g = geo(1024, 1, pairs, digits)
    assert g['C'] <= 1 << 22


def test_table_scale_forces_large_groups(geo):
    """DA4ML_HIP_TABLE_SCALE reaches groups of 2^15 and 2^16 slots on the recorded 128x128 / 256x256 matrices (tests/test_tall_kernels_gpu.py)"""
    for n, scales in ((128, (200, 400)), (256, (25, 50))):
        pairs, digits = prep(int_matrix(0, n, n, -128, 128))
        assert [geo(n, n, pairs, digits, table_scale=s)['gs_log2'] for s in scales] == [15, 16]


@pytest.mark.parametrize('shape', [(256, 1, -128), (512, 1, -8), (384, 2, -128), (768, 1, -128), (512, 4, -8), (1024, 1, -8)])
def test_capped_tables_hold_the_model_peak(geo, model, shape):
    """the sequential engine model's exact peak of live blocks, over the load factor, fits the table the chain gets (with the tables
    of these shapes capped as if their heuristic had asked for more than 2^25 slots: table_scale 1e4)"""
    n_in, n_out, lo = shape
    k = int_matrix(1, n_in, n_out, lo, -lo)
    lib = model.lib
    lib.mdl_stats.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.int64)]
    h = model.g('solve')(k, n_in, n_out, b'wmc', b'wmc', -1, -1, None, None, -1, -1, 0)
    assert h, model.g('last_error')().decode()
    st = np.zeros(8, np.int64)
    lib.mdl_stats(h, st)
    model.g('free')(h)
    peak, iterations = int(st[4]), int(st[0])
    pairs, digits = prep(k)
    for ts in (1.0, 1e4):
        g = geo(n_in, n_out, pairs, digits, table_scale=ts)
        assert g['C'] >= peak / LOAD_FACTOR
    capped = geo(n_in, n_out, pairs, digits, table_scale=1e4)
    assert heuristic_want(n_in, pairs, 1e4) > 1 << 25 and capped['C'] < heuristic_want(n_in, pairs, 1e4)
    assert capped['rcap'] > n_in + iterations  # (no row-capacity retry)


def structured_prep(name):
    """prep of a structured family at its medium size (frac85: scaled to integers by a power of two, which leaves the digits as they are)"""
    k = structured_matrix(name)
    while np.any(k != np.round(k)):
        k = k * 2
    return k, *prep(k)


@pytest.mark.parametrize('name', STRUCTURED)
def test_structured_families_get_a_geometry(geo, name):
    """the pair statistics of the structured matrices sit at the extremes of the sizing rule (all-ones: every row pair in every column;
    one-hot rows and the diagonal: no pair across rows at all) -- each gets a power-of-two table in at most 2048 groups"""
    k, pairs, digits = structured_prep(name)
    n_in, n_out = k.shape
    if name in ('ones', 'ones_wide'):
        assert pairs == n_out * (n_in * (n_in - 1) // 2) and digits == n_in * n_out
    if name in ('diag', 'one_hot_rows'):
        assert digits == int(naf_weight(k).sum()) and pairs == sum(w * (w - 1) // 2 for w in naf_weight(k).sum(axis=0))
    for ts in (1.0, 4.0, 16.0):  # as sized, and after one and two capacity retries
        g = geo(n_in, n_out, pairs, digits, table_scale=ts, row_scale=ts)
        assert g['C'] >= 256 and g['C'] & (g['C'] - 1) == 0, (ts, g)
        assert 1 <= g['n_groups'] <= MAX_GROUPS and g['C'] == g['n_groups'] << g['gs_log2'] and g['gs_log2'] >= 8, (ts, g)
        assert g['rcap'] > n_in


@pytest.mark.parametrize('name', ['ones', 'full85', 'dup_rows', 'ternary_dense'])
def test_structured_tables_hold_the_model_peak(geo, model, name):
    """the sequential engine model's exact peak of live blocks of a single wmc chain, over the load factor, fits the table the
    chain gets without a capacity retry -- at the all-ones extreme of the pair count and on duplicate rows as on random matrices"""
    k, pairs, digits = structured_prep(name)
    n_in, n_out = k.shape
    lib = model.lib
    lib.mdl_stats.argtypes = [C.c_void_p, np.ctypeslib.ndpointer(np.int64)]
    h = model.g('solve')(k, n_in, n_out, b'wmc', b'wmc', -1, -1, None, None, -1, -1, 0)
    assert h, model.g('last_error')().decode()
    st = np.zeros(8, np.int64)
    lib.mdl_stats(h, st)
    model.g('free')(h)
    peak, iterations = int(st[4]), int(st[0])
    g = geo(n_in, n_out, pairs, digits)
    print(f'{name}: pairs {pairs} digits {digits} peak {peak} iterations {iterations} geometry {g}')
    assert peak > 0 and iterations > 0
    assert g['C'] >= peak / LOAD_FACTOR


def scale_for_groups(geo, name, groups):
    """the smallest power-of-two DA4ML_HIP_TABLE_SCALE at which the single chain of a structured family gets `groups` table groups"""
    k, pairs, digits = structured_prep(name)
    for e in range(0, 16):
        if geo(*k.shape, pairs, digits, table_scale=float(2**e))['n_groups'] == groups:
            return float(2**e)
    raise AssertionError(f'no table scale gives {name} {groups} groups')


def test_table_scale_forces_all_groups_on_the_tied_families(geo):
    """tests/test_structured_gpu.py solves `ones` and `full85` with the scale found here: 2048 groups of 256 slots, every group bound of
    the selection's arg-max in use, where the chains get 128 and 64 groups as sized"""
    for name, groups, scale in (('ones', 128, 16.0), ('full85', 64, 32.0)):
        k, pairs, digits = structured_prep(name)
        assert geo(*k.shape, pairs, digits)['n_groups'] == groups
        assert scale_for_groups(geo, name, MAX_GROUPS) == scale
        assert strip(geo(*k.shape, pairs, digits, table_scale=scale)) == dict(C=1 << 19, gs_log2=8, n_groups=MAX_GROUPS)
