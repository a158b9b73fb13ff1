"""The newest-row-first tie order of a seeded chain (tie_word(id0, id1, idx, seed, order) with TIE_ORDER_NEWEST, da4ml_amd/csrc/cmvm_core.h)
through tests/tie_newest/libtie_newest.so: a strict total order for every seed, below 2^55, the larger id1 always wins, the rows of an entry
come back from its word over the whole id range, inside a block the order of (idx ^ k7) -- and the order argument changes nothing that was:
order 0 is the four-argument word, seed 0 the reference's word under both orders."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

DIR = Path(__file__).resolve().parent / 'tie_newest'
SEEDS = (1, 2, 0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15, 0x0123456789ABCDEF, 0xFE00000000000001, 12345)  # those of test_tie_order.py
RANDOM, NEWEST = 0, 1
M24 = (1 << 24) - 1

_u32 = np.ctypeslib.ndpointer(np.uint32, flags='C_CONTIGUOUS')
_i32 = np.ctypeslib.ndpointer(np.int32, flags='C_CONTIGUOUS')
_u64 = np.ctypeslib.ndpointer(np.uint64, flags='C_CONTIGUOUS')


@pytest.fixture(scope='module')
def tn():
    subprocess.run(['make', '-s', '-C', str(DIR)], check=True)
    lib = C.CDLL(str(DIR / 'libtie_newest.so'))
    lib.tn_words.argtypes = [_u32, _u32, _i32, C.c_longlong, C.c_uint64, C.c_uint32, _u64]
    lib.tn_words_newest.argtypes = [_u32, _u32, _i32, C.c_longlong, C.c_uint64, _u64]
    lib.tn_words4.argtypes = [_u32, _u32, _i32, C.c_longlong, C.c_uint64, _u64]
    lib.tn_decode.argtypes = [_u64, C.c_longlong, C.c_uint64, C.c_uint32, _u32, _u32, _i32]
    lib.tn_mix24.argtypes = [_u32, C.c_longlong, C.c_uint64, _u32, _u32]
    lib.tn_exhaustive.argtypes = [C.c_uint32, C.c_int, C.c_uint64, C.c_uint32, _u64]
    return lib


def words(tn, id0, id1, idx, seed, order):
    id0, id1, idx = np.ascontiguousarray(id0, np.uint32), np.ascontiguousarray(id1, np.uint32), np.ascontiguousarray(idx, np.int32)
    out = np.zeros(len(id0), np.uint64)
    tn.tn_words(id0, id1, idx, len(id0), seed, order, out)
    return out


def sample(seed, n):
    """entries of the whole domain: ids below 2^24 (small ids, as chains have them, and the largest ones among them), idx below 128"""
    rng = np.random.default_rng(seed)
    top = rng.choice([64, 4096, 1 << 16, 1 << 24], n)
    id0 = (rng.integers(0, 1 << 24, n) % top).astype(np.uint32)
    id1 = (rng.integers(0, 1 << 24, n) % top).astype(np.uint32)
    id0[:4], id1[:4] = [M24, 0, M24, 0], [M24, M24, 0, 0]
    return id0, id1, rng.integers(0, 128, n).astype(np.int32)


def mix24_py(id0, seed):
    """the specification, in Python integers"""
    h = id0 ^ (seed & M24)
    h = (h * 0x9E3779B97F4B) & M24
    h ^= h >> 12
    return h ^ ((seed >> 24) & M24)


@pytest.mark.parametrize('seed', SEEDS)
def test_newest_word_is_injective_on_the_exhaustive_small_domain(tn, seed):
    out = np.zeros(5, np.uint64)
    tn.tn_exhaustive(64, 128, seed, NEWEST, out)
    assert int(out[0]) == int(out[1]) == 64 * 64 * 128
    assert int(out[2]) < 1 << 55
    assert int(out[3]) == 0  # rows and key index come back from every word
    assert int(out[4]) == 0  # the run-time-order expression is id1 << 31 | mix24(id0) << 7 | (idx ^ k7)


@pytest.mark.parametrize('seed', SEEDS + (0,))
def test_the_order_argument_leaves_the_random_order_and_seed_0_what_they_were(tn, seed):
    out = np.zeros(5, np.uint64)
    tn.tn_exhaustive(48, 128, seed, RANDOM, out)
    assert int(out[0]) == int(out[1]) and int(out[3]) == 0 and int(out[4]) == 0  # tie_word_seeded, resp. the reference's word
    id0, id1, idx = sample(seed & 0xFFFF, 100_000)
    ref = (id1.astype(np.uint64) << np.uint64(31)) | (id0.astype(np.uint64) << np.uint64(7)) | idx.astype(np.uint64)
    if seed == 0:
        assert np.array_equal(words(tn, id0, id1, idx, 0, RANDOM), ref) and np.array_equal(words(tn, id0, id1, idx, 0, NEWEST), ref)
    old = np.zeros(len(id0), np.uint64)
    tn.tn_words4(id0, id1, idx, len(id0), seed, old)  # the four-argument word, untouched
    assert np.array_equal(words(tn, id0, id1, idx, seed, RANDOM), old)
    r0, r1, ri = np.zeros_like(id0), np.zeros_like(id1), np.zeros_like(idx)
    tn.tn_decode(old, len(old), seed, RANDOM, r0, r1, ri)
    assert np.array_equal(r0, id0) and np.array_equal(r1, id1) and np.array_equal(ri, idx)


@pytest.mark.parametrize('seed', SEEDS)
def test_newest_word_over_the_whole_domain(tn, seed):
    """samples with ids up to 2^24 - 1: the specification's bits, below 2^55, injective, decode round trip"""
    id0, id1, idx = sample(seed & 0xFFFF, 400_000)
    w = words(tn, id0, id1, idx, seed, NEWEST)
    k7 = seed >> 57
    want = [(int(b) << 31) | (mix24_py(int(a), seed) << 7) | (int(k) ^ k7) for a, b, k in zip(id0[:20_000], id1[:20_000], idx[:20_000])]
    assert w[:20_000].tolist() == want
    spelled = np.zeros_like(w)
    tn.tn_words_newest(id0, id1, idx, len(w), seed, spelled)
    assert np.array_equal(w, spelled)
    assert int(w.max()) < 1 << 55
    triple = (id1.astype(np.uint64) << np.uint64(31)) | (id0.astype(np.uint64) << np.uint64(7)) | idx.astype(np.uint64)
    assert len(np.unique(w)) == len(np.unique(triple))
    r0, r1, ri = np.zeros_like(id0), np.zeros_like(id1), np.zeros_like(idx)
    tn.tn_decode(w, len(w), seed, NEWEST, r0, r1, ri)
    assert np.array_equal(r0, id0) and np.array_equal(r1, id1) and np.array_equal(ri, idx)


@pytest.mark.parametrize('seed', SEEDS)
def test_mix24_is_a_bijection_of_24_bits_with_unmix24_its_inverse(tn, seed):
    ids = np.arange(1 << 24, dtype=np.uint32)  # every id there is
    mixed, back = np.zeros_like(ids), np.zeros_like(ids)
    tn.tn_mix24(ids, len(ids), seed, mixed, back)
    assert np.array_equal(back, ids) and int(mixed.max()) <= M24
    assert np.array_equal(np.bincount(mixed, minlength=1 << 24), np.ones(1 << 24, np.int64))
    assert mixed[:1000].tolist() == [mix24_py(i, seed) for i in range(1000)]


@pytest.mark.parametrize('seed', SEEDS)
def test_the_newer_id1_wins_whatever_id0_idx_and_the_seed(tn, seed):
    rng = np.random.default_rng(seed & 0xFFFF)
    n = 300_000
    a0, a1, ai = sample((seed & 0xFFFF) + 1, n)
    b0, b1, bi = sample((seed & 0xFFFF) + 2, n)
    a1[:2], b1[:2], a0[:2], b0[:2], ai[:2], bi[:2] = [0, M24 - 1], [1, M24], [M24, M24], [0, 0], [127, 127], [0, 0]  # neighbours at both ends, everything else against them
    near = rng.integers(0, 2, n).astype(bool)
    b1 = np.where(near, np.minimum(a1.astype(np.int64) + 1, M24), b1).astype(np.uint32)
    wa, wb = words(tn, a0, a1, ai, seed, NEWEST), words(tn, b0, b1, bi, seed, NEWEST)
    lt, gt = a1 < b1, a1 > b1
    assert lt.sum() > n // 4
    assert np.all(wa[lt] < wb[lt]) and np.all(wa[gt] > wb[gt])
    assert np.array_equal(wa >> np.uint64(31), a1.astype(np.uint64))  # id1 sits in the word as it is: bound words (word >> 23) hold it whole
    # ... which the random order does not give (it is what this order is for)
    ra, rb = words(tn, a0, a1, ai, seed, RANDOM), words(tn, b0, b1, bi, seed, RANDOM)
    assert not np.all(ra[lt] < rb[lt])


@pytest.mark.parametrize('seed', SEEDS)
def test_order_inside_a_block_is_the_order_of_idx_xor_k7(tn, seed):
    k7 = seed >> 57
    idx = np.arange(128, dtype=np.int32)
    for id0, id1 in ((0, 0), (3, 17), (255, 256), (70000, 70001), (M24, M24)):
        w = words(tn, np.full(128, id0), np.full(128, id1), idx, seed, NEWEST)
        assert np.array_equal(w & np.uint64(0x7F), (idx ^ k7).astype(np.uint64))
        assert np.array_equal(np.argsort(w), np.argsort(idx ^ k7))
        assert len(set((w >> np.uint64(7)).tolist())) == 1  # one row pair, one high part


def test_seeds_give_different_orders_below_id1(tn):
    id0, idx = np.arange(2000, dtype=np.uint32) % 500, (np.arange(2000) // 500).astype(np.int32)  # 500 pairs of one id1, four keys each
    id1 = np.full(2000, 777, np.uint32)
    orders = {tuple(np.argsort(words(tn, id0, id1, idx, s, NEWEST), kind='stable').tolist()) for s in SEEDS}
    assert len(orders) == len(SEEDS)
