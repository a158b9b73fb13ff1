"""The digit recoding a greedy chain starts from (digit_masks(x, mode, seed) of da4ml_amd/csrc/cmvm_core.h) through tests/recode/librecode.so,
against an independent restatement in NumPy written from the rule as the header states it: exhaustively for |x| < 2^16, all three modes, four
seeds.  Every mode keeps the value and the digit count, never raises the top position and keeps plus and minus disjoint; COMPACT leaves no
`s 0 -s` site; x and -x get mirrored digits; mode CSD is naf_masks."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from da4ml_amd.cmvm import splitmix64

DIR = Path(__file__).resolve().parent / 'recode'
CSD, COMPACT, SEEDED = 0, 1, 2
SEEDS = (0, 1, 0x9E3779B97F4A7C15, 0xFFFFFFFFFFFFFFFF)
LIMIT = 1 << 16
X = np.arange(-(LIMIT - 1), LIMIT, dtype=np.int32)

_u32 = np.ctypeslib.ndpointer(np.uint32, flags='C_CONTIGUOUS')
_i32 = np.ctypeslib.ndpointer(np.int32, flags='C_CONTIGUOUS')


@pytest.fixture(scope='module')
def rc():
    subprocess.run(['make', '-s', '-C', str(DIR)], check=True)
    lib = C.CDLL(str(DIR / 'librecode.so'))
    lib.rc_digit_masks.argtypes = [_i32, C.c_longlong, C.c_uint32, C.c_uint64, _u32, _u32]
    lib.rc_naf_masks.argtypes = [_i32, C.c_longlong, _u32, _u32]
    lib.rc_splitmix64.argtypes = [C.c_uint64]
    lib.rc_splitmix64.restype = C.c_uint64
    lib.rc_widths.argtypes = [_i32, C.c_longlong, _i32, _i32]
    return lib


def masks(rc, x, mode, seed):
    x = np.ascontiguousarray(x, np.int32)
    p, m = np.zeros(len(x), np.uint32), np.zeros(len(x), np.uint32)
    rc.rc_digit_masks(x, len(x), mode, seed, p, m)
    return p, m


def splitmix64_np(z):
    """SplitMix64 of an array of states (uint64 arithmetic wraps)"""
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def naf_digits(a, width):
    """non-adjacent form of the magnitudes `a`, least significant digit first: the textbook recurrence (digit = 2 - (a mod 4) for odd a)"""
    a = a.astype(np.int64).copy()
    d = np.zeros((len(a), width), np.int64)
    for p in range(width):
        odd = (a & 1) == 1
        d[:, p] = np.where(odd, 2 - (a & 3), 0)
        a = (a - d[:, p]) >> 1
    assert not a.any()
    return d


def restated(x, mode, seed):
    """the rule of the header on digit arrays: signed digits of every x, least significant first"""
    x = np.asarray(x, np.int64)
    a = np.abs(x)
    width = 18
    d = naf_digits(a, width)
    if mode != CSD:
        nz = d != 0
        top = np.where(nz.any(axis=1), width - 1 - np.argmax(nz[:, ::-1], axis=1), -1)
        key = np.uint64(splitmix64(seed))
        for p in range(width - 3, -1, -1):
            s = d[:, p + 2]
            site = (p + 2 <= top) & (s != 0) & (d[:, p + 1] == 0) & (d[:, p] == -s)
            if mode == SEEDED:
                coin = splitmix64_np(key ^ ((a.astype(np.uint64) << np.uint64(5)) | np.uint64(p))) >> np.uint64(63)
                site &= coin == 1
            d[site, p + 1] = s[site]
            d[site, p] = s[site]
            d[site, p + 2] = 0
    return d * np.sign(x)[:, None]  # x < 0: the mirrored digits of |x|


def to_digits(p, m, width=18):
    bits = np.arange(width, dtype=np.uint32)
    return ((p[:, None] >> bits) & 1).astype(np.int64) - ((m[:, None] >> bits) & 1).astype(np.int64)


def test_splitmix64_is_the_python_side(rc):
    for s in (*SEEDS, 12345, 1 << 63):
        assert rc.rc_splitmix64(s) == splitmix64(s)
    assert int(splitmix64_np(np.array([12345], np.uint64))[0]) == splitmix64(12345)


@pytest.mark.parametrize('mode', [CSD, COMPACT, SEEDED])
def test_digits_are_the_restatement_and_keep_value_count_and_top(rc, mode):
    """exhaustive below 2^16"""
    p0, m0 = masks(rc, X, CSD, 0)
    seen = set()
    for seed in SEEDS:
        p, m = masks(rc, X, mode, seed)
        d = to_digits(p, m)
        assert not (p >> 18).any() and not (m >> 18).any()
        assert np.array_equal(d, restated(X, mode, seed)), (mode, seed)
        assert not (p & m).any()  # disjoint
        assert np.array_equal((d * (1 << np.arange(18, dtype=np.int64))).sum(axis=1), X.astype(np.int64))  # the value
        assert np.array_equal(np.abs(d).sum(axis=1), np.abs(to_digits(p0, m0)).sum(axis=1))  # the digit count
        both = p | m
        # the top position: the highest set bit of the recoded digits is not above the NAF's
        hi = np.floor(np.log2(np.maximum(both, 1))).astype(int)
        hi0 = np.floor(np.log2(np.maximum(p0 | m0, 1))).astype(int)
        assert (hi <= hi0).all()
        # x and -x are mirrored (X is symmetric: reversing it negates it)
        assert np.array_equal(p[::-1], m) and np.array_equal(m[::-1], p)
        seen.add((p.tobytes(), m.tobytes()))
    assert len(seen) == (len(SEEDS) if mode == SEEDED else 1)  # the seed matters to SEEDED alone


def test_mode_csd_is_naf_masks(rc):
    x = np.concatenate([X, np.array([2**30, -(2**30), 2**31 - 1, -(2**31 - 1), 0x2AAAAAAA, 0x55555555, -0x55555555, 715827883], np.int32)])
    p0, m0 = np.zeros(len(x), np.uint32), np.zeros(len(x), np.uint32)
    rc.rc_naf_masks(np.ascontiguousarray(x), len(x), p0, m0)
    for seed in SEEDS:
        p, m = masks(rc, x, CSD, seed)
        assert np.array_equal(p, p0) and np.array_equal(m, m0)


def test_compact_leaves_no_site(rc):
    d = to_digits(*masks(rc, X, COMPACT, 0))
    for p in range(16):
        s = d[:, p + 2]
        assert not ((s != 0) & (d[:, p + 1] == 0) & (d[:, p] == -s)).any(), p


def test_known_vectors(rc):
    def terms(x, mode=COMPACT):
        p, m = masks(rc, [x], mode, 0)
        return sorted([1 << b for b in range(32) if (int(p[0]) >> b) & 1] + [-(1 << b) for b in range(32) if (int(m[0]) >> b) & 1], key=abs, reverse=True)

    assert terms(3) == [2, 1] and terms(3, CSD) == [4, -1]
    assert terms(-3) == [-2, -1]
    assert terms(11) == [8, 2, 1] and terms(11, CSD) == [16, -4, -1]  # 16 - 4 - 1 -> 8 + 4 - 1 -> 8 + 2 + 1: a site the first rewrite creates
    assert terms(7) == [8, -1] and terms(5) == [4, 1]  # no site
    assert terms(0) == []


def test_wide_values_keep_value_count_and_width(rc):
    """a sample of the whole range the engine takes (30 digits): value, digit count (naf_weight) and csd_width hold under every mode"""
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.integers(-(2**29), 2**29, 20000), np.array([2**29, -(2**29), 0x15555555, 0x2AAAAAAA // 2, 357913941, -357913941])]).astype(np.int32)
    w, n = np.zeros(len(x), np.int32), np.zeros(len(x), np.int32)
    rc.rc_widths(x, len(x), w, n)
    for mode in (CSD, COMPACT, SEEDED):
        for seed in SEEDS[1:3]:
            p, m = masks(rc, x, mode, seed)
            d = to_digits(p, m, 32)
            assert not (p & m).any()
            assert np.array_equal((d * (1 << np.arange(32, dtype=np.int64))).sum(axis=1), x.astype(np.int64))
            assert np.array_equal(np.abs(d).sum(axis=1), w)
            assert ((p | m).astype(np.uint64) < (np.uint64(1) << n.astype(np.uint64))).all()  # inside the csd_width of the value itself
