"""entry_rank_slack and slack_byte of da4ml_amd/csrc/cmvm_core.h through tests/slack_rank/libslack_rank.so, against a restatement in NumPy of the
definition in that header's comment: base = count (mc family) or the integer product count * ov (wmc family), discounted by
(base * ((byte * slack) >> 8)) >> 8 when 0 < base < 2^24, then entry_rank's float score, cut and order-preserving map."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

DIR = Path(__file__).resolve().parent / 'slack_rank'
NAMES = ('mc', 'mc-dc', 'mc-pdc', 'wmc', 'wmc-dc', 'wmc-pdc', 'dummy')

_u32 = np.ctypeslib.ndpointer(np.uint32, flags='C_CONTIGUOUS')
_i32 = np.ctypeslib.ndpointer(np.int32, flags='C_CONTIGUOUS')
_f32 = np.ctypeslib.ndpointer(np.float32, flags='C_CONTIGUOUS')


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', str(DIR)], check=True)
    L = C.CDLL(str(DIR / 'libslack_rank.so'))
    L.slk_ranks_plain.argtypes = [_u32, _i32, _f32, _i32, _f32, C.c_longlong, _u32]
    L.slk_ranks.argtypes = [_u32, _i32, _f32, _i32, _f32, _u32, _u32, C.c_longlong, _u32]
    L.slk_discount.argtypes = [_u32, _u32, _u32, C.c_longlong, _u32]
    L.slk_bytes.argtypes = [_u32, _u32, _i32, C.c_uint64, C.c_longlong, _u32]
    L.slk_bytes_by_word.argtypes = [_u32, _u32, _i32, C.c_uint64, C.c_longlong, _u32]
    return L


def method_ids(lib):
    return {name: lib.slk_method_id(i) for i, name in enumerate(NAMES)}


def inputs(lib, seed, n):
    """counts from 0 (below 2: never selectable) through the u16 range the device stores to beyond 2^24, overlaps of both signs, latency
    differences that are integers, fractions, zero, tiny, huge, infinite and NaN, weights from 0 to the mc constant; all seven methods"""
    rng = np.random.default_rng(seed)
    top = rng.choice([4, 64, 1 << 16, 1 << 26], n).astype(np.uint64)
    count = (rng.integers(0, 1 << 26, n).astype(np.uint64) % top).astype(np.uint32)
    ov = rng.integers(-20, 21, n).astype(np.int32)
    kind = rng.integers(0, 8, n)
    dl = np.where(kind < 3, rng.integers(0, 6, n), rng.random(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    dl[kind == 6] = 0.0
    special = rng.random(n) < 0.01
    dl[special] = rng.choice(np.array([np.nan, np.inf, 1e-42, 3.4e38], np.float32), int(special.sum()))
    method = np.array([lib.slk_method_id(int(i)) for i in rng.integers(0, 7, n)], np.int32)
    w = rng.choice(np.array([0.0, 0.5, 3.3, 256.0, 1e9], np.float32), n)
    return count, ov, dl, method, w


def ranks(lib, count, ov, dl, method, w, slack, byte):
    out = np.zeros(len(count), np.uint32)
    lib.slk_ranks(count, ov, dl, method, np.ascontiguousarray(w, np.float32), np.ascontiguousarray(slack, np.uint32), np.ascontiguousarray(byte, np.uint32), len(count), out)
    return out


def model_discount(base, slack, byte):
    """uint64 in, uint64 out: the definition, in arithmetic that cannot wrap"""
    base = base.astype(np.uint64)
    d = (byte.astype(np.uint64) * slack.astype(np.uint64)) >> np.uint64(8)
    cut = (base * d) >> np.uint64(8)
    return np.where((base > 0) & (base < (1 << 24)), base - cut, base)


def model_float_rank(s):
    s = s.astype(np.float32)
    u = np.where(s == 0, np.float32(0.0), s).view(np.uint32)
    r = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0), r).astype(np.uint32)


def model_ranks(ids, count, ov, dl, method, w, slack, byte):
    c64, o64 = count.astype(np.int64), ov.astype(np.int64)
    out = np.zeros(len(count), np.uint32)
    with np.errstate(all='ignore'):
        pen = (w.astype(np.float32) * dl.astype(np.float32)).astype(np.float32)
        # mc: the bare count
        m = method == ids['mc']
        out[m] = (model_discount(count, slack, byte)[m] + np.uint64(1)).astype(np.uint32)
        # wmc: the signed product; negative is not selectable
        m = method == ids['wmc']
        prod = c64 * o64
        disc = model_discount(np.where(prod >= 0, prod, 0).astype(np.uint64) & np.uint64(0xFFFFFFFF), slack, byte)
        out[m] = np.where(prod >= 0, (disc + np.uint64(1)) & np.uint64(0xFFFFFFFF), 0).astype(np.uint32)[m]
        for fam, base in (('mc', count.astype(np.uint64)), ('wmc', (c64 * o64).astype(np.uint64) & np.uint64(0xFFFFFFFF))):  # (the reference's unsigned wrap)
            b = model_discount(base, slack, byte)
            score = (b.astype(np.float32) - pen).astype(np.float32)
            r = model_float_rank(score)
            m = method == ids[fam + '-pdc']
            out[m] = r[m]
            m = method == ids[fam + '-dc']
            out[m] = np.where(score >= 0, r, 0)[m]
    out[count < 2] = 0
    return out


def test_slack_zero_is_entry_rank_bit_for_bit(lib):
    count, ov, dl, method, w = inputs(lib, 1, 300_000)
    plain = np.zeros(len(count), np.uint32)
    lib.slk_ranks_plain(count, ov, dl, method, w, len(count), plain)
    rng = np.random.default_rng(2)
    byte = rng.integers(0, 256, len(count)).astype(np.uint32)
    got = ranks(lib, count, ov, dl, method, w, np.zeros(len(count), np.uint32), byte)
    assert np.array_equal(got, plain)
    ids = method_ids(lib)
    for name in NAMES[:6]:
        assert (method == ids[name]).sum() > 10_000 and (plain[method == ids[name]] != 0).any(), name


def test_ranks_equal_the_numpy_restatement(lib):
    count, ov, dl, method, w = inputs(lib, 3, 300_000)
    rng = np.random.default_rng(4)
    slack = rng.integers(0, 256, len(count)).astype(np.uint32)
    byte = rng.integers(0, 256, len(count)).astype(np.uint32)
    got = ranks(lib, count, ov, dl, method, w, slack, byte)
    want = model_ranks(method_ids(lib), count, ov, dl, method, w, slack, byte)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(int(count[i]), int(ov[i]), float(dl[i]), int(method[i]), float(w[i]), int(slack[i]), int(byte[i]), int(got[i]), int(want[i])) for i in bad[:5]]
    plain = np.zeros(len(count), np.uint32)
    lib.slk_ranks_plain(count, ov, dl, method, w, len(count), plain)
    assert (got != plain).mean() > 0.2  # (the slack does move ranks)


def test_discount_bounds(lib):
    """a discount is at most slack / 256 of the base, a base >= 1 stays >= 1, bases from 2^24 on and 0 are left alone, 32-bit arithmetic suffices"""
    rng = np.random.default_rng(5)
    n = 400_000
    base = np.concatenate([np.arange(0, 4096, dtype=np.uint32), np.array([(1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0xFFFFFFFF, 0xFFFF0000], np.uint32),
                           rng.integers(0, 1 << 25, n).astype(np.uint32)])  # fmt: skip
    slack = rng.integers(0, 256, len(base)).astype(np.uint32)
    byte = rng.integers(0, 256, len(base)).astype(np.uint32)
    slack[:4096], byte[:4096] = 255, 255  # the largest discount on the small bases
    out = np.zeros(len(base), np.uint32)
    lib.slk_discount(base, slack, byte, len(base), out)
    assert np.array_equal(out.astype(np.uint64), model_discount(base, slack, byte))
    b, o = base.astype(np.int64), out.astype(np.int64)
    assert (o <= b).all() and ((b - o) * 256 <= b * slack.astype(np.int64)).all()
    assert (o[b >= 1] >= 1).all()
    untouched = (b == 0) | (b >= (1 << 24))
    assert np.array_equal(o[untouched], b[untouched])
    assert (b.astype(np.uint64) * ((byte.astype(np.uint64) * slack.astype(np.uint64)) >> np.uint64(8)))[~untouched].max() < (1 << 32)


@pytest.mark.parametrize('name', NAMES[:6])
def test_rank_is_non_decreasing_in_the_count(lib, name):
    """for every (overlap, latency difference, weight, slack, byte): count -> rank never steps down -- over the u16 range the device stores, and
    across 2^24, where the discount ends"""
    mid = method_ids(lib)[name]
    rng = np.random.default_rng(6)
    spans = [np.arange(0, 70_000, dtype=np.uint32), np.arange((1 << 24) - 3000, (1 << 24) + 3000, dtype=np.uint32)]
    for ov in (0, 1, 3, 7, 20) if name.startswith('wmc') else (1,):
        for dl, w in ((0.0, 256.0), (1.0, 3.3), (2.5, 256.0)):
            for slack, byte in ((255, 255), (16, 200), (3, 77), (int(rng.integers(1, 256)), int(rng.integers(0, 256)))):
                for count in spans:
                    n = len(count)
                    r = ranks(lib, count, np.full(n, ov, np.int32), np.full(n, dl, np.float32), np.full(n, mid, np.int32), np.full(n, w, np.float32),
                              np.full(n, slack, np.uint32), np.full(n, byte, np.uint32))  # fmt: skip
                    if name.endswith('-dc'):  # (the cut: not selectable below it, non-decreasing from the first selectable count on)
                        first = int(np.argmax(r != 0)) if (r != 0).any() else n
                        assert (r[:first] == 0).all()
                        r = r[first:]
                    assert (np.diff(r.astype(np.int64)) >= 0).all(), (name, ov, dl, w, slack, byte)


def test_byte_is_the_per_block_word_and_roughly_uniform(lib):
    """over a grid of row pairs and all keys of an 8-bit chain: every one of the 256 values occurs about equally often; another seed gives other bytes;
    the byte of a key is the one the kernels take from the block's word.
    Bounds: a uniform byte puts 45 150 / 256 = 176 pairs into a bin per key, standard deviation 13 (7.5 %): 40 % is more than five of them, for
    the 8 704 bins looked at; summed over the 34 keys a bin holds 5 996, standard deviation 77 (1.3 %): 8 % is six."""
    ids = np.arange(0, 300, dtype=np.uint32)
    id0, id1 = [a.ravel() for a in np.meshgrid(ids, ids, indexing='ij')]
    keep = id0 <= id1
    id0, id1 = np.ascontiguousarray(id0[keep]), np.ascontiguousarray(id1[keep])
    hist = np.zeros(256, np.int64)
    per_key = []
    for idx in range(0, 34):  # K = 2 (2 * 9 - 1) keys of 9 digit positions
        out, out2, other = (np.zeros(len(id0), np.uint32) for _ in range(3))
        lib.slk_bytes(id0, id1, np.full(len(id0), idx, np.int32), 0x9E3779B97F4A7C15, len(id0), out)
        lib.slk_bytes_by_word(id0, id1, np.full(len(id0), idx, np.int32), 0x9E3779B97F4A7C15, len(id0), out2)
        lib.slk_bytes(id0, id1, np.full(len(id0), idx, np.int32), 12345, len(id0), other)
        assert np.array_equal(out, out2) and out.max() <= 255
        assert 0.98 < (out != other).mean()
        h = np.bincount(out, minlength=256)
        assert h.min() > 0.6 * len(id0) / 256 and h.max() < 1.4 * len(id0) / 256, (idx, h.min(), h.max())
        hist += h
        per_key.append(out)
    n = hist.sum()
    assert hist.min() > 0.92 * n / 256 and hist.max() < 1.08 * n / 256
    # the keys of one block do not all share a byte, and two keys are not tied to each other
    per_key = np.array(per_key)
    assert (per_key.max(axis=0) != per_key.min(axis=0)).mean() > 0.999
    for a, b in ((0, 1), (1, 2), (0, 33), (16, 17)):
        assert abs(np.corrcoef(per_key[a].astype(float), per_key[b].astype(float))[0, 1]) < 0.05, (a, b)
