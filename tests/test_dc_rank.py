"""entry_rank of da4ml_amd/csrc/cmvm_core.h with the latency-penalty weight as an argument, through tests/dc_rank/libdc_rank.so: with the named
constants it is the four-argument form bit for bit, and for any weight it is a float32 restatement in NumPy -- score = float(count) - w dl resp.
float(uint32 count * ov) - w dl, the multiply and the subtract rounded once each, then the order-preserving map of floats to ranks."""

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

DIR = Path(__file__).resolve().parent / 'dc_rank'
NAMES = ('mc', 'mc-dc', 'mc-pdc', 'wmc', 'wmc-dc', 'wmc-pdc', 'dummy')

_u32 = np.ctypeslib.ndpointer(np.uint32, flags='C_CONTIGUOUS')
_i32 = np.ctypeslib.ndpointer(np.int32, flags='C_CONTIGUOUS')
_f32 = np.ctypeslib.ndpointer(np.float32, flags='C_CONTIGUOUS')


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', str(DIR)], check=True)
    L = C.CDLL(str(DIR / 'libdc_rank.so'))
    L.dc_ranks4.argtypes = [_u32, _i32, _f32, _i32, C.c_longlong, _u32]
    L.dc_ranks5.argtypes = [_u32, _i32, _f32, _i32, _f32, C.c_longlong, _u32]
    for f in (L.dc_weight_mc, L.dc_weight_wmc, L.dc_weight_of):
        f.restype = C.c_float
    return L


def inputs(lib, seed, n):
    """counts from 0 (below 2: never selectable) to the u16 range and beyond, overlaps of both signs, latency differences that are integers,
    fractions, zero, tiny, huge, infinite and NaN; all seven methods"""
    rng = np.random.default_rng(seed)
    count = rng.choice([4, 64, 1 << 16, 1 << 26], n).astype(np.uint64)
    count = (rng.integers(0, 1 << 26, n).astype(np.uint64) % count).astype(np.uint32)
    ov = rng.integers(-20, 21, n).astype(np.int32)
    kind = rng.integers(0, 8, n)
    dl = np.where(kind < 3, rng.integers(0, 6, n), rng.random(n) * 10.0 ** rng.integers(-6, 7, n)).astype(np.float32)
    dl[kind == 6] = 0.0
    special = rng.random(n) < 0.01
    dl[special] = rng.choice(np.array([np.nan, np.inf, 1e-42, 3.4e38], np.float32), int(special.sum()))
    method = np.array([lib.dc_method_id(int(i)) for i in rng.integers(0, 7, n)], np.int32)
    return count, ov, dl, method


def ranks5(lib, count, ov, dl, method, w):
    out = np.zeros(len(count), np.uint32)
    lib.dc_ranks5(count, ov, dl, method, np.ascontiguousarray(w, np.float32), len(count), out)
    return out


def test_the_named_constants_are_the_reference_s(lib):
    assert lib.dc_weight_mc() == np.float32(1e9) and lib.dc_weight_wmc() == 256.0
    got = [lib.dc_weight_of(lib.dc_method_id(i)) for i in range(6)]
    assert got == [256.0, np.float32(1e9), np.float32(1e9), 256.0, 256.0, 256.0]  # (mc and wmc never read theirs)


def test_five_arguments_with_the_constants_equal_four(lib):
    count, ov, dl, method = inputs(lib, 1, 200_000)
    want = np.zeros(len(count), np.uint32)
    lib.dc_ranks4(count, ov, dl, method, len(count), want)
    w = np.array([lib.dc_weight_of(int(m)) for m in range(7)], np.float32)[np.searchsorted(np.arange(7), method)]
    assert np.array_equal(ranks5(lib, count, ov, dl, method, w), want)
    assert len(np.unique(want)) > 1000 and (want == 0).any()


def float_rank(s):
    """order-preserving float32 -> uint32, rank >= 1; -0 == +0; NaN -> 0 (cmvm_core.h)"""
    s = np.where(s == 0.0, np.float32(0.0), s).astype(np.float32)
    u = s.view(np.uint32)
    r = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return np.where(np.isnan(s), np.uint32(0), r)


def restated(lib, count, ov, dl, method, w):
    name = np.array([NAMES[[lib.dc_method_id(i) for i in range(7)].index(int(m))] for m in range(7)])[method]
    with np.errstate(all='ignore'):
        pen = (w.astype(np.float32) * dl.astype(np.float32)).astype(np.float32)  # one rounding
        s_mc = (count.astype(np.float32) - pen).astype(np.float32)  # and one more
        prod = (count.astype(np.uint64) * ov.astype(np.int64).astype(np.uint64)).astype(np.uint32)  # uint32 wrap for a negative overlap
        s_wmc = (prod.astype(np.float32) - pen).astype(np.float32)
    wmc = count.astype(np.int64) * ov
    out = np.zeros(len(count), np.uint32)
    out = np.where(name == 'mc', count + np.uint32(1), out)
    out = np.where(name == 'wmc', np.where(wmc >= 0, (wmc + 1).astype(np.uint32), 0), out)
    out = np.where(name == 'mc-pdc', float_rank(s_mc), out)
    out = np.where(name == 'mc-dc', np.where(s_mc >= 0, float_rank(s_mc), 0), out)  # (a NaN score compares false: dropped)
    out = np.where(name == 'wmc-pdc', float_rank(s_wmc), out)
    out = np.where(name == 'wmc-dc', np.where(s_wmc >= 0, float_rank(s_wmc), 0), out)
    return np.where(count < 2, 0, out).astype(np.uint32)


def test_any_weight_equals_the_float32_restatement(lib):
    count, ov, dl, method = inputs(lib, 2, 200_000)
    rng = np.random.default_rng(3)
    w = np.where(rng.random(len(count)) < 0.5, rng.choice(np.array([0, 0.3, 0.5, 0.75, 1, 2, 2.5, 3.3, 4, 256, 1e6, 1e9], np.float32), len(count)),
                 (rng.random(len(count)) * 10.0 ** rng.integers(-3, 10, len(count)))).astype(np.float32)  # fmt: skip
    got, want = ranks5(lib, count, ov, dl, method, w), restated(lib, count, ov, dl, method, w)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, [(int(count[i]), int(ov[i]), float(dl[i]), int(method[i]), float(w[i]), int(got[i]), int(want[i])) for i in bad[:5]]
    assert (count < 2).any() and (ov < 0).any() and np.isnan(dl).any()


def test_weight_zero_orders_as_the_selector_without_a_penalty(lib):
    """mc-pdc at weight 0 orders entries as mc does, whatever dl (counts below 2^24 are exact in float32)"""
    count, ov, dl, _ = inputs(lib, 4, 50_000)
    keep = ~np.isnan(dl) & ~np.isinf(dl)
    count, ov, dl = count[keep] % (1 << 24), ov[keep], dl[keep]
    m = lambda i: np.full(len(count), lib.dc_method_id(i), np.int32)  # noqa: E731
    zero = np.zeros(len(count), np.float32)
    a, b = ranks5(lib, count, ov, dl, m(2), zero), ranks5(lib, count, ov, dl, m(0), zero)
    order = np.argsort(count, kind='stable')
    assert np.array_equal(np.argsort(a, kind='stable'), np.argsort(b, kind='stable')) and (np.diff(a[order].astype(np.int64)) >= 0).all()
