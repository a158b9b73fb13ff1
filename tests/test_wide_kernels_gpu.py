"""Kernels of up to 4095 output columns.  Chains whose regular carve of the selection kernel's substitution block does not fit beside the
kernel's static LDS (120 816 bytes are left: about 3300 columns and more) run its many-column form, k_iter_select2<Cell, false, MANYCOL> (B's list worked on where it
lies in memory, 16-bit per-column arrays); k_iter_update gets more than 64 KB of dynamic LDS from about 2800 columns on.  The default search
needs the width twice: stage 2 of a decompose_dc >= 0 candidate is an n_out x n_out chain.

  * DA4ML_HIP_MANYCOL_FROM=1 forces the many-column form for every chain: small problems, checked against the reference's own sources run live
    and against the same solve without the knob;
  * the real widths 2560 columns (regular carve) and 3400 and 4095 columns (many-column carve) against records of the reference build (tests/golden/make_wide_golden.py: it spends 14 s to
    3.3 minutes on each);
  * a batch that mixes the carves; the width the row-reference format cannot hold."""

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from cases import int_matrix, random_case

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / 'golden'
SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
N_RANDOM = 40


@pytest.fixture(scope='module')
def oracle(reference_oracle):
    return reference_oracle


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


def digest(p):
    dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))
    return hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest()


def small_cases():
    """name -> (kernel, options): what runs under the forced many-column form"""
    cases = {}
    for seed in range(N_RANDOM):
        k, opts, _ = random_case(seed)
        cases[f'random_{seed}'] = (k, opts)
    cases['4x257_single_chain'] = (int_matrix(5, 4, 257, -2, 2), SINGLE)  # the narrowest chain of the wide layout
    cases['6x1100_single_chain'] = (int_matrix(1, 6, 1100, -8, 8), SINGLE)  # lists longer than a block of the selection kernel has threads: chunked passes
    cases['6x1100_default'] = (int_matrix(1, 6, 1100, -8, 8), {})
    return cases


SUB = (
    "import sys, json, hashlib\nsys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
    "from test_wide_kernels_gpu import small_cases, digest\nfrom da4ml_amd import _binary as hip\n"
    "got = {name: digest(hip.solve(k, **opts)) for name, (k, opts) in small_cases().items()}\ntm = hip.timings()\n"
    "print(json.dumps({'digests': got, 'chains': tm['chains'], 'manycol_chains': tm['manycol_chains']}))\n"
)


def solve_small_cases(**env):
    """all of small_cases() in one fresh process (the knob is read when the backend is created): the digests, and how many of the chains
    that went to the device ran the many-column instantiation"""
    e = {k: v for k, v in os.environ.items() if k != 'DA4ML_HIP_MANYCOL_FROM'}
    e.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, '-c', SUB], env=e, capture_output=True, text=True, cwd=str(ROOT), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope='module')
def forced_run():
    return solve_small_cases(DA4ML_HIP_MANYCOL_FROM=1)


@pytest.fixture(scope='module')
def regular_run():
    return solve_small_cases()


@pytest.fixture(scope='module')
def forced(forced_run):
    return forced_run['digests']


@pytest.fixture(scope='module')
def regular(regular_run):
    return regular_run['digests']


def test_the_knob_decides_the_instantiation(forced_run, regular_run):
    """every chain of the forced run went through k_iter_select2<Cell, false, true>, none of the regular run (no case here is wide enough)"""
    assert forced_run['chains'] > 0 and forced_run['manycol_chains'] == forced_run['chains']
    assert regular_run['chains'] == forced_run['chains'] and regular_run['manycol_chains'] == 0


@pytest.fixture(scope='module')
def want(oracle):
    return {name: digest(oracle.solve(k, **opts)) for name, (k, opts) in small_cases().items()}


def test_forced_manycol_random_option_sets_against_oracle(forced, want):
    names = [f'random_{s}' for s in range(N_RANDOM)]
    assert [n for n in names if forced[n] != want[n]] == []


@pytest.mark.parametrize('name', ['4x257_single_chain', '6x1100_single_chain', '6x1100_default'])
def test_forced_manycol_wide_layout_against_oracle(forced, want, name):
    assert forced[name] == want[name]


def test_forced_manycol_equals_the_regular_carve(forced, regular):
    assert set(forced) == set(regular) == set(small_cases())
    assert [n for n in forced if forced[n] != regular[n]] == []


@pytest.mark.parametrize('name,manycol', [('2x2560_int4_seed1_single_chain', False), ('2x2560_int4_seed1_default', False), ('2x2560_int8_seed1_single_chain', False),
                                          ('2x3400_int4_seed1_single_chain', True), ('3x4095_int4_seed1_single_chain', True), ('2x4095_int4_seed3_default', True)])  # fmt: skip
def test_real_width_against_reference_record(hip, name, manycol):
    """2560 columns: still the regular carve (it fits up to about 3300 columns), k_iter_update close to its 64 KB; 3400 columns: the many-column
    carve because nothing else fits, k_iter_update with 78 KB of dynamic LDS; 4095 columns: 93 KB, one block per CU.  The default searches
    solve n_out x n_out chains in stage 2 (4095 x 4095: 268 MB of dense row lists, 8.4 M row pairs)"""
    rec = json.loads((GOLDEN / 'wide_golden.json').read_text())[name]
    k = int_matrix(*rec['matrix'])
    hip.timings(reset=True)
    p = hip.solve(k, **rec['opts'])
    tm = hip.timings()
    assert (p.kernel == k).all()
    assert p.cost == rec['cost'] and [len(s.ops) for s in p.solutions] == rec['n_ops'] and digest(p) == rec['sha256']
    assert tm['chains'] > 0 and tm['manycol_chains'] == (tm['chains'] if manycol else 0)


def test_mixed_batch_of_regular_and_manycol_chains(hip):
    """narrow, wide with the regular carve (257 and 2560 columns) and wide with the many-column carve (3400 columns) in one call"""
    ks = [int_matrix(4, 64, 64, -128, 128), int_matrix(1, 2, 2560, -8, 8), int_matrix(5, 4, 257, -2, 2), int_matrix(1, 2, 3400, -8, 8)]
    hip.timings(reset=True)
    batch = hip.solve_many(ks, **SINGLE)
    assert hip.timings()['manycol_chains'] == 1
    for k, p in zip(ks, batch):
        assert p == hip.solve(k, **SINGLE)
        assert (p.kernel == k).all()


def test_4096_columns_are_refused(hip):
    """the row-reference format holds list lengths below 4096 (REF_LEN_BITS = 12)"""
    with pytest.raises(RuntimeError):
        hip.solve(int_matrix(0, 2, 4096, -8, 8))
