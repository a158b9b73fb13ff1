"""GPU parity on STRUCTURED matrices (cases.STRUCTURED at their medium sizes): what quantised layer weights look like, and what a
random int8 matrix barely visits -- every row pair of the table tied at step 0 (all-ones), every column substituted in every step
(8x300 all-ones), overlapping occurrences of one pair (85 = 0b1010101 in every cell), duplicate / negated / doubled rows and columns,
rows that empty out, chains of 7 and of 2 400 steps in one lockstep batch.  The pick is then decided by the tie-break alone: here by
the hash table's incremental counts, the "pick known one step ahead" comparison and the arg-max over group bounds, in the reference
by the scan order of a regenerated table.  All comparisons are exact.  The checker is the reference build, live
(conftest.reference_oracle), and its committed records (tests/golden/structured_golden.json.gz); tests/test_structured.py pins
the restatement to the same records on the CPU, tests/test_emulated_device.py runs the small twins through the emulated kernels."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from cases import SINGLE_CHAIN, STRUCTURED, STRUCTURED_OPTS, samples_inside, structured_matrix
from test_gpu_methods import digest
from test_structured import GOLD

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def hip():
    from da4ml_amd import _binary

    assert _binary.device_count() >= 1, 'no HIP device visible: the GPU tests must run on the MI355X box'
    return _binary


@pytest.fixture(scope='module')
def solved(hip):
    """hip.solve of (family at medium size, option set), once per module; prints the capacity retries of the solve (reported, not asserted)"""
    done = {}

    def get(name, oname):
        if (name, oname) not in done:
            before = hip.timings()['retries']
            done[name, oname] = hip.solve(structured_matrix(name), **STRUCTURED_OPTS[oname])
            print(f'[structured] {name}/{oname}: capacity retries {int(hip.timings()["retries"] - before)}')
        return done[name, oname]

    return get


@pytest.mark.parametrize('oname', STRUCTURED_OPTS)
@pytest.mark.parametrize('name', STRUCTURED)
def test_parity(solved, reference_oracle, name, oname):
    """the complete result equals the live checker's and the committed record of the reference build"""
    k, rec = structured_matrix(name), GOLD[f'{name}/{oname}']
    got = solved(name, oname)
    assert got == reference_oracle.solve(k, **STRUCTURED_OPTS[oname])
    assert digest(got) == rec['sha256']
    assert got.cost == rec['cost'] and [len(s.ops) for s in got.solutions] == rec['n_ops']
    assert np.all(got.kernel == k)


@pytest.mark.parametrize('name', STRUCTURED)
def test_function_against_plain_arithmetic(solved, name):
    """Independent of any oracle: the solution computes x @ k exactly.  |x| <= 128, |k| < 2^13 and at most 128 terms keep every
    product and sum far below 2^53, and frac85 is dyadic, so float64 is exact.

    The host executor wraps every value into the format of its op's interval, and the intervals a solution declares are the
    reference's: the input ops carry the interval of the input times 2^inp_shifts, and stage 1 declares the intervals of stage 0's
    result ops BEFORE their output shifts and signs (reference api.cc:100-113).  Stage 0's output therefore lies outside what stage
    1 declares wherever a column has a common power of two (full_8191: 2^13), and feeding one executor's output to the other wraps.
    So: (1) the two stages in plain float64 arithmetic, stage 0 into stage 1, on 256 int8 vectors equal x @ k; (2) the host
    executor of EACH stage equals samples @ stage.kernel on 256 vectors drawn from all of its declared input range, and stage
    0's executor output times stage 1's matrix equals x @ k"""
    k = structured_matrix(name)
    k64 = k.astype(np.float64)
    rng = np.random.default_rng(1)
    x = rng.integers(-128, 128, (256, k.shape[0])).astype(np.float64)
    for oname in ('single', 'default'):
        p = solved(name, oname)
        stage0, stage1 = p.solutions
        assert np.array_equal(stage1(stage0(x)), x @ k64), oname
        for stage in (stage0, stage1):
            xs = samples_inside(stage, rng, 256)
            assert np.array_equal(stage.predict(xs), xs @ stage.kernel.astype(np.float64)), oname
        x0 = samples_inside(stage0, rng, 256)
        assert np.array_equal(stage0.predict(x0) @ stage1.kernel.astype(np.float64), x0 @ k64), oname
        if name == 'frac85':
            assert np.array_equal(stage1(stage0(x)), x @ k) and np.array_equal(stage0.predict(x0) @ stage1.kernel.astype(np.float64), x0 @ k), oname


def test_one_batch(hip, solved):
    """all medium families as ONE batch of single chains: both layouts, 7 to about 2 400 steps per chain, lockstep groups that
    lose members early -- element by element the single solves; then the same batch listed in reverse order"""
    ks = [structured_matrix(name) for name in STRUCTURED]
    for order in (1, -1):
        before = hip.timings()['retries']
        got = hip.solve_many(ks[::order], **SINGLE_CHAIN)[::order]
        print(f'[structured] batch order {order}: capacity retries {int(hip.timings()["retries"] - before)}')
        for name, g in zip(STRUCTURED, got):
            assert g == solved(name, 'single'), (name, order)
            assert digest(g) == GOLD[f'{name}/single']['sha256'], (name, order)


def test_determinism_under_ties(hip, reference_oracle):
    """a tie decided by the store order between wavefronts would show as a run that differs: 30 repetitions of small all-tied
    problems, alternating between single calls and one batch, and between the single chain and the default search"""
    ks = [structured_matrix('ones', shape=(16, 16)), structured_matrix('full85', shape=(16, 16)), structured_matrix('ternary_dense', shape=(24, 24))]
    modes = [(batched, opts) for opts in (SINGLE_CHAIN, {}) for batched in (False, True)]
    want = [[reference_oracle.solve(k, **opts) for k in ks] for _, opts in modes]
    for rep in range(30):
        batched, opts = modes[rep % 4]
        got = hip.solve_many(ks, **opts) if batched else [hip.solve(k, **opts) for k in ks]
        for i, (g, w) in enumerate(zip(got, want[rep % 4])):
            assert g == w, f'repetition {rep}, case {i} ({"batch" if batched else "single call"}, {opts})'


FORCED = r'''
import json, os, sys
sys.path.insert(0, os.environ["DA_ROOT"]); sys.path.insert(0, os.path.join(os.environ["DA_ROOT"], "tests"))
from cases import STRUCTURED_OPTS, structured_matrix
from da4ml_amd import _binary as hip
from test_gpu_methods import digest
k = structured_matrix(sys.argv[1])
out = {}
for oname in ("single", "default"):
    p = hip.solve(k, **STRUCTURED_OPTS[oname])
    out[oname] = dict(sha256=digest(p), cost=p.cost, n_ops=[len(s.ops) for s in p.solutions])
tm = hip.timings()
print(json.dumps(dict(out, table_bytes=tm["table_bytes"], retries=tm["retries"])), flush=True)
'''


@pytest.mark.parametrize('name', ['ones', 'full85'])
def test_forced_large_tables(name):
    """DA4ML_HIP_TABLE_SCALE chosen, with the product's own sizing rule (tests/geometry), to give the family's chain 2048 groups: the
    tie then spans every group bound of the selection's arg-max -- same records"""
    from test_table_geometry import MAX_GROUPS, load_geo, scale_for_groups

    scale = scale_for_groups(load_geo(), name, MAX_GROUPS)
    env = dict(os.environ, DA_ROOT=str(ROOT), DA4ML_HIP_TABLE_SCALE=repr(scale))
    r = subprocess.run([sys.executable, '-c', FORCED, name], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(f'[structured] {name} with table scale {scale}: capacity retries {int(out["retries"])}, table bytes {out["table_bytes"]:.0f}')
    for oname in ('single', 'default'):
        rec = GOLD[f'{name}/{oname}']
        assert out[oname] == dict(sha256=rec['sha256'], cost=rec['cost'], n_ops=rec['n_ops']), oname
