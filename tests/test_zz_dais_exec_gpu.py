"""Compiled DAIS executables on the GPU (kernel k_dais_exec of csrc/dais_gpu.hip through da4ml_amd._binary.dais_compile): host arrays
staged in tiles and torch tensors that stay on the device, against the committed golden vectors and the stage-by-stage composition on
the host.  Like tests/test_zz_dais_gpu.py the file sorts after the solver's parity tests and every body runs in a child process, so that
a device fault fails one test, not the pytest process."""

import gzip
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _in_child(name: str):
    env_path = [str(ROOT), str(ROOT / 'tests')]
    # torch first: a torch build that ships its own ROCm runtime finds no device once the library has loaded the system's (README.md)
    code = f'import torch; import sys; sys.path[:0] = {env_path!r}; import test_zz_dais_exec_gpu as t; t.{name}(); print("child ok")'
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and 'child ok' in r.stdout, f'{name}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'


def test_golden_vectors_on_the_device():
    _in_child('body_golden_vectors')


def test_random_chains_equal_the_host_composition():
    _in_child('body_random_chains')


def test_solve_result_as_a_pipeline_on_device_tensors():
    _in_child('body_solve_pipeline')


def test_to_pipeline_split_equals_the_unsplit_stage():
    _in_child('body_split')


def test_one_handle_run_50_times():
    _in_child('body_stability')


def test_table_fault_in_resident_mode_raises():
    _in_child('body_table_fault')


def _resident(ex, x, **kw):
    import torch

    y = ex(torch.from_numpy(np.ascontiguousarray(x)).cuda(), **kw)
    return y.cpu().numpy()


def body_golden_vectors():
    from da4ml_amd._binary import dais_compile

    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'dais_golden.json.gz', 'rt'))
    for case in gold['cases']:
        prog = np.asarray(case['program'], dtype=np.int32)
        x = np.asarray([float.fromhex(v) for v in case['inputs']]).reshape(case['n_samples'], -1)
        want = np.asarray([float.fromhex(v) for v in case['outputs']]).reshape(case['n_samples'], -1)
        with dais_compile(prog) as ex:
            assert np.array_equal(ex(x, executor='device'), want), case['seed']
            assert np.array_equal(_resident(ex, x), want), case['seed']


def body_random_chains():
    """30 random 2-stage chains of 30 to 180 statements per stage, 700 samples (a partial last block), half of them far outside the declared
    input formats; staged in tiles of 256 and resident in one tile"""
    import os

    from dais_exec_cases import compose, random_chain

    from da4ml_amd._binary import dais_compile

    for seed in range(30):
        progs, x = random_chain(seed, 2, n_samples=700)
        assert all(30 <= int(p[4]) <= 180 for p in progs)
        want = compose(progs, x)
        with dais_compile(progs) as ex:
            os.environ['DA4ML_DAIS_TILE'] = '256'  # read at every run
            assert np.array_equal(ex(x, executor='device'), want), seed
            os.environ.pop('DA4ML_DAIS_TILE')
            assert np.array_equal(_resident(ex, x), want), seed


def body_solve_pipeline():
    """Two 64x64 solves as two-stage Pipelines in one executable each, 20 000 samples in torch tensors on the device: the int8 matrix of
    tests/test_zz_dais_gpu.py and a matrix of +-1 entries.  Both: equal to Pipeline.predict on the host (the stage-by-stage composition).
    The product x @ kernel is asserted for the +-1 matrix, whose first stage has neither a shifted nor a negated output (checked).  The
    first stage of the int8 matrix shifts outputs (out_shifts 0..7), and `solve` declares the second stage's input intervals from the first
    stage's result ops before that shift: its composition wraps at the boundary on the host too (types.Pipeline.compile), so for it the
    product is asserted for the first stage alone -- and for its to_pipeline split in body_split."""
    import torch
    from cases import int_matrix

    from da4ml_amd.cmvm import solve

    k = np.random.default_rng(0).choice([-1.0, 1.0], (64, 64)).astype(np.float32)
    exact = solve(k, method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
    assert set(exact.solutions[0].out_shifts) == {0} and not any(exact.solutions[0].out_negs)
    x = np.random.default_rng(0).integers(-128, 128, (20_000, 64)).astype(np.float64)
    xd = torch.from_numpy(x).cuda()
    want = exact.predict(x, executor='host')
    assert np.array_equal(want, x @ k.astype(np.float64))
    with exact.compile() as ex:
        assert np.array_equal(ex(xd).cpu().numpy(), want)
        assert np.array_equal(ex(xd.float(), out_dtype=torch.float32).cpu().numpy(), want.astype(np.float32))

    k = int_matrix(0, 64, 64, -128, 128)
    pipe = solve(k, method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
    want = pipe.predict(x, executor='host')
    assert np.array_equal(want, pipe.solutions[1].predict(pipe.solutions[0].predict(x)))
    with pipe.compile() as ex:
        assert ex.n_stages == 2
        y = ex(xd)
        assert y.is_cuda and y.dtype == torch.float64 and np.array_equal(y.cpu().numpy(), want)
        assert np.array_equal(ex(xd.float()).cpu().numpy(), want)  # float32 inputs: these integers are exact
        y32 = ex(xd.float(), out_dtype=torch.float32)
        assert y32.dtype == torch.float32 and np.array_equal(y32.cpu().numpy(), want.astype(np.float32))
        wide = torch.full((20_000, 100), float('nan'), dtype=torch.float64, device='cuda')
        wide[:, 7:71] = xd
        assert np.array_equal(ex(wide[:, 7:71]).cpu().numpy(), want)  # row stride 100 > n_in
        out = torch.full((20_000, 80), -7.0, dtype=torch.float64, device='cuda')
        got = ex(xd, out=out[:, 3:67])
        assert got.data_ptr() == out[:, 3:67].data_ptr() and np.array_equal(out[:, 3:67].cpu().numpy(), want)
        assert bool((out[:, :3] == -7.0).all()) and bool((out[:, 67:] == -7.0).all())
        side = torch.cuda.Stream()  # queued on a stream of the caller's
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ys = ex(xd)
        side.synchronize()
        assert np.array_equal(ys.cpu().numpy(), want)
        assert np.array_equal(ex(x, executor='device'), want)  # the same handle on host arrays
    stage0 = pipe.solutions[0]
    with stage0.compile() as ex0:
        assert np.array_equal(ex0(xd).cpu().numpy(), x @ stage0.kernel.astype(np.float64))
    assert np.array_equal(pipe.predict(xd[:1000], executor='device').cpu().numpy(), want[:1000])


def body_split():
    """a 3-stage to_pipeline split (no retiming) of the first stage of the 64x64 solve: inner boundaries with shift 0, no negation and the
    producer's interval, so the chain equals the unsplit stage's predict, and x @ kernel"""
    import torch
    from cases import int_matrix

    from da4ml_amd.cmvm import solve
    from da4ml_amd.trace import to_pipeline

    k = int_matrix(0, 64, 64, -128, 128)
    stage = solve(k, method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False).solutions[0]
    pipe = next(p for p in (to_pipeline(stage, cut, retiming=False, verbose=False) for cut in (3.0, 4.0, 3.5, 2.5, 5.0)) if len(p.solutions) == 3)
    for s in pipe.solutions[:-1]:
        assert set(s.out_shifts) == {0} and not any(s.out_negs)
    x = np.random.default_rng(1).integers(-128, 128, (20_000, 64)).astype(np.float64)
    want = stage.predict(x)
    with pipe.compile() as ex:
        assert ex.n_stages == 3
        y = ex(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(y, want)
    assert np.array_equal(y, pipe.predict(x, executor='host'))
    assert np.array_equal(y, x @ stage.kernel.astype(np.float64))


def body_stability():
    import torch
    from dais_exec_cases import compose, random_chain

    from da4ml_amd._binary import dais_compile

    progs, x = random_chain(5, 3, n_samples=5000)
    want = compose(progs, x)
    xd = torch.from_numpy(x).cuda()
    with dais_compile(progs) as ex:
        first = ex(xd)
        torch.cuda.synchronize()
        info = ex.info
        assert info['scratch_ptr'] != 0 and info['allocations'] == 1
        assert np.array_equal(first.cpu().numpy(), want)
        for _ in range(50):
            assert torch.equal(ex(xd), first)
        assert ex.info == info  # same scratch, no further allocation


def body_table_fault():
    import torch
    from dais_cases import random_program
    from dais_exec_cases import faulting_stage

    from da4ml_amd._binary import dais_compile

    p0, x = random_program(11, n_in=3, n_ops=40, n_out=2)
    with dais_compile([p0, faulting_stage(2)]) as ex:
        for _ in range(2):  # the handle stays usable and reports again
            with pytest.raises(RuntimeError, match=r'Logic lookup index out of bounds: index=\d+, table_size=4'):
                ex(torch.from_numpy(x).cuda())
        with pytest.raises(RuntimeError, match='Logic lookup index out of bounds'):
            ex(x, executor='device')
