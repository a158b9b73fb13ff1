"""The level-parallel executor of compiled DAIS executables on the GPU (kernel k_dais_exec_level of csrc/dais_gpu.hip, mode='level'): the
value file in the workgroup's LDS and, under DA4ML_DAIS_LEVEL_LDS=0, in global memory, against mode='sample', the committed golden vectors
and the stage-by-stage composition on the host.  Like tests/test_zz_dais_exec_gpu.py every body runs in a child process, so that a device
fault fails one test, not the pytest process.  Nothing here measures time."""

import gzip
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KNOBS = ('DA4ML_DAIS_MODE', 'DA4ML_DAIS_LEVEL_LDS', 'DA4ML_DAIS_LEVEL_S', 'DA4ML_DAIS_LEVEL_TPB', 'DA4ML_DAIS_TILE')
FILES = (('level-lds', None), ('level-global', '0'))


def _in_child(name: str):
    env_path = [str(ROOT), str(ROOT / 'tests')]
    # torch first: a torch build that ships its own ROCm runtime finds no device once the library has loaded the system's (README.md)
    code = f'import torch; import sys; sys.path[:0] = {env_path!r}; import test_zz_dais_level_gpu as t; t.{name}(); print("child ok")'
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and 'child ok' in r.stdout, f'{name}: rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}'


def test_golden_vectors_in_level_mode():
    _in_child('body_golden_vectors')


def test_random_chains_level_equals_sample_equals_host():
    _in_child('body_random_chains')


def test_solve_result_on_device_tensors():
    _in_child('body_solve_stage')


def test_to_pipeline_split_equals_the_unsplit_stage():
    _in_child('body_split')


def test_one_handle_run_50_times_allocates_once():
    _in_child('body_stability')


def test_table_fault_in_resident_level_mode_raises():
    _in_child('body_table_fault')


def test_info_reports_the_mode_and_file_that_ran():
    _in_child('body_info')


def _file(lds):
    """DA4ML_DAIS_LEVEL_LDS is read at every run"""
    if lds is None:
        os.environ.pop('DA4ML_DAIS_LEVEL_LDS', None)
    else:
        os.environ['DA4ML_DAIS_LEVEL_LDS'] = lds


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
            for file, lds in FILES:
                _file(lds)
                assert np.array_equal(_resident(ex, x, mode='level'), want) and ex.info['last_run'] == file, (case['seed'], file)
            assert np.array_equal(ex(x, executor='device', mode='level'), want), case['seed']


def body_random_chains():
    """random 2- and 3-stage chains, half of the samples far outside the declared input formats, at 1, 63, 64, 65 and 700 rows: level (LDS
    file and global file) == sample == the host composition"""
    from dais_exec_cases import compose, random_chain

    from da4ml_amd._binary import dais_compile

    for seed in range(6):
        progs, x = random_chain(seed, 2 + seed % 2, n_samples=700)
        want = compose(progs, x)
        with dais_compile(progs) as ex:
            for n in (1, 63, 64, 65, 700):
                assert np.array_equal(_resident(ex, x[:n], mode='sample'), want[:n]) and ex.info['last_run'] == 'sample', (seed, n)
                for file, lds in FILES:
                    _file(lds)
                    assert np.array_equal(_resident(ex, x[:n], mode='level'), want[:n]) and ex.info['last_run'] == file, (seed, n, file)
                _file(None)
            assert np.array_equal(ex(x, executor='device', mode='level'), want), seed  # staged host arrays


def _stage64():
    from cases import int_matrix

    from da4ml_amd.cmvm import solve

    return solve(int_matrix(0, 64, 64, -128, 128), method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False).solutions[0]


def body_solve_stage():
    """the first stage of a 64x64 solve, 1 000 rows in torch tensors on the device, in place inside wider tensors: level == sample == host
    == x @ kernel, float64 and float32"""
    import torch

    stage = _stage64()
    x = np.random.default_rng(0).integers(-128, 128, (1000, 64)).astype(np.float64)
    want = stage.predict(x, executor='host')
    assert np.array_equal(want, x @ stage.kernel.astype(np.float64))
    with stage.compile() as ex:
        for file, lds in FILES:
            _file(lds)
            for dtype in (torch.float64, torch.float32):
                wide = torch.full((1000, 100), float('nan'), dtype=dtype, device='cuda')
                wide[:, 7:71] = torch.from_numpy(x).cuda().to(dtype)
                out = torch.full((1000, 80), -7.0, dtype=dtype, device='cuda')
                got = ex(wide[:, 7:71], out=out[:, 3:67], mode='level')
                assert got.data_ptr() == out[:, 3:67].data_ptr() and ex.info['last_run'] == file
                assert np.array_equal(out[:, 3:67].cpu().numpy(), want.astype(np.float32 if dtype == torch.float32 else np.float64)), (file, dtype)
                assert bool((out[:, :3] == -7.0).all()) and bool((out[:, 67:] == -7.0).all())
                assert torch.equal(ex(wide[:, 7:71], out_dtype=dtype, mode='sample'), got)
        _file(None)
        xd = torch.from_numpy(x).cuda()
        assert np.array_equal(ex(xd).cpu().numpy(), want) and ex.info['last_run'] == 'level-lds'  # AUTO: 4 955 statements, 1 000 rows
        os.environ['DA4ML_DAIS_MODE'] = 'sample'
        assert np.array_equal(ex(xd).cpu().numpy(), want) and ex.info['last_run'] == 'sample'
        os.environ.pop('DA4ML_DAIS_MODE')
        _file(None)


def body_split():
    """a 3-stage to_pipeline split (no retiming) of that stage as one chain in level mode == the unsplit stage in level mode == x @ kernel"""
    from da4ml_amd.trace import to_pipeline

    stage = _stage64()
    pipe = next(p for p in (to_pipeline(stage, cut, retiming=False, verbose=False) for cut in (3.0, 4.0, 3.5, 2.5, 5.0)) if len(p.solutions) == 3)
    x = np.random.default_rng(1).integers(-128, 128, (1000, 64)).astype(np.float64)
    with stage.compile() as ex:
        want = _resident(ex, x, mode='level')
    assert np.array_equal(want, x @ stage.kernel.astype(np.float64))
    with pipe.compile() as ex:
        assert ex.n_stages == 3
        for file, lds in FILES:
            _file(lds)
            assert np.array_equal(_resident(ex, x, mode='level'), want) and ex.info['last_run'] == file, file
        _file(None)


def body_stability():
    import torch
    from dais_exec_cases import compose, random_chain

    from da4ml_amd._binary import dais_compile

    progs, x = random_chain(5, 3, n_samples=5000)
    want = compose(progs, x)
    xd = torch.from_numpy(x).cuda()
    for file, lds in FILES:
        _file(lds)
        with dais_compile(progs) as ex:
            first = ex(xd, mode='level')
            torch.cuda.synchronize()
            info = ex.info
            assert info['last_run'] == file and info['allocations'] == (0 if file == 'level-lds' else 1), info
            assert np.array_equal(first.cpu().numpy(), want)
            for _ in range(50):
                assert torch.equal(ex(xd, mode='level'), first)
            assert ex.info == info  # no further allocation
    _file(None)


def body_table_fault():
    import torch
    from dais_cases import random_program
    from dais_exec_cases import faulting_stage

    from da4ml_amd._binary import dais_compile

    p0, x = random_program(11, n_in=3, n_ops=40, n_out=2)
    with dais_compile([p0, faulting_stage(2)]) as ex:
        for file, lds in FILES:
            _file(lds)
            for _ in range(2):  # the handle stays usable and reports again
                with pytest.raises(RuntimeError, match=r'Logic lookup index out of bounds: index=\d+, table_size=4'):
                    ex(torch.from_numpy(x).cuda(), mode='level')
        _file(None)


def body_info():
    from dais_exec_cases import random_chain

    from da4ml_amd._binary import dais_compile

    progs, x = random_chain(2, 2, n_samples=300)
    with dais_compile(progs) as ex:
        assert ex.info['last_run'] == 'none' and ex.info['level_S'] == 0
        a = _resident(ex, x, mode='sample')
        assert ex.info['last_run'] == 'sample'
        b = _resident(ex, x, mode='level')
        info = ex.info
        assert info['last_run'] == 'level-lds' and info['level_S'] >= 1 and info['level_S'] & (info['level_S'] - 1) == 0
        _file('0')
        c = ex(x, executor='device', mode='level')
        assert ex.info['last_run'] == 'level-global'
        _file(None)
        os.environ['DA4ML_DAIS_MODE'] = 'level'  # decides for 'auto', leaves an explicit mode alone
        d = _resident(ex, x)
        assert ex.info['last_run'] == 'level-lds'
        _resident(ex, x, mode='sample')
        assert ex.info['last_run'] == 'sample'
        os.environ.pop('DA4ML_DAIS_MODE')
        _resident(ex, x)  # AUTO: a chain this small is outside the measured region of the level kernel
        assert ex.info['last_run'] == 'sample'
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
        assert info['n_levels'] > 1 and info['level_width'] >= 1 and info['level_slots'] >= 1
