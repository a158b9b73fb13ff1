"""Worker of tests/test_emulated_dais_level.py (DA4ML_HIP_LIB = tests/emu/libda4ml_emu.so: kernel k_dais_exec_level on the CPU, thread by
thread, three workgroups in the persistent grid): chains through executor='device', mode='level' -- staged host arrays, the only memory
the emulated device has -- against the stage-by-stage composition on the host.  The knobs DA4ML_DAIS_LEVEL_LDS / _S / _TPB are read at
every run.  One JSON line on stdout.
usage: dais_level_worker.py <what>"""

import gzip
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
from dais_cases import random_program  # noqa: E402
from dais_exec_cases import compose, faulting_stage, random_chain, with_absent_output  # noqa: E402

from da4ml_amd._binary import dais_compile  # noqa: E402

FILES = (('level-lds', None), ('level-global', '0'))


def knobs(lds=None, s=None, tpb=None):
    for name, v in (('DA4ML_DAIS_LEVEL_LDS', lds), ('DA4ML_DAIS_LEVEL_S', s), ('DA4ML_DAIS_LEVEL_TPB', tpb)):
        if v is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = str(v)


def level(ex, x, file, **kw):
    """one level-mode run; the handle must report the value file that was asked for"""
    got = ex(x, executor='device', mode='level', **kw)
    assert ex.info['last_run'] == file, (ex.info, file)
    return got


def chains():
    """random chains of 1, 2 and 3 stages, 700 samples, both value files, S chosen by the library; blocks of 1024 and of 128 lanes"""
    bad, n, seen_s = [], 0, set()
    for seed in range(9):
        progs, x = random_chain(seed, 1 + seed % 3, n_samples=700)
        want = compose(progs, x)
        with dais_compile(progs) as ex:
            for file, lds in FILES:
                knobs(lds=lds, tpb=(None, 128)[seed % 2])
                n += 1
                if not np.array_equal(level(ex, x, file), want):
                    bad.append([seed, file])
                seen_s.add(ex.info['level_S'])
            knobs()
            if not np.array_equal(ex(x, executor='device', mode='sample'), want) or ex.info['last_run'] != 'sample':
                bad.append([seed, 'sample', ex.info['last_run']])
    return dict(bad=bad, n=n, s=sorted(seen_s))


def counts():
    """1, 2, S - 1, S, S + 1 and 700 samples at S = 8 (forced) in both files, a tile of 16 for one sample (n < S); an absent output at the
    boundary; rows inside wider arrays; the four element type pairs; a second run of a handle allocates nothing"""
    bad, n = [], 0
    progs, x = random_chain(3, 2, n_samples=700)
    progs[0] = with_absent_output(progs[0], 1)
    want = compose(progs, x)
    n_in, n_out = x.shape[1], want.shape[1]
    x32 = x.astype(np.float32)
    want32 = compose(progs, x32.astype(np.float64))
    with dais_compile(progs) as ex:
        for file, lds in FILES:
            knobs(lds=lds, s=8, tpb=256)
            for m in (1, 2, 7, 8, 9, 700):
                n += 1
                if not np.array_equal(level(ex, x[:m], file), want[:m]) or ex.info['level_S'] != 8:
                    bad.append([file, m, ex.info['level_S']])
            knobs(lds=lds, s=16, tpb=64)
            if not np.array_equal(level(ex, x[:1], file), want[:1]) or ex.info['level_S'] != 16:
                bad.append([file, 'n < S', ex.info['level_S']])
            knobs(lds=lds)
            wide = np.full((130, n_in + 3), np.nan)
            wide[:, 2 : 2 + n_in] = x[:130]
            out = np.full((130, n_out + 4), -7.0)
            level(ex, wide[:, 2 : 2 + n_in], file, out=out[:, 1 : 1 + n_out])
            if not (np.array_equal(out[:, 1 : 1 + n_out], want[:130]) and np.all(out[:, 0] == -7.0) and np.all(out[:, 1 + n_out :] == -7.0)):
                bad.append([file, 'strides'])
            for xin, ref in ((x, want), (x32, want32)):
                for out_dtype in (np.float64, np.float32):
                    got = level(ex, xin[:130], file, out_dtype=out_dtype)
                    if got.dtype != out_dtype or not np.array_equal(got, ref[:130].astype(out_dtype)):
                        bad.append([file, str(xin.dtype), str(np.dtype(out_dtype))])
            level(ex, x, file)
            before = ex.info
            if not np.array_equal(level(ex, x, file), want) or ex.info != before:
                bad.append([file, 'second run', before, ex.info])
    knobs()
    return dict(bad=bad, n=n)


def wide():
    """a level of 2500 statements under blocks of 64 and 1024 lanes, a chain of 120 levels of one statement; both files"""
    rng = np.random.default_rng(5)
    n_in, n_ops = 4, 2500
    ops = [[-1, j, -1, 0, 0, 1, 6, 3] for j in range(n_in)]
    for _ in range(n_ops):
        a, b = (int(v) for v in rng.integers(0, n_in, 2))
        ops.append([int(rng.integers(0, 2)), a, b, int(rng.integers(-2, 3)), 0, 1, 12, 5])
    outs = [n_in + int(v) for v in rng.choice(n_ops, 40, replace=False)]
    wide_prog = np.asarray([1, 0, n_in, 40, len(ops), 0] + [0] * n_in + outs + [0] * 80 + [w for op in ops for w in op], dtype=np.int32)
    deep_ops = [[-1, 0, -1, 0, 0, 1, 6, 2]] + [[4, i, -1, i + 1, 0, 1, 30, 2] for i in range(119)]
    deep_prog = np.asarray([1, 0, 1, 2, 120, 0, 0, 119, 60, 0, 0, 0, 0] + [w for op in deep_ops for w in op], dtype=np.int32)
    bad, widths = [], []
    for prog, x in ((wide_prog, rng.integers(-200, 200, (37, n_in)) / 8.0), (deep_prog, np.linspace(-20, 20, 37).reshape(-1, 1))):
        want = compose([prog], x)
        with dais_compile(prog) as ex:
            widths.append([ex.info['n_levels'], ex.info['level_width']])
            for file, lds in FILES:
                for tpb in (64, None):
                    knobs(lds=lds, tpb=tpb)
                    if not np.array_equal(level(ex, x, file), want):
                        bad.append([widths[-1], file, tpb])
    knobs()
    return dict(bad=bad, widths=widths)


def golden():
    """the reference's golden vectors (every opcode) in both files and a lookup out of bounds in the second stage"""
    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'dais_golden.json.gz', 'rt'))
    bad, n = [], 0
    for case in gold['cases']:
        prog = np.asarray(case['program'], dtype=np.int32)
        x = np.asarray([float.fromhex(v) for v in case['inputs']]).reshape(case['n_samples'], -1)
        want = np.asarray([float.fromhex(v) for v in case['outputs']]).reshape(case['n_samples'], -1)
        with dais_compile(prog) as ex:
            for file, lds in FILES:
                knobs(lds=lds, tpb=256)
                n += 1
                if not np.array_equal(level(ex, x, file), want):
                    bad.append([case['seed'], file])
    p0, x = random_program(11, n_in=3, n_ops=40, n_out=2)
    faults = []
    with dais_compile([p0, faulting_stage(2)]) as ex:
        for file, lds in FILES:
            knobs(lds=lds, tpb=256)
            for rows in (x, x[:1]):  # the handle stays usable, and still reports
                try:
                    level(ex, rows, file)
                    faults.append('no error')
                except RuntimeError as e:
                    faults.append(str(e))
    knobs()
    return dict(bad=bad, n=n, faults=faults)


if __name__ == '__main__':
    print(json.dumps({'chains': chains, 'counts': counts, 'wide': wide, 'golden': golden}[sys.argv[1]]()), flush=True)
