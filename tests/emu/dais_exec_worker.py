"""Worker of tests/test_emulated_dais_exec.py (DA4ML_HIP_LIB = tests/emu/libda4ml_emu.so: kernel k_dais_exec on the CPU, thread by
thread): the chains of tests/dais_exec_cases.py through executor='device' -- staged host arrays, the only memory the emulated device
has -- against the stage-by-stage composition on the host.  DA4ML_DAIS_TILE is read at every run.  One JSON line on stdout.
usage: dais_exec_worker.py <what>"""

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


def compiled(progs):
    ex = dais_compile(progs)
    assert ex.info['regfile'] == 'hbm', ex.info
    yield 'hbm', ex
    ex.close()


def chains():
    """random chains of 2 and 3 stages, 700 samples in tiles of 256: two whole tiles and a partial one whose last block is partial"""
    os.environ['DA4ML_DAIS_TILE'] = '256'
    bad, n = [], 0
    for seed in range(12):
        progs, x = random_chain(seed, 2 + seed % 2, n_samples=700)
        want = compose(progs, x)
        for name, ex in compiled(progs):
            got = ex(x, executor='device')
            n += 1
            if not np.array_equal(got, want):
                bad.append([seed, name])
            if (ex.info['scratch_bytes'] != 8 * 256 * ex.info['n_slots'] or ex.info['scratch_ptr'] == 0):
                bad.append([seed, 'scratch', ex.info])
    return dict(bad=bad, n=n)


def counts():
    """1, 63, 64 and 65 samples; an absent output at the boundary; rows inside wider arrays, float32 in and out; one handle run again"""
    os.environ.pop('DA4ML_DAIS_TILE', None)
    bad, n = [], 0
    progs, x = random_chain(3, 2, n_samples=130)
    progs[0] = with_absent_output(progs[0], 1)
    want = compose(progs, x)
    n_in, n_out = x.shape[1], want.shape[1]
    for name, ex in compiled(progs):
        for m in (1, 63, 64, 65, 130):
            n += 1
            if not np.array_equal(ex(x[:m], executor='device'), want[:m]):
                bad.append([name, m])
        wide = np.full((130, n_in + 3), np.nan)
        wide[:, 2 : 2 + n_in] = x
        out = np.full((130, n_out + 4), -7.0)
        ex(wide[:, 2 : 2 + n_in], out=out[:, 1 : 1 + n_out], executor='device')
        if not (np.array_equal(out[:, 1 : 1 + n_out], want) and np.all(out[:, 0] == -7.0) and np.all(out[:, 1 + n_out :] == -7.0)):
            bad.append([name, 'strides'])
        x32 = x.astype(np.float32)
        want32 = compose(progs, x32.astype(np.float64))
        if not np.array_equal(ex(x32, out_dtype=np.float32, executor='device'), want32.astype(np.float32)):
            bad.append([name, 'float32'])
        before = ex.info
        if not np.array_equal(ex(x, executor='device'), want) or ex.info != before:
            bad.append([name, 'second run', before, ex.info])
    return dict(bad=bad, n=n)


def golden():
    """the reference's golden vectors (every opcode) and a lookup out of bounds in the second stage"""
    os.environ.pop('DA4ML_DAIS_TILE', None)
    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'dais_golden.json.gz', 'rt'))
    bad, n = [], 0
    for case in gold['cases']:
        prog = np.asarray(case['program'], dtype=np.int32)
        x = np.asarray([float.fromhex(v) for v in case['inputs']]).reshape(case['n_samples'], -1)
        want = np.asarray([float.fromhex(v) for v in case['outputs']]).reshape(case['n_samples'], -1)
        for name, ex in compiled([prog]):
            n += 1
            if not np.array_equal(ex(x, executor='device'), want):
                bad.append([case['seed'], name])
    p0, x = random_program(11, n_in=3, n_ops=40, n_out=2)
    faults = []
    for name, ex in compiled([p0, faulting_stage(2)]):
        try:
            ex(x, executor='device')
            faults.append('no error')
        except RuntimeError as e:
            faults.append(str(e))
        try:  # the handle stays usable, and still reports
            ex(x[:1], executor='device')
            faults.append('no error')
        except RuntimeError as e:
            faults.append(str(e))
    return dict(bad=bad, n=n, faults=faults)


if __name__ == '__main__':
    print(json.dumps({'chains': chains, 'counts': counts, 'golden': golden}[sys.argv[1]]()), flush=True)
