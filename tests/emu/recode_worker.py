"""Worker of tests/test_emulated_recode.py: the digit recodings (da4ml_amd.cmvm.solve_recoded, 'recode' / 'recode_seed' of _binary.solve_each,
da_solve_batch_recode) on the emulated device, in a process whose DA4ML_HIP_LIB points at tests/emu/libda4ml_emu.so.  One JSON line on
stdout.  usage: recode_worker.py <what> [args]"""

import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
import restart_cases  # noqa: E402
from cases import int_matrix  # noqa: E402
from recode_cases import CASES, SINGLE, digest, mixed_batch, op_list, points  # noqa: E402

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import restart_seeds, solve_recoded, solve_restarts  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def case(name):
    mat, opts, n, seed = CASES[name]
    k = int_matrix(*mat)
    best, pipes, costs = solve_recoded(k, n, seed=seed, return_all=True, **opts)
    tm = hip.timings()
    out(digests=[digest(p) for p in pipes], costs=costs, adders=[p.n_adders for p in pipes], best=best, ops=[op_list(p) for p in pipes],
        kernel_ok=all(np.array_equal(p.kernel, k) for p in pipes), cost_ok=all(c == pipeline_cost_f32(p) for c, p in zip(costs, pipes)),
        plain=digest(hip.solve(k, **opts)), winner=digest(solve_recoded(k, n, seed=seed, **opts)), retries=tm['retries'], manycol=tm['manycol_chains'])  # fmt: skip


def mixed():
    """every problem of the mixed call, in the call and alone"""
    batch = mixed_batch()
    ks = [int_matrix(*mat) for _, mat, _ in batch]
    together = hip.solve_each(ks, [o for _, _, o in batch])
    alone = [hip.solve_each([k], [o])[0] for k, (_, _, o) in zip(ks, batch)]
    plain = {label: digest(hip.solve(k, **SINGLE)) for k, (label, _, _) in zip(ks, batch) if label.startswith('plain')}
    out(labels=[label for label, _, _ in batch], together=[digest(p) for p in together], alone=[digest(p) for p in alone], plain=plain,
        costs=[pipeline_cost_f32(p) for p in together], adders=[p.n_adders for p in together], kernel_ok=all(np.array_equal(p.kernel, k) for p, k in zip(together, ks)))  # fmt: skip


def raw_call(k, opts, recode, n):
    r = (C.c_void_p * n)()
    args = (n, (C.c_void_p * n)(*[k.ctypes.data] * n), np.array([k.shape[0]] * n, np.int64), np.array([k.shape[1]] * n, np.int64), C.cast(opts, C.c_void_p))
    if recode == 'opts':
        rc = hip.lib().da_solve_batch_opts(*args, None, None, r)
    else:
        rc = hip.lib().da_solve_batch_recode(*args, None if recode is None else C.cast(recode, C.c_void_p), None, None, r)
    if rc != 0:
        return [rc, hip.lib().da_last_error().decode()]
    return [rc, [digest(hip._collect(r[i])) for i in range(n)]]


def abi():
    mat, _, n, seed = CASES['bits8']
    k = int_matrix(*mat)
    s = restart_seeds(n, seed)
    size = C.sizeof(hip.RecodeOpts)
    mk = lambda tie_seed=0: hip.SolveOpts(C.sizeof(hip.SolveOpts), b'wmc', b'wmc', -1, -1, -1, -1, 0, hip.DC_WEIGHT_DEFAULT, tie_seed, 0)  # noqa: E731
    opts = (hip.SolveOpts * 2)(mk(), mk())
    tied = (hip.SolveOpts * 2)(mk(), mk(s[1]))  # the second problem with a tie seed
    rec = lambda *modes: (hip.RecodeOpts * len(modes))(*[hip.RecodeOpts(sz, m, sd) for sz, m, sd in modes])  # noqa: E731
    res = dict(size=size, opts_size=C.sizeof(hip.SolveOpts))
    res['opts'] = raw_call(k, opts, 'opts', 2)
    res['null'] = raw_call(k, opts, None, 2)
    res['csd'] = raw_call(k, opts, rec((size, 0, 0), (size, 0, s[2])), 2)  # CSD reads no seed
    res['compact'] = raw_call(k, opts, rec((size, 1, 0), (size, 1, s[2])), 2)
    res['compact_seed_ignored'] = raw_call(k, opts, rec((size, 1, 77), (size, 1, 0)), 2)
    res['seeded'] = raw_call(k, opts, rec((size, 2, s[2]), (size, 2, s[3])), 2)
    res['seeded_again'] = raw_call(k, opts, rec((size, 2, s[2]), (size, 2, s[3])), 2)
    for mode in (3, 4, 0xFFFFFFFF):
        res[f'mode {mode}'] = raw_call(k, opts, rec((size, 0, 0), (size, mode, 0)), 2)
    for bad in (0, 8, 12, 24, 32):
        res[f'size {bad}'] = raw_call(k, opts, rec((size, 1, 0), (bad, 1, 0)), 2)
    res['tied_opts'] = raw_call(k, tied, 'opts', 2)
    res['tied_csd'] = raw_call(k, tied, rec((size, 0, 0), (size, 0, 0)), 2)
    res['tied_compact'] = raw_call(k, tied, rec((size, 1, 0), (size, 1, 0)), 2)
    res['each_tied_compact'] = [digest(p) for p in hip.solve_each([k, k], [dict(SINGLE, recode='compact'), dict(SINGLE, seed=s[1], recode='compact')])]
    out(**res)


def shard():
    """a column-sharded chain takes the CSD digits only (the test hook DA4ML_SHARD_RECODE is how a mode gets there at all)"""
    k = int_matrix(*CASES['small16'][0])
    res = {}
    for mode in ('0', '1', '2'):
        os.environ['DA4ML_SHARD_RECODE'] = mode
        try:
            p, st = hip.solve_sharded(k, rank=0, world=1, **SINGLE)
            res[mode] = [digest(p), int(st['sharded_chains'])]
        except Exception as e:  # noqa: BLE001
            res[mode] = [type(e).__name__, str(e), hip.lib().da_last_error_code()]
    del os.environ['DA4ML_SHARD_RECODE']
    res['plain'] = digest(hip.solve(k, **SINGLE))
    out(**res)


def python_api():
    mat, opts, n, seed = restart_cases.CASES['small16']
    k = int_matrix(*mat)
    res = {}
    res['default'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, **opts)[1]]
    res['csd'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, recode='csd', **opts)[1]]
    res['csd_newest'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, order='newest', recode='csd', **opts)[1]]
    res['newest'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, order='newest', **opts)[1]]
    s = restart_seeds(4, seed)
    for mode in ('compact', 'seeded'):
        res[mode] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, recode=mode, **opts)[1]]
        res[mode + '_each'] = [digest(p) for p in hip.solve_each([k] * 4, [dict(opts, seed=v, recode=mode, recode_seed=v) if v else dict(opts) for v in s])]
        res[mode + '_many'] = [digest(p) for p in hip.solve_many([k] * 4, seeds=s, recode=mode, **opts)]
    res['plain'] = digest(hip.solve(k, **opts))
    rmat, ropts, rn, rseed = CASES['bits8']
    rk = int_matrix(*rmat)
    best, pipes, costs = solve_recoded(rk, rn, seed=rseed, return_all=True, **ropts)
    res['recoded'] = [digest(p) for p in pipes]
    res['recoded_each'] = [digest(p) for p in hip.solve_each([rk] * rn, [dict(ropts, recode=m, recode_seed=v) for m, v in points(rn, rseed)])]
    res['recoded_plain'] = digest(hip.solve(rk, **ropts))
    res['recoded_one'] = digest(solve_recoded(rk, 1, **ropts))
    for label, fn in (('restarts', lambda: solve_restarts(k, 2, recode='naf', **opts)), ('restarts None', lambda: solve_restarts(k, 2, recode=None, **opts)),
                      ('many', lambda: hip.solve_many([k], seeds=[1], recode='Compact', **opts)), ('each', lambda: hip.solve_each([k], [dict(opts, recode=1)])),
                      ('recoded seed', lambda: solve_recoded(k, 2, tie_order='newest', **opts)), ('recoded n', lambda: solve_recoded(k, 0, **opts))):  # fmt: skip
        try:
            fn()
            res['error ' + label] = None
        except Exception as e:  # noqa: BLE001
            res['error ' + label] = type(e).__name__
    out(**res)


def sharded_stand_in():
    """multi_gpu.solve_restarts_sharded(recode=) in one process (world 1): the recoding reaches the solver, the result is solve_restarts'"""
    from da4ml_amd import multi_gpu as mg

    mat, opts, n, seed = CASES['bits8']
    k = int_matrix(*mat)
    mg.init('gloo')
    got = digest(mg.solve_restarts_sharded(k, n, seed=seed, recode='compact', **opts))
    csd = digest(mg.solve_restarts_sharded(k, n, seed=seed, **opts))
    try:
        mg.solve_restarts_sharded(k, n, seed=seed, recode='x', **opts)
        err = None
    except ValueError:
        err = 'ValueError'
    mg.shutdown()
    out(compact=got, csd=csd, want_compact=digest(solve_restarts(k, n, seed=seed, recode='compact', **opts)), want_csd=digest(solve_restarts(k, n, seed=seed, **opts)), error=err)


if __name__ == '__main__':
    {'case': lambda: case(sys.argv[2]), 'mixed': mixed, 'abi': abi, 'shard': shard, 'python_api': python_api, 'sharded': sharded_stand_in}[sys.argv[1]]()
