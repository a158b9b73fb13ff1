"""Worker of tests/test_emulated_slack.py: the score slack (slack= of da4ml_amd.cmvm.solve_restarts, 'slack' of _binary.solve_each,
da_solve_batch_search) on the emulated device, in a process whose DA4ML_HIP_LIB points at tests/emu/libda4ml_emu.so.  One JSON line on
stdout.  usage: slack_worker.py <what> [args]"""

import ctypes as C
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import newest_cases  # noqa: E402
import numpy as np  # noqa: E402
import restart_cases  # noqa: E402
from cases import int_matrix  # noqa: E402
from slack_cases import CASES, SINGLE, digest, mixed_batch, op_list, restart_options  # noqa: E402

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import first_strict_minimum, restart_seeds, solve_recoded, solve_restarts  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def case(name):
    mat, opts = CASES[name][:2]
    k = int_matrix(*mat)
    pipes = hip.solve_each([k] * CASES[name][2], restart_options(name))
    tm = hip.timings()
    costs = [pipeline_cost_f32(p) for p in pipes]
    out(digests=[digest(p) for p in pipes], costs=costs, adders=[p.n_adders for p in pipes], best=first_strict_minimum(costs), ops=[op_list(p) for p in pipes],
        kernel_ok=all(np.array_equal(p.kernel, k) for p in pipes), plain=digest(hip.solve(k, **{key: v for key, v in opts.items() if key != 'dc_weight'})),
        retries=tm['retries'], manycol=tm['manycol_chains'])  # fmt: skip


def mixed():
    """every problem of the mixed call, in the call and alone"""
    batch = mixed_batch()
    ks = [int_matrix(*mat) for _, mat, _ in batch]
    together = hip.solve_each(ks, [o for _, _, o in batch])
    alone = [hip.solve_each([k], [o])[0] for k, (_, _, o) in zip(ks, batch)]
    plain = {label: digest(hip.solve(k, **SINGLE)) for k, (label, _, _) in zip(ks, batch) if label.startswith('plain')}
    out(labels=[label for label, _, _ in batch], together=[digest(p) for p in together], alone=[digest(p) for p in alone], plain=plain,
        costs=[pipeline_cost_f32(p) for p in together], adders=[p.n_adders for p in together], kernel_ok=all(np.array_equal(p.kernel, k) for p, k in zip(together, ks)))  # fmt: skip


def old_records():
    """the restarts of tests/restart_cases.py and tests/newest_cases.py through this library: nothing that was recorded moves"""
    res = {}
    for tag, cases, order in (('random', {n: restart_cases.CASES[n] for n in ('small16', 'wide300')}, 'random'), ('newest', {n: newest_cases.CASES[n] for n in ('small16', 'wmcdc16')}, 'newest')):
        for name, (mat, opts, n, seed) in cases.items():
            k = int_matrix(*mat)
            res[f'{tag}:{name}'] = [digest(p) for p in solve_restarts(k, n, seed=seed, order=order, return_all=True, **opts)[1]]
            res[f'{tag}:{name}:slack0'] = [digest(p) for p in solve_restarts(k, n, seed=seed, order=order, slack=0, return_all=True, **opts)[1]]
    out(**res)


def raw_call(k, opts, search, n, recode=None, entry='search'):
    r = (C.c_void_p * n)()
    args = (n, (C.c_void_p * n)(*[k.ctypes.data] * n), np.array([k.shape[0]] * n, np.int64), np.array([k.shape[1]] * n, np.int64), C.cast(opts, C.c_void_p))
    rec = None if recode is None else C.cast(recode, C.c_void_p)
    if entry == 'recode':
        rc = hip.lib().da_solve_batch_recode(*args, rec, None, None, r)
    else:
        rc = hip.lib().da_solve_batch_search(*args, rec, None if search is None else C.cast(search, C.c_void_p), None, None, r)
    if rc != 0:
        return [rc, hip.lib().da_last_error().decode()]
    return [rc, [digest(hip._collect(r[i])) for i in range(n)]]


def abi():
    mat, _, n, seed, slack, _ = CASES['small16']
    k = int_matrix(*mat)
    s = restart_seeds(n, seed)
    size = C.sizeof(hip.SearchOpts)
    mk = lambda tie_seed=0: hip.SolveOpts(C.sizeof(hip.SolveOpts), b'wmc', b'wmc', -1, -1, -1, -1, 0, hip.DC_WEIGHT_DEFAULT, tie_seed, 0)  # noqa: E731
    seeded = (hip.SolveOpts * 2)(mk(s[1]), mk(s[2]))
    half = (hip.SolveOpts * 2)(mk(), mk(s[2]))  # the first problem without a seed
    sea = lambda *v: (hip.SearchOpts * len(v))(*[hip.SearchOpts(sz, sl) for sz, sl in v])  # noqa: E731
    compact = (hip.RecodeOpts * 2)(*[hip.RecodeOpts(C.sizeof(hip.RecodeOpts), 1, 0)] * 2)
    res = dict(size=size, opts_size=C.sizeof(hip.SolveOpts), recode_size=C.sizeof(hip.RecodeOpts))
    res['recode'] = raw_call(k, seeded, None, 2, entry='recode')
    res['null'] = raw_call(k, seeded, None, 2)
    res['zero'] = raw_call(k, seeded, sea((size, 0), (size, 0)), 2)
    res['slack'] = raw_call(k, seeded, sea((size, slack), (size, slack)), 2)
    res['slack_again'] = raw_call(k, seeded, sea((size, slack), (size, slack)), 2)
    res['one'] = raw_call(k, seeded, sea((size, 0), (size, slack)), 2)
    res['half'] = raw_call(k, half, sea((size, 0), (size, slack)), 2)  # slack 0 on the unseeded problem is fine
    res['255'] = raw_call(k, seeded, sea((size, 255), (size, 255)), 2)
    for bad in (256, 1000, 0xFFFFFFFF):
        res[f'slack {bad}'] = raw_call(k, seeded, sea((size, slack), (size, bad)), 2)
    for bad in (0, 4, 12, 16):
        res[f'size {bad}'] = raw_call(k, seeded, sea((size, slack), (bad, slack)), 2)
    res['no seed'] = raw_call(k, half, sea((size, slack), (size, slack)), 2)
    res['compact_recode'] = raw_call(k, seeded, None, 2, recode=compact, entry='recode')
    res['compact_null'] = raw_call(k, seeded, None, 2, recode=compact)
    res['compact_slack'] = raw_call(k, seeded, sea((size, slack), (size, slack)), 2, recode=compact)
    out(**res)


def shard():
    """a column-sharded chain takes no slack (the test hook DA4ML_SHARD_SLACK is how one gets there at all)"""
    k = int_matrix(*CASES['small16'][0])
    res = {}
    for slack in ('0', '16'):
        os.environ['DA4ML_SHARD_SLACK'] = slack
        try:
            p, st = hip.solve_sharded(k, rank=0, world=1, **SINGLE)
            res[slack] = [digest(p), int(st['sharded_chains'])]
        except Exception as e:  # noqa: BLE001
            res[slack] = [type(e).__name__, str(e), hip.lib().da_last_error_code()]
    del os.environ['DA4ML_SHARD_SLACK']
    res['plain'] = digest(hip.solve(k, **SINGLE))
    out(**res)


def python_api():
    res = {}
    for name in ('small16', 'newest16', 'compact16'):
        mat, opts, n, seed, slack, extra = CASES[name]
        k = int_matrix(*mat)
        kw = dict({'order': extra['tie_order']} if 'tie_order' in extra else {}, **({'recode': extra['recode']} if 'recode' in extra else {}))
        best, pipes, costs = solve_restarts(k, n, seed=seed, slack=slack, return_all=True, **kw, **opts)
        res[name] = [digest(p) for p in pipes]
        res[name + ' best'] = best
        res[name + ' winner'] = digest(solve_restarts(k, n, seed=seed, slack=slack, **kw, **opts))
        res[name + ' never dearer'] = costs[best] <= costs[0]
        many_kw = dict({'tie_order': extra['tie_order']} if 'tie_order' in extra else {}, **({'recode': extra['recode']} if 'recode' in extra else {}))
        res[name + ' many'] = [digest(p) for p in hip.solve_many([k] * n, seeds=restart_seeds(n, seed), slack=slack, **many_kw, **opts)]
    mat, opts, n, seed, slack, _ = CASES['small16']
    k = int_matrix(*mat)
    res['plain'] = digest(hip.solve(k, **opts))
    res['slack0'] = [digest(p) for p in solve_restarts(k, n, seed=seed, slack=0, return_all=True, **opts)[1]]
    res['default'] = [digest(p) for p in solve_restarts(k, n, seed=seed, return_all=True, **opts)[1]]
    res['numpy int'] = [digest(p) for p in solve_restarts(k, 2, seed=seed, slack=np.int64(slack), return_all=True, **opts)[1]]
    errors = (('restarts 256', lambda: solve_restarts(k, 2, slack=256, **opts)), ('restarts -1', lambda: solve_restarts(k, 2, slack=-1, **opts)),
              ('restarts float', lambda: solve_restarts(k, 2, slack=4.0, **opts)), ('restarts str', lambda: solve_restarts(k, 2, slack='4', **opts)),
              ('restarts None', lambda: solve_restarts(k, 2, slack=None, **opts)), ('restarts bool', lambda: solve_restarts(k, 2, slack=True, **opts)),
              ('many', lambda: hip.solve_many([k], seeds=[1], slack=300, **opts)), ('each', lambda: hip.solve_each([k], [dict(opts, seed=1, slack=2.5)])),
              ('each no seed', lambda: hip.solve_each([k], [dict(opts, slack=4)])), ('recoded', lambda: solve_recoded(k, 2, slack=4, **opts)))  # fmt: skip
    for label, fn in errors:
        try:
            fn()
            res['error ' + label] = None
        except Exception as e:  # noqa: BLE001
            res['error ' + label] = type(e).__name__
    out(**res)


def sharded_stand_in():
    """multi_gpu.solve_restarts_sharded(slack=) in one process (world 1): the slack reaches the solver only when it is not 0, the result is solve_restarts'"""
    from da4ml_amd import multi_gpu as mg

    mat, opts, n, seed, slack, _ = CASES['small16']
    k = int_matrix(*mat)
    mg.init('gloo')
    seen = []

    def spy(kernels, **kw):
        seen.append(sorted(kw))
        return hip.solve_many(kernels, **kw)

    got = digest(mg.solve_restarts_sharded(k, n, seed=seed, slack=slack, solver=spy, **opts))
    flat = digest(mg.solve_restarts_sharded(k, n, seed=seed, solver=spy, **opts))
    zero = digest(mg.solve_restarts_sharded(k, n, seed=seed, slack=0, solver=spy, **opts))
    real = digest(mg.solve_restarts_sharded(k, n, seed=seed, slack=slack, **opts))
    try:
        mg.solve_restarts_sharded(k, n, seed=seed, slack=256, **opts)
        err = None
    except ValueError:
        err = 'ValueError'
    mg.shutdown()
    out(slack=got, real=real, flat=flat, zero=zero, want_slack=digest(solve_restarts(k, n, seed=seed, slack=slack, **opts)), want_flat=digest(solve_restarts(k, n, seed=seed, **opts)),
        error=err, saw_slack=['slack' in s for s in seen])  # fmt: skip


if __name__ == '__main__':
    {'case': lambda: case(sys.argv[2]), 'mixed': mixed, 'old': old_records, 'abi': abi, 'shard': shard, 'python_api': python_api, 'sharded': sharded_stand_in}[sys.argv[1]]()
