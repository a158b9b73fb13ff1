"""Worker of tests/test_emulated_newest.py: the newest-row-first tie order (order='newest' of da4ml_amd.cmvm.solve_restarts, 'tie_order' of
_binary.solve_each / solve_many, da_solve_opts.tie_order) on the emulated device, in a process whose DA4ML_HIP_LIB points at
tests/emu/libda4ml_emu.so.  That build runs candidate lists of two entries, so most steps find their pick by a pass over the whole table and
the others take it from the lists the step before left: the two agree only if every site forms the word of the chain's order.  One JSON
line on stdout.  usage: newest_worker.py <what> [args]"""

import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
from cases import int_matrix  # noqa: E402
from newest_cases import CASES, SINGLE, digest, mixed_batch, op_list  # noqa: E402

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import restart_seeds, solve_restarts  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def case(name):
    mat, opts, n, seed = CASES[name]
    k = int_matrix(*mat)
    best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, order='newest', **opts)
    tm = hip.timings()
    out(digests=[digest(p) for p in pipes], costs=costs, adders=[p.n_adders for p in pipes], best=best, ops=[op_list(p) for p in pipes],
        kernel_ok=all(np.array_equal(p.kernel, k) for p in pipes), cost_ok=all(c == pipeline_cost_f32(p) for c, p in zip(costs, pipes)),
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


def raw_call(k, blob, n=1):
    r = (C.c_void_p * n)()
    rc = hip.lib().da_solve_batch_opts(n, (C.c_void_p * n)(*[k.ctypes.data] * n), np.array([k.shape[0]] * n, np.int64), np.array([k.shape[1]] * n, np.int64),
                                       C.cast(blob, C.c_void_p), None, None, r)  # fmt: skip
    if rc != 0:
        return [rc, hip.lib().da_last_error().decode()]
    return [rc, [digest(hip._collect(r[i])) for i in range(n)]]


class OptsV1(C.Structure):
    """da_solve_opts as it was before tie_order: what a caller built against the previous header passes"""

    _fields_ = hip.SolveOpts._fields_[:-1]


def abi():
    mat, opts, n, seed = CASES['small16']
    k = int_matrix(*mat)
    s = restart_seeds(n, seed)
    res = dict(size_v1=C.sizeof(OptsV1), size=C.sizeof(hip.SolveOpts), last_field=hip.SolveOpts._fields_[-1][0])
    mk = lambda cls, size, seed_, *more: cls(size, b'wmc', b'wmc', -1, -1, -1, -1, 0, hip.DC_WEIGHT_DEFAULT, seed_, *more)  # noqa: E731
    # the previous struct, two of them in one array (56 bytes apart): accepted, the random order
    res['v1'] = raw_call(k, (OptsV1 * 2)(mk(OptsV1, C.sizeof(OptsV1), s[1]), mk(OptsV1, C.sizeof(OptsV1), s[2])), 2)
    res['new_random'] = raw_call(k, (hip.SolveOpts * 2)(mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), s[1], 0), mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), s[2], 0)), 2)
    res['new_newest'] = raw_call(k, (hip.SolveOpts * 2)(mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), s[1], 1), mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), s[2], 1)), 2)
    res['seed0_newest'] = raw_call(k, (hip.SolveOpts * 1)(mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), 0, 1)))
    res['seeded_api'] = [digest(p) for p in hip.solve_many([k, k], seeds=s[1:3], **SINGLE)]  # da_solve_batch_seeded: the random order
    res['plain'] = digest(hip.solve(k, **SINGLE))
    for size in (0, 8, C.sizeof(OptsV1) - 8, C.sizeof(OptsV1) + 4, C.sizeof(hip.SolveOpts) + 8, 2 * C.sizeof(hip.SolveOpts)):
        res[f'size {size}'] = raw_call(k, (hip.SolveOpts * 2)(mk(hip.SolveOpts, size, s[1], 0), mk(hip.SolveOpts, size, s[2], 0)))
    res['mixed sizes'] = raw_call(k, (hip.SolveOpts * 2)(mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), s[1], 0), mk(hip.SolveOpts, C.sizeof(OptsV1), s[2], 0)), 2)
    for order in (2, 3, 0xFFFFFFFF):
        res[f'order {order}'] = raw_call(k, (hip.SolveOpts * 1)(mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), s[1], order)))
    res['order 2 seed 0'] = raw_call(k, (hip.SolveOpts * 1)(mk(hip.SolveOpts, C.sizeof(hip.SolveOpts), 0, 2)))[0]  # an unknown order is an error whatever the seed
    out(**res)


def python_api():
    mat, opts, n, seed = CASES['small16']
    k = int_matrix(*mat)
    res = {}
    res['default'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, **opts)[1]]
    res['random'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, order='random', **opts)[1]]
    res['newest'] = [digest(p) for p in solve_restarts(k, 4, seed=seed, return_all=True, order='newest', **opts)[1]]
    res['many_newest'] = [digest(p) for p in hip.solve_many([k] * 4, seeds=restart_seeds(4, seed), tie_order='newest', **opts)]
    res['many_newest_no_seeds'] = [digest(p) for p in hip.solve_many([k], tie_order='newest', **opts)]
    res['plain'] = digest(hip.solve(k, **opts))
    for label, fn in (('restarts', lambda: solve_restarts(k, 2, order='oldest', **opts)), ('restarts None', lambda: solve_restarts(k, 2, order=None, **opts)),
                      ('many', lambda: hip.solve_many([k], seeds=[1], tie_order='Newest', **opts)), ('each', lambda: hip.solve_each([k], [dict(opts, seed=1, tie_order=1)]))):  # fmt: skip
        try:
            fn()
            res['error ' + label] = None
        except Exception as e:  # noqa: BLE001
            res['error ' + label] = type(e).__name__
    out(**res)


def sharded_stand_in():
    """multi_gpu.solve_restarts_sharded(order=) in one process (world 1): the order reaches the solver, the result is solve_restarts'"""
    from da4ml_amd import multi_gpu as mg

    mat, opts, n, seed = CASES['small16']
    k = int_matrix(*mat)
    mg.init('gloo')
    got = digest(mg.solve_restarts_sharded(k, n, seed=seed, order='newest', **opts))
    rnd = digest(mg.solve_restarts_sharded(k, n, seed=seed, **opts))
    try:
        mg.solve_restarts_sharded(k, n, seed=seed, order='x', **opts)
        err = None
    except ValueError:
        err = 'ValueError'
    mg.shutdown()
    out(newest=got, random=rnd, want_newest=digest(solve_restarts(k, n, seed=seed, order='newest', **opts)), want_random=digest(solve_restarts(k, n, seed=seed, **opts)), error=err)


if __name__ == '__main__':
    {'case': lambda: case(sys.argv[2]), 'mixed': mixed, 'abi': abi, 'python_api': python_api, 'sharded': sharded_stand_in}[sys.argv[1]]()
