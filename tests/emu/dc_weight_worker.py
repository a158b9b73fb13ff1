"""Worker of tests/test_emulated_dc_weight.py: the tunable latency-penalty weight of the -dc / -pdc selectors (_binary.solve_each, da_solve_batch_opts,
da4ml_amd.cmvm.solve_tradeoff) on the emulated device, in a process whose DA4ML_HIP_LIB points at tests/emu/libda4ml_emu.so.  That build runs candidate
lists of two entries, so most steps find their pick by a pass over the whole table and the others take it from the lists the step before left: the
two agree only if every rank of a weighted chain is formed with the chain's weight.  One JSON line on stdout.  usage: dc_weight_worker.py <what> [args]"""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
from cases import int_matrix  # noqa: E402
from dc_weight_cases import CASES, DEFAULT_WEIGHT, ONE_CHAIN, digest, latency_of, matrix_args, mixed_call, op_list, points, wkey  # noqa: E402

from da4ml_amd import _binary as hip  # noqa: E402
from da4ml_amd.cmvm import cheapest_within, solve_tradeoff  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402


def out(**kw):
    print(json.dumps(kw), flush=True)


def solve_points(name):
    k = int_matrix(*CASES[name][0])
    pts = points(name)
    q = [p[3] for p in pts] if pts[0][3] is not None else None
    l = [p[4] for p in pts] if pts[0][4] is not None else None
    return k, pts, hip.solve_each([k] * len(pts), [p[2] for p in pts], qintervals=q, latencies=l)


def records(name):
    """every method and weight of a case, all in one call: {method: {weight: {digest, cost, latency}}}, and whether every graph implements the matrix"""
    k, pts, pipes = solve_points(name)
    rec = {}
    for (m, w, *_), p in zip(pts, pipes):
        rec.setdefault(str(m), {})[wkey(w)] = dict(digest=digest(p), cost=pipeline_cost_f32(p), latency=latency_of(p), adders=p.n_adders)
    t = hip.timings()
    out(points=rec, kernel_ok=all(np.array_equal(p.kernel, k) for p in pipes), manycol=t['manycol_chains'], chains=t['chains'], retries=t['retries'])


def pins():
    """the ends of the weight axis, against the UNPATCHED restatement: weight 0 is the selector without a penalty, a huge weight of mc-dc is mc-dc"""
    from oracle.oracle import Oracle

    o = Oracle('port')
    one = lambda m, **kw: dict(ONE_CHAIN, method0=m, method1=m, **kw)  # noqa: E731
    res = {}
    for name, asked, want in (('mc12', ('mc-pdc', 0.0), 'mc'), ('mc12', ('mc-dc', 0.0), 'mc'), ('narrow16', ('wmc-pdc', 0.0), 'wmc'), ('mc12', ('mc-dc', 1e6), 'mc-dc'),
                              ('narrow16', ('mc-pdc', 0.0), 'mc'), ('narrow16', ('mc-dc', 1e6), 'mc-dc')):  # fmt: skip
        k = int_matrix(*CASES[name][0])
        got = hip.solve_each([k], [one(asked[0], dc_weight=asked[1])])[0]
        res[f'{name} {asked[0]} {asked[1]} == {want}'] = op_list(got) == op_list(o.solve(k, **one(want)))
    out(pins=res)


def equivalence():
    """the method's own constant spelled out == unset == solve(), for every method of the one-chain cases with narrow entries"""
    bad = []
    for name in ('narrow16', 'mc12', 'lat16'):
        mat, opts, methods, _ = CASES[name]
        k = int_matrix(*mat)
        for m in methods:
            o = dict(opts, **(dict(method0=m, method1=m) if m else {}))
            per = {key: v for key, v in o.items() if key not in ('qintervals', 'latencies')}
            kw = {key: [o[key]] * 3 for key in ('qintervals', 'latencies') if key in o}
            explicit = DEFAULT_WEIGHT[m]
            a, b, c = hip.solve_each([k] * 3, [dict(per, dc_weight=explicit), dict(per, dc_weight=None), per], **kw)
            if not (a == b == c == hip.solve(k, **o)):
                bad.append([name, m])
    out(bad=bad)


def narrow_chains():
    """op lists of the narrow16 chains (the test runs this under several table geometries)"""
    k, pts, pipes = solve_points('narrow16')
    out(op_lists=[op_list(p) for p in pipes], kernel_ok=all(np.array_equal(p.kernel, k) for p in pipes), retries=hip.timings()['retries'],
        distinct=len({json.dumps(op_list(p)) for p in pipes}))  # fmt: skip


def mixed():
    """one call with mixed options against every problem solved alone"""
    call = mixed_call()
    mats = {name: int_matrix(*matrix_args(name)) for name, _ in call}
    got = hip.solve_each([mats[name] for name, _ in call], [o for _, o in call])
    alone = [hip.solve_each([mats[name]], [o])[0] for name, o in call]
    out(equal=[digest(a) == digest(b) for a, b in zip(got, alone)], digests=[digest(p) for p in got], kernel_ok=[bool(np.array_equal(p.kernel, mats[name])) for (name, _), p in zip(call, got)],
        weight_matters=digest(got[1]) != digest(got[4]))  # fmt: skip


def errors():
    k = int_matrix(*CASES['mc12'][0])
    res = {}
    for label, w in (('-0.5', -0.5), ('nan', float('nan')), ('inf', float('inf')), ('-1', -1.0)):
        try:
            hip.solve_each([k], [dict(dc_weight=w)])
            res[label] = 'no error'
        except ValueError as e:
            res[label] = f'ValueError: {e}'
    # the library's own check (the binding raises before the call for the values above): the struct handed over as it is
    import ctypes as C

    for label, w in (('abi -0.5', -0.5), ('abi nan', float('nan')), ('abi inf', float('inf'))):
        o = (hip.SolveOpts * 1)(hip.SolveOpts(C.sizeof(hip.SolveOpts), b'wmc', b'auto', -1, -2, -1, -1, 1, w, 0))
        r = (C.c_void_p * 1)()
        rc = hip.lib().da_solve_batch_opts(1, (C.c_void_p * 1)(k.ctypes.data), np.array([k.shape[0]], np.int64), np.array([k.shape[1]], np.int64), C.cast(o, C.c_void_p), None, None, r)
        res[label] = [rc, hip.lib().da_last_error().decode()]
    try:
        hip.solve_each([k, k], [{}])
        res['length'] = 'no error'
    except ValueError as e:
        res['length'] = f'ValueError: {e}'
    out(**res)


def tradeoff():
    """solve_tradeoff on narrow16 with the case's own options (one chain per point), its default weights and methods"""
    k, opts = int_matrix(*CASES['narrow16'][0]), CASES['narrow16'][1]
    L = hip.lib()
    real, calls = L.da_solve_batch_opts, []

    def counting(*a):
        calls.append(a[0])
        return real(*a)

    L.da_solve_batch_opts = counting
    front, pts = solve_tradeoff(k, return_all=True, **opts)
    L.da_solve_batch_opts = real
    plain = hip.solve(k, **opts)
    small = int_matrix(*CASES['mc12'][0])  # (the front alone: a sweep of two points on the small matrix)
    few = dict(weights=(1.0,), methods=('wmc-pdc',), **opts)
    row = lambda p: [p.cost, p.latency, p.method0, p.method1, p.dc_weight, digest(p.pipeline)]  # noqa: E731
    try:
        cheapest_within(front, front[0].latency - 1)
        below = 'no error'
    except ValueError as e:
        below = str(e)
    out(front=[row(p) for p in front], points=[row(p) for p in pts], calls=calls, point0_is_solve=pts[0].pipeline == plain, solve_cost=pipeline_cost_f32(plain),
        within=row(cheapest_within(front, pts[0].latency)), below=below,
        front_only_ok=[row(p) for p in solve_tradeoff(small, **few)] == [row(p) for p in solve_tradeoff(small, return_all=True, **few)[0]],
        kernel_ok=all(np.array_equal(p.pipeline.kernel, k) for p in pts))  # fmt: skip


if __name__ == '__main__':
    what = sys.argv[1]
    {'records': lambda: records(sys.argv[2]), 'pins': pins, 'equivalence': equivalence, 'narrow': narrow_chains, 'mixed': mixed, 'errors': errors, 'tradeoff': tradeoff}[what]()
