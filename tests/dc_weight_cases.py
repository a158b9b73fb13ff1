"""The latency-penalty-weight cases that tests/golden/make_dc_weight_golden.py records with a patched copy of the restatement (oracle/cmvm_oracle.cc
with its two constants made a variable) and that tests/test_emulated_dc_weight.py / tests/test_dc_weight_gpu.py replay: the smallest shapes at
which each path that writes a block through the engine's block evaluator -- the one place that forms a rank -- and each layout runs.

name -> (int_matrix arguments, options without the methods, methods, weights); weight None = unset (the method's own constant).
  narrow16   narrow entries, one chain per point: table_insert of k_init_pairs, the side-by-side re-evaluation and the block creation of k_iter_update
  mc12       the mc-* pair (float(count) - w dl)
  wide300    64-bit entries (more than 256 columns); again under DA4ML_HIP_MANYCOL_FROM=1
  lat16      intervals of its own, input latencies 0.1 i (no dyadic numbers) and the latency-aware cost model: dl is non-zero and no integer from the
             first step on, so the rank of k_init_pairs' blocks and the rounding of w * dl count
  search32   the default search with hard_dc=2: the forced wmc-dc and the latency retries carry the weight"""

import hashlib
import json

ONE_CHAIN = dict(decompose_dc=-1, search_all_decompose_dc=False)
N16 = 16
LAT16 = dict(
    ONE_CHAIN,
    adder_size=4,
    carry_size=8,
    qintervals=[(-(16.0 + 4 * i) * 2.0 ** -(i % 3), (15.0 + 3 * i) * 2.0 ** -(i % 3), 2.0 ** -(i % 3)) for i in range(N16)],
    latencies=[0.1 * i for i in range(N16)],
)

CASES = {
    'narrow16': ((0, 16, 16, -128, 128), ONE_CHAIN, ('wmc-pdc', 'wmc-dc'), (0.0, 0.3, 1.0, 3.3, 4.0, None, 1e6)),
    'mc12': ((24, 9, 12, -128, 128), ONE_CHAIN, ('mc-dc', 'mc-pdc'), (0.0, 0.75, 2.5, None, 1e6)),
    'wide300': ((22, 4, 300, -8, 8), ONE_CHAIN, ('wmc-dc',), (0.3, 4.0)),
    'lat16': ((0, 16, 16, -128, 128), LAT16, ('wmc-pdc', 'wmc-dc'), (0.3, 3.3)),
    'search32': ((2, 32, 32, -128, 128), dict(search_all_decompose_dc=True, hard_dc=2), (None,), (2.0,)),
}
DEFAULT_WEIGHT = {'mc-dc': 1e9, 'mc-pdc': 1e9, 'wmc-dc': 256.0, 'wmc-pdc': 256.0}


def wkey(w):
    return 'default' if w is None else repr(float(w))


def points(name):
    """[(method or None, weight or None, solve_each options, qintervals, latencies)] of a case, in record order"""
    _, opts, methods, weights = CASES[name]
    per = {k: v for k, v in opts.items() if k not in ('qintervals', 'latencies')}
    out = []
    for m in methods:
        for w in weights:
            o = dict(per, dc_weight=w)
            if m is not None:
                o.update(method0=m, method1=m)
            out.append((m, w, o, opts.get('qintervals'), opts.get('latencies')))
    return out


def digest(p):
    return hashlib.sha256(json.dumps(json.loads(json.dumps(p, default=lambda x: x.to_dict())), separators=(',', ':')).encode()).hexdigest()


def op_list(p):
    return [[op.id0, op.id1, op.opcode, op.data] for s in p.solutions for op in s.ops]


def latency_of(p):
    return float(max(p.out_latencies, default=0.0))


# matrices of the mixed call that no case has: LARGER ones of either layout, solved at their method's own weight beside smaller weighted ones
EXTRA = {'narrow40': (5, 12, 40, -128, 128), 'wide320': (23, 4, 320, -8, 8)}


def matrix_args(name):
    return CASES[name][0] if name in CASES else EXTRA[name]


def mixed_call():
    """One solve_each call that mixes methods, weights, a seed, both layouts, two problems that differ ONLY in their weight (positions 1 and 4), and in
    either layout a larger problem at its method's own weight beside smaller weighted ones (positions 10 and 11): the selection kernel has no
    weighted form, so what a launch of it is sized by must cover both.  [(matrix name, options)]"""
    one = dict(ONE_CHAIN)
    return [
        ('wide300', dict(one, method0='wmc-dc', method1='wmc-dc', dc_weight=0.3)),
        ('narrow16', dict(one, method0='wmc-pdc', method1='wmc-pdc', dc_weight=1.0)),
        ('mc12', dict(one, method0='mc-pdc', method1='mc-pdc', dc_weight=2.5)),
        ('narrow16', dict(one, method0='wmc', method1='wmc', dc_weight=3.3)),  # (wmc ignores it)
        ('narrow16', dict(one, method0='wmc-pdc', method1='wmc-pdc', dc_weight=4.0)),
        ('narrow16', dict(one, method0='wmc-pdc', method1='wmc-pdc')),
        ('mc12', dict(one, method0='mc-dc', method1='mc-dc')),
        ('narrow16', dict(one, method0='wmc-dc', method1='wmc-dc', dc_weight=0.3, seed=12345)),
        ('mc12', dict(search_all_decompose_dc=True, hard_dc=2, dc_weight=2.0)),  # (a searching solve: the forced wmc-dc, the retries, two stages)
        ('narrow16', dict(one, method0='wmc-pdc', method1='wmc-pdc', dc_weight=1.0)),  # (position 1 again: solved once, copied)
        ('narrow40', dict(one, method0='wmc-pdc', method1='wmc-pdc')),
        ('wide320', dict(one, method0='wmc-dc', method1='wmc-dc')),
    ]
