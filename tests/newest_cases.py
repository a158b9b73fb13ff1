"""The cases of the newest-row-first tie order (order='newest' of da4ml_amd.cmvm.solve_restarts, 'tie_order' of _binary.solve_each) that
tests/golden/make_newest_golden.py records with a patched copy of the restatement and that tests/test_emulated_newest.py / tests/test_newest_gpu.py
replay: name -> (int_matrix arguments, options, number of restarts, seed).  The smallest shapes at which each seeded instantiation of the
loop's kernels runs: narrow and wide entries, the many-column carve (the wide case again under DA4ML_HIP_MANYCOL_FROM=1), a searching solve,
and the two selectors whose ranks are formed another way (mc: the bare count; wmc-dc: a float score with a latency penalty)."""

import hashlib
import json

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)


def single(method):
    return dict(SINGLE, method0=method, method1=method)


CASES = {
    'small16': ((0, 16, 16, -128, 128), SINGLE, 8, 1),
    'small32': ((1, 32, 32, -128, 128), SINGLE, 8, 2),
    'wide300': ((22, 4, 300, -8, 8), SINGLE, 4, 3),
    'search32': ((2, 32, 32, -128, 128), dict(search_all_decompose_dc=True, hard_dc=2), 4, 4),
    'mc16': ((0, 16, 16, -128, 128), single('mc'), 4, 5),
    'wmcdc16': ((0, 16, 16, -128, 128), single('wmc-dc'), 4, 6),
}
NARROW = ('small16', 'small32')  # the chains that run again under other table geometries
MANYCOL = 'wide300'  # ... and under DA4ML_HIP_MANYCOL_FROM=1

# The mixed call: chains of every kind side by side, widths and kinds scrambled.  (label, int_matrix arguments, solve_each options); the seeds of the
# random-order problems are restarts of tests/restart_cases.py MIXED, so their records are those of tests/golden/restarts_golden.json
# (label 'random:<case>:<restart>'); 'plain:*' are unseeded; 'newest:*' and the weighted 'newest-w:*' are recorded in newest_golden.json under 'mixed'.
MIX_MATS = {'mix16': (0, 16, 16, -128, 128), 'mix12': (24, 9, 12, -128, 128), 'mix300': (22, 4, 300, -8, 8)}
MIX_RANDOM_SEED = {'mix16': 1, 'mix12': 5, 'mix300': 3}  # restart_cases.MIXED
WEIGHTED = dict(single('wmc-dc'), dc_weight=3.3)


def mixed_batch():
    from da4ml_amd.cmvm import restart_seeds

    out = []
    for r, mat in ((3, 'mix300'), (1, 'mix16'), (0, 'mix12'), (2, 'mix16'), (1, 'mix300'), (3, 'mix12'), (0, 'mix16'), (2, 'mix12'), (0, 'mix300')):
        s = restart_seeds(8, MIX_RANDOM_SEED[mat])[r]
        if r == 0:
            out.append((f'plain:{mat}', MIX_MATS[mat], dict(SINGLE, tie_order='newest')))  # seed 0: the reference whatever the order says
        else:
            out.append((f'newest:{mat}:{r}', MIX_MATS[mat], dict(SINGLE, seed=s, tie_order='newest')))
            out.append((f'random:{mat}:{r}', MIX_MATS[mat], dict(SINGLE, seed=s)))
        if (r, mat) == (2, 'mix16'):
            out.append((f'newest-w:{mat}:{r}', MIX_MATS[mat], dict(WEIGHTED, seed=s, tie_order='newest')))
    return out


def digest(p):
    return hashlib.sha256(json.dumps(json.loads(json.dumps(p, default=lambda x: x.to_dict())), separators=(',', ':')).encode()).hexdigest()


def op_list(p):
    return [[op.id0, op.id1, op.opcode, op.data] for s in p.solutions for op in s.ops]
