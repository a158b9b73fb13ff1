"""The cases of the digit recodings (da4ml_amd.cmvm.solve_recoded, 'recode' / 'recode_seed' of _binary.solve_each, da_solve_batch_recode) that
tests/golden/make_recode_golden.py records with a patched copy of the restatement and that tests/test_emulated_recode.py / tests/test_recode_gpu.py
replay: name -> (int_matrix arguments, options, number of points, seed).  The points of a case are those of solve_recoded(kernel, n, seed): point 0
is solve, point 1 COMPACT, the others SEEDED with restart_seeds(n, seed).  The smallest shapes that reach each code path: narrow cells in a
single chain (3 and 4 bit), 8-bit entries, wide cells and the many-column carve (the wide case again under DA4ML_HIP_MANYCOL_FROM=1), a searching
solve with a latency budget (both stages, every decompose_dc candidate, the minimal latency and the retries), and the two selectors whose ranks
are formed another way (mc, wmc-dc)."""

import hashlib
import json

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)


def single(method):
    return dict(SINGLE, method0=method, method1=method)


CASES = {
    'small16': ((0, 16, 16, -4, 4), SINGLE, 4, 1),
    'small32': ((1, 32, 32, -8, 8), SINGLE, 4, 2),
    'bits8': ((24, 9, 12, -128, 128), SINGLE, 4, 3),
    'wide300': ((22, 4, 300, -8, 8), SINGLE, 4, 4),
    'search32': ((2, 32, 32, -4, 4), dict(search_all_decompose_dc=True, hard_dc=2), 4, 5),
    'mc16': ((0, 16, 16, -4, 4), single('mc'), 3, 6),
    'wmcdc16': ((0, 16, 16, -4, 4), single('wmc-dc'), 3, 7),
}
NARROW = ('small16', 'small32')  # the chains that run again under other table geometries
MANYCOL = 'wide300'  # ... and under DA4ML_HIP_MANYCOL_FROM=1

# The mixed call: plain, COMPACT and SEEDED chains, a SEEDED one with a tie seed in the newest order and a weighted COMPACT one side by side, widths
# and kinds scrambled.  (label, int_matrix arguments, solve_each options); every label is recorded in recode_golden.json under 'mixed'.
MIX_MATS = {'mix16': (0, 16, 16, -4, 4), 'mix12': (24, 9, 12, -128, 128), 'mix300': (22, 4, 300, -8, 8)}
WEIGHTED = dict(single('wmc-dc'), dc_weight=3.3)


def mixed_batch():
    from da4ml_amd.cmvm import restart_seeds

    s = restart_seeds(8, 11)
    return [
        ('seeded:mix300', MIX_MATS['mix300'], dict(SINGLE, recode='seeded', recode_seed=s[1])),
        ('compact:mix16', MIX_MATS['mix16'], dict(SINGLE, recode='compact')),
        ('plain:mix12', MIX_MATS['mix12'], dict(SINGLE)),
        ('seeded-newest:mix16', MIX_MATS['mix16'], dict(SINGLE, recode='seeded', recode_seed=s[2], seed=s[3], tie_order='newest')),
        ('compact:mix300', MIX_MATS['mix300'], dict(SINGLE, recode='compact')),
        ('compact-w:mix16', MIX_MATS['mix16'], dict(WEIGHTED, recode='compact')),
        ('seeded:mix12', MIX_MATS['mix12'], dict(SINGLE, recode='seeded', recode_seed=s[4])),
        ('plain:mix300', MIX_MATS['mix300'], dict(SINGLE, recode='csd', recode_seed=s[5])),  # CSD reads no seed: solve itself
        ('compact:mix12', MIX_MATS['mix12'], dict(SINGLE, recode='compact', recode_seed=s[6])),  # nor does COMPACT
        ('seeded:mix16', MIX_MATS['mix16'], dict(SINGLE, recode='seeded', recode_seed=s[1])),
        ('plain:mix16', MIX_MATS['mix16'], dict(SINGLE)),
    ]


def points(n, seed):
    """(recode, recode_seed) of the n points of solve_recoded(kernel, n, seed)"""
    from da4ml_amd.cmvm import restart_seeds

    s = restart_seeds(n, seed)
    return [('csd', 0)] + [('compact', 0) if r == 1 else ('seeded', s[r]) for r in range(1, n)]


def digest(p):
    return hashlib.sha256(json.dumps(json.loads(json.dumps(p, default=lambda x: x.to_dict())), separators=(',', ':')).encode()).hexdigest()


def op_list(p):
    return [[op.id0, op.id1, op.opcode, op.data] for s in p.solutions for op in s.ops]
