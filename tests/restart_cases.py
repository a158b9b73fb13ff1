"""The restart cases that tests/golden/make_restarts_golden.py records on the emulated device and tests/test_restarts_gpu.py replays on the GPU:
name -> (int_matrix arguments, options, number of restarts, seed).  The smallest shapes at which each seeded instantiation of the loop's kernels
runs: narrow and wide entries, the many-column carve (the wide case again under DA4ML_HIP_MANYCOL_FROM=1), a searching solve."""

import hashlib
import json

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)

CASES = {
    'small16': ((0, 16, 16, -128, 128), SINGLE, 8, 1),
    'small32': ((1, 32, 32, -128, 128), SINGLE, 8, 2),
    'wide300': ((22, 4, 300, -8, 8), SINGLE, 4, 3),
    'search32': ((2, 32, 32, -128, 128), dict(search_all_decompose_dc=True, hard_dc=2), 4, 4),
}
# the mixed batch: three matrices of different widths (narrow 16x16, narrow 9x12, wide 4x300), eight seeds each -- 24 problems in one call
MIXED = {'mix16': ((0, 16, 16, -128, 128), SINGLE, 8, 1), 'mix12': ((24, 9, 12, -128, 128), SINGLE, 8, 5), 'mix300': ((22, 4, 300, -8, 8), SINGLE, 8, 3)}


def digest(p):
    return hashlib.sha256(json.dumps(json.loads(json.dumps(p, default=lambda x: x.to_dict())), separators=(',', ':')).encode()).hexdigest()


def mixed_batch():
    """(case name, restart) of the 24 problems of the mixed call: the three matrices interleaved, the unseeded restart 0 of each somewhere in the middle"""
    order = []
    for r in (3, 1, 0, 5, 2, 7, 4, 6):
        order += [('mix300', r), ('mix16', r), ('mix12', r)]
    return order
