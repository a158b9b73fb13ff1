"""The cases of the score slack (slack= of da4ml_amd.cmvm.solve_restarts, 'slack' of _binary.solve_each, da_solve_batch_search) that
tests/golden/make_slack_golden.py records with a patched copy of the restatement and that tests/test_emulated_slack.py / tests/test_slack_gpu.py
replay: name -> (int_matrix arguments, options, number of restarts, seed, slack, what else the restarts r >= 1 get).  The restarts of a case are
those of solve_restarts(kernel, n, seed, slack=slack): restart 0 is solve, restart r >= 1 runs with the tie seed restart_seeds(n, seed)[r] and the
slack.  The smallest shapes at which each slack instantiation of the loop's kernels runs: narrow and wide entries, the many-column carve (the
wide case again under DA4ML_HIP_MANYCOL_FROM=1), a searching solve with a latency budget (both stages, every candidate, the retries), the
selectors whose ranks are formed another way (mc: the bare count; wmc-dc: a float score with a latency penalty, on its constant and on another
weight), the newest-first tie order and a recoding under the slack."""

import hashlib
import json

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)


def single(method, **more):
    return dict(SINGLE, method0=method, method1=method, **more)


CASES = {
    'small16': ((0, 16, 16, -128, 128), SINGLE, 8, 1, 16, {}),
    'small32': ((1, 32, 32, -128, 128), SINGLE, 8, 2, 16, {}),
    'wide300': ((22, 4, 300, -8, 8), SINGLE, 4, 3, 16, {}),
    'search32': ((2, 32, 32, -128, 128), dict(search_all_decompose_dc=True, hard_dc=2), 4, 4, 16, {}),
    'mc16': ((0, 16, 16, -128, 128), single('mc'), 4, 5, 128, {}),  # (counts of a 16x16 matrix stay below 20: a smaller slack discounts none of them)
    'wmcdc16': ((0, 16, 16, -128, 128), single('wmc-dc'), 4, 6, 16, {}),
    'wmcdcw16': ((0, 16, 16, -128, 128), single('wmc-dc', dc_weight=3.3), 4, 7, 16, {}),
    'newest16': ((0, 16, 16, -128, 128), SINGLE, 4, 8, 16, dict(tie_order='newest')),
    'compact16': ((0, 16, 16, -128, 128), SINGLE, 4, 9, 16, dict(recode='compact')),
}
NARROW = ('small16', 'small32')  # the chains that run again under other table geometries
MANYCOL = 'wide300'  # ... and under DA4ML_HIP_MANYCOL_FROM=1


def restart_options(name, slack=None):
    """solve_each's options of the restarts of a case (with another slack than the case's: 0 gives the plain restarts of the same seeds)"""
    from da4ml_amd.cmvm import restart_seeds

    _, opts, n, seed, case_slack, extra = CASES[name]
    slack = case_slack if slack is None else slack
    out = []
    for s in restart_seeds(n, seed):
        o = dict(opts)
        if s:
            o.update(seed=s, **extra)
            if extra.get('recode') == 'seeded':
                o['recode_seed'] = s
            if slack:
                o['slack'] = slack
        out.append(o)
    return out


# The mixed call: unseeded chains, seeded chains without a slack and slack chains at two slacks side by side, widths and kinds scrambled.
# (label, int_matrix arguments, solve_each options); every label is recorded in slack_golden.json under 'mixed'.
MIX_MATS = {'mix16': (0, 16, 16, -128, 128), 'mix12': (24, 9, 12, -128, 128), 'mix300': (22, 4, 300, -8, 8)}


def mixed_batch():
    from da4ml_amd.cmvm import restart_seeds

    s = restart_seeds(8, 21)
    return [
        ('slack16:mix300', MIX_MATS['mix300'], dict(SINGLE, seed=s[1], slack=16)),
        ('seeded:mix16', MIX_MATS['mix16'], dict(SINGLE, seed=s[2])),
        ('plain:mix12', MIX_MATS['mix12'], dict(SINGLE)),
        ('slack5:mix16', MIX_MATS['mix16'], dict(SINGLE, seed=s[2], slack=5)),
        ('slack16:mix16', MIX_MATS['mix16'], dict(SINGLE, seed=s[2], slack=16)),
        ('slack16-newest-w:mix16', MIX_MATS['mix16'], dict(single('wmc-dc', dc_weight=3.3), seed=s[3], slack=16, tie_order='newest')),
        ('seeded:mix300', MIX_MATS['mix300'], dict(SINGLE, seed=s[1])),
        ('slack5:mix12', MIX_MATS['mix12'], dict(SINGLE, seed=s[4], slack=5)),
        ('plain:mix300', MIX_MATS['mix300'], dict(SINGLE)),
        ('slack5:mix300', MIX_MATS['mix300'], dict(SINGLE, seed=s[5], slack=5)),
        ('slack16:mix12', MIX_MATS['mix12'], dict(SINGLE, seed=s[4], slack=16)),
        ('plain:mix16', MIX_MATS['mix16'], dict(SINGLE)),
    ]


def digest(p):
    return hashlib.sha256(json.dumps(json.loads(json.dumps(p, default=lambda x: x.to_dict())), separators=(',', ':')).encode()).hexdigest()


def op_list(p):
    return [[op.id0, op.id1, op.opcode, op.data] for s in p.solutions for op in s.ops]
