"""Writes tests/golden/newest_golden.json: digest, float32 cost and adders of every restart of the cases of tests/newest_cases.py in the newest-row-first
tie order, the best index of each case, and the newest-order problems of the mixed call.

The reference has no seeded tie order, so these records have no counterpart there.  THEIR SOURCE IS A PATCHED COPY OF THE RESTATEMENT:
oracle/cmvm_oracle.cc is copied to a temporary directory and every pick function (the four `if (score >= top)` of pick_mc, pick_mc_dc, pick_wmc,
pick_wmc_dc -- there must be exactly four) takes, among entries of equal score, the one with the largest
    tie_word(id0, id1, key_index(shift, sub, n_bits), seed, order)
-- the product's own word function from da4ml_amd/csrc/cmvm_core.h and nothing else of the product: no kernel, no table, no host code.  The two
penalty constants are made a variable as tests/golden/make_dc_weight_golden.py does (for the weighted chain of the mixed call).  The copy is
never committed.  Before anything is recorded:
  * the copy at seed 0 must equal oracle/liboracle.so on every case, under both orders;
  * the copy in the RANDOM order must reproduce every digest of tests/golden/restarts_golden.json.  Those came from the product's kernels on the
    emulated device: this is their first independent pin, and it shows that restatement and engine number their rows alike on every path the
    cases take (a difference would show as a digest that does not come back, and stops the script).

Run from the repository root:  python tests/golden/make_newest_golden.py"""

import ctypes as C
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))
sys.path.insert(0, str(ROOT / 'tests' / 'golden'))

import numpy as np  # noqa: E402
import restart_cases  # noqa: E402
from cases import int_matrix  # noqa: E402
from make_dc_weight_golden import HEAD as W_HEAD  # noqa: E402
from make_dc_weight_golden import PATCHES as W_PATCHES  # noqa: E402
from make_dc_weight_golden import TAIL as W_TAIL  # noqa: E402
from newest_cases import CASES, MIX_MATS, digest, mixed_batch  # noqa: E402

import oracle.oracle as om  # noqa: E402
from da4ml_amd._binary import TIE_ORDERS  # noqa: E402
from da4ml_amd.cmvm import first_strict_minimum, restart_seeds  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402

PICK = re.compile(r'if \((score|e\.second) >= top\) \{')
ANCHOR = 'static const PairKey NO_PAIR{-1, -1, 0, false};'
HEAD = '#include "cmvm_core.h"\nstatic uint64_t g_tie_seed = 0;\nstatic uint32_t g_tie_order = 0;\n'
HELPERS = '''
static uint64_t orc_tie_word(const State &s, const PairKey &p) {
    return da::tie_word((uint32_t)p.id0, (uint32_t)p.id1, da::key_index(p.shift, p.sub, s.n_bits), g_tie_seed, g_tie_order);
}
// `a` comes after `b` in the chain's tie order (anything comes after "no pair yet")
static bool orc_tie_after(const State &s, const PairKey &a, const PairKey &b) { return b.id0 < 0 || orc_tie_word(s, a) > orc_tie_word(s, b); }
'''
TAIL = '\nextern "C" void orc_set_tie(uint64_t seed, uint32_t order) {\n    g_tie_seed = seed;\n    g_tie_order = order;\n}\n'


def patched_oracle(tmp: Path):
    src = (om.HERE / 'cmvm_oracle.cc').read_text()
    for old, new in W_PATCHES:
        assert src.count(old) == 1, f'{old!r} occurs {src.count(old)} times in oracle/cmvm_oracle.cc'
        src = src.replace(old, new)
    assert len(PICK.findall(src)) == 4, 'oracle/cmvm_oracle.cc no longer has four pick functions of the shape this script patches'
    src = PICK.sub(lambda m: f'if ({m.group(1)} > top || ({m.group(1)} == top && orc_tie_after(s, e.first, best))) {{', src)
    assert src.count(ANCHOR) == 1
    src = src.replace(ANCHOR, HELPERS + ANCHOR)
    (tmp / 'cmvm_oracle.cc').write_text(HEAD + W_HEAD + src + W_TAIL + TAIL)
    flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', (om.HERE / 'Makefile').read_text(), re.M).group(1).split()
    subprocess.run(['g++', *flags, '-ffp-contract=off', f'-I{ROOT / "da4ml_amd" / "csrc"}', '-shared', '-o', str(tmp / 'liboracle.so'), str(tmp / 'cmvm_oracle.cc')], check=True)
    keep, om.HERE = om.HERE, tmp  # (Oracle('port') loads HERE / liboracle.so)
    try:
        o = om.Oracle('port')
    finally:
        om.HERE = keep
    o.lib.orc_set_dc_weight.argtypes = [C.c_float]
    o.lib.orc_set_tie.argtypes = [C.c_uint64, C.c_uint32]
    return o


def solve_at(o, k, opts, seed, order, weight=None):
    o.lib.orc_set_tie(int(seed), TIE_ORDERS[order])
    o.lib.orc_set_dc_weight(-1.0 if weight is None else float(weight))
    try:
        return o.solve(k, **opts)
    finally:
        o.lib.orc_set_tie(0, 0)
        o.lib.orc_set_dc_weight(-1.0)


def record(p):
    return dict(digest=digest(p), cost=pipeline_cost_f32(p), adders=p.n_adders)


def main():
    plain = om.Oracle('port')
    out = {'source': 'oracle/cmvm_oracle.cc with every pick taking the largest tie_word(id0, id1, key_index, seed, order) of cmvm_core.h among equal scores (this script)',
           'cases': {}, 'mixed': {}}  # fmt: skip
    old = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']
    with tempfile.TemporaryDirectory() as d:
        o = patched_oracle(Path(d))
        # 1. seed 0 is the restatement, whatever the order says
        for name, (mat, opts, _, _) in {**CASES, **{m: (v, restart_cases.SINGLE, 0, 0) for m, v in MIX_MATS.items()}}.items():
            k = int_matrix(*mat)
            want = plain.solve(k, **opts)
            for order in TIE_ORDERS:
                assert solve_at(o, k, opts, 0, order) == want, (name, order)
        # 2. the random order gives the recorded restarts of the emulated device
        for name, (mat, opts, n, seed) in {**restart_cases.CASES, **restart_cases.MIXED}.items():
            k = int_matrix(*mat)
            got = [digest(solve_at(o, k, opts, s, 'random')) for s in restart_seeds(n, seed)]
            assert got == old[name]['digests'], f'{name}: the restatement in the random order does not give the digests of restarts_golden.json: {[a == b for a, b in zip(got, old[name]["digests"])]}'
            print('random order reproduces', name, flush=True)
        # 3. the records
        for name, (mat, opts, n, seed) in CASES.items():
            k = int_matrix(*mat)
            seeds = restart_seeds(n, seed)
            pipes = [solve_at(o, k, opts, s, 'newest') for s in seeds]
            assert all(np.array_equal(p.kernel, k) for p in pipes), name
            recs = [record(p) for p in pipes]
            costs = [r['cost'] for r in recs]
            out['cases'][name] = dict(matrix=list(mat), opts=opts, n_restarts=n, seed=seed, seeds=[str(s) for s in seeds], best=first_strict_minimum(costs),
                                      digests=[r['digest'] for r in recs], costs=costs, adders=[r['adders'] for r in recs])  # fmt: skip
            print(name, out['cases'][name]['best'], costs, flush=True)
        for label, mat, opts in mixed_batch():
            if not label.startswith('newest'):
                continue
            k = int_matrix(*mat)
            p = solve_at(o, k, {key: v for key, v in opts.items() if key not in ('seed', 'tie_order', 'dc_weight')}, opts['seed'], 'newest', opts.get('dc_weight'))
            assert np.array_equal(p.kernel, k), label
            out['mixed'][label] = record(p)
            print(label, out['mixed'][label]['cost'], flush=True)
    (ROOT / 'tests' / 'golden' / 'newest_golden.json').write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
