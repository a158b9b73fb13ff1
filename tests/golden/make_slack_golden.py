"""Writes tests/golden/slack_golden.json: digest, float32 cost and adders of every restart of the cases of tests/slack_cases.py, the best index of each
case, and every problem of the mixed call.

The reference has no score slack, so these records have no counterpart there.  THEIR SOURCE IS A PATCHED COPY OF THE RESTATEMENT:
oracle/cmvm_oracle.cc is copied to a temporary directory and each of its four pick functions (pick_mc, pick_mc_dc, pick_wmc, pick_wmc_dc) is
replaced by one loop over the table that takes the entry with the largest
    (entry_rank_slack(count, overlap, |latency difference|, method, weight, slack, slack_byte(id0, id1, key_index, seed)), tie_word(id0, id1, key_index, seed, order)),
rank 0 not selectable -- the product's own rank and word from da4ml_amd/csrc/cmvm_core.h and nothing else of the product: no kernel, no table, no
host code; the overlap and the latencies are the restatement's.  The digits are made a variable as tests/golden/make_recode_golden.py does (for
the case with a recoding).  The copy is never committed.  Before anything is recorded:
  * with slack 0 and seed 0 the copy must equal oracle/liboracle.so on every case and every matrix of the mixed call;
  * with slack 0 and seeds != 0 it must reproduce every digest of tests/golden/restarts_golden.json (random order) and of
    tests/golden/newest_golden.json (newest order): the rank it now compares orders the entries as the native scores did;
  * for every recorded case at least one restart's op list must differ from the same seed at slack 0, and the restarts must not all be one graph:
    a case that fails this needs a larger slack in tests/slack_cases.py.

Run from the repository root:  python tests/golden/make_slack_golden.py"""

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

import newest_cases  # noqa: E402
import numpy as np  # noqa: E402
import restart_cases  # noqa: E402
from cases import int_matrix  # noqa: E402
from make_dc_weight_golden import HEAD as W_HEAD  # noqa: E402
from make_dc_weight_golden import PATCHES as W_PATCHES  # noqa: E402
from make_dc_weight_golden import TAIL as W_TAIL  # noqa: E402
from make_newest_golden import ANCHOR  # noqa: E402
from make_newest_golden import HEAD as T_HEAD  # noqa: E402
from make_newest_golden import TAIL as T_TAIL  # noqa: E402
from make_recode_golden import DIGITS, RECODED  # noqa: E402
from make_recode_golden import HEAD as R_HEAD  # noqa: E402
from make_recode_golden import TAIL as R_TAIL  # noqa: E402
from slack_cases import CASES, MIX_MATS, SINGLE, digest, mixed_batch, op_list, restart_options  # noqa: E402

import oracle.oracle as om  # noqa: E402
from da4ml_amd._binary import RECODES, TIE_ORDERS  # noqa: E402
from da4ml_amd.cmvm import first_strict_minimum, restart_seeds  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402

HEAD = 'static uint32_t g_slack = 0;\n'
RANKED = '''
// the entry with the largest (rank, tie word) of the chain, rank 0 not selectable: what every pick function of the copy is
static PairKey orc_pick_ranked(const State &s, int method) {
    PairKey best{-1, -1, 0, false};
    uint32_t top = 0;
    uint64_t top_tie = 0;
    const float w = (method == da::M_MC_DC || method == da::M_MC_PDC) ? g_dc_weight_mc : g_dc_weight_wmc;
    for (const auto &e : s.table) {
        const PairKey &p = e.first;
        const int ov = overlap_accum(s.ops[p.id0].q, s.ops[p.id1].q).first;
        const float dl = std::abs(s.ops[p.id0].latency - s.ops[p.id1].latency);
        const int idx = da::key_index(p.shift, p.sub, s.n_bits);
        const uint32_t r = da::entry_rank_slack((uint32_t)e.second, ov, dl, method, w, g_slack, da::slack_byte((uint32_t)p.id0, (uint32_t)p.id1, idx, g_tie_seed));
        if (!r) continue;
        const uint64_t t = da::tie_word((uint32_t)p.id0, (uint32_t)p.id1, idx, g_tie_seed, g_tie_order);
        if (r > top || (r == top && t > top_tie)) {
            top = r;
            top_tie = t;
            best = p;
        }
    }
    return best;
}
'''
PICKS = {
    'pick_mc': ('const State &s', 'da::M_MC'),
    'pick_mc_dc': ('const State &s, bool absolute', 'absolute ? da::M_MC_DC : da::M_MC_PDC'),
    'pick_wmc': ('const State &s', 'da::M_WMC'),
    'pick_wmc_dc': ('const State &s, bool absolute', 'absolute ? da::M_WMC_DC : da::M_WMC_PDC'),
}
TAIL = '\nextern "C" void orc_set_slack(uint32_t slack) { g_slack = slack; }\n'


def patched_oracle(tmp: Path):
    src = (om.HERE / 'cmvm_oracle.cc').read_text()
    for old, new in (*W_PATCHES, (DIGITS, RECODED)):
        assert src.count(old) == 1, f'{old!r} occurs {src.count(old)} times in oracle/cmvm_oracle.cc'
        src = src.replace(old, new)
    assert len(re.findall(r'\nstatic PairKey pick_\w+\(', src)) == 4, 'oracle/cmvm_oracle.cc no longer has four pick functions'
    for name, (args, method) in PICKS.items():
        body = re.compile(r'\nstatic PairKey ' + name + r'\(' + re.escape(args) + r'\) \{\n.*?\n\}\n', re.S)
        assert len(body.findall(src)) == 1, name
        src = body.sub(lambda m: f'\nstatic PairKey {name}({args}) {{ return orc_pick_ranked(s, {method}); }}\n', src)
    assert src.count(ANCHOR) == 1
    # (the ranked pick stands behind overlap_accum, which it calls: the pick functions are declared ahead of it)
    src = src.replace(ANCHOR, ANCHOR + '\nstatic PairKey orc_pick_ranked(const State &s, int method);')
    assert src.count('\nstatic PairKey pick_wmc(') == 1
    src = src.replace('\nstatic PairKey pick_wmc(', RANKED + '\nstatic PairKey pick_wmc(')  # (behind overlap_accum, inside the restatement's namespace)
    (tmp / 'cmvm_oracle.cc').write_text(T_HEAD + W_HEAD + R_HEAD + HEAD + src + W_TAIL + T_TAIL + R_TAIL + TAIL)
    flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', (om.HERE / 'Makefile').read_text(), re.M).group(1).split()
    subprocess.run(['g++', *flags, '-ffp-contract=off', f'-I{ROOT / "da4ml_amd" / "csrc"}', '-shared', '-o', str(tmp / 'liboracle.so'), str(tmp / 'cmvm_oracle.cc')], check=True)
    keep, om.HERE = om.HERE, tmp  # (Oracle('port') loads HERE / liboracle.so)
    try:
        o = om.Oracle('port')
    finally:
        om.HERE = keep
    o.lib.orc_set_dc_weight.argtypes = [C.c_float]
    o.lib.orc_set_tie.argtypes = [C.c_uint64, C.c_uint32]
    o.lib.orc_set_recode.argtypes = [C.c_uint32, C.c_uint64]
    o.lib.orc_set_slack.argtypes = [C.c_uint32]
    return o


def solve_at(o, k, opts):
    """one problem with solve_each's options"""
    own = ('seed', 'tie_order', 'dc_weight', 'recode', 'recode_seed', 'slack')
    assert not opts.get('slack') or opts.get('seed'), 'a slack wants a seed'
    o.lib.orc_set_recode(RECODES[opts.get('recode', 'csd')], int(opts.get('recode_seed', 0)))
    o.lib.orc_set_tie(int(opts.get('seed', 0)), TIE_ORDERS[opts.get('tie_order', 'random')])
    o.lib.orc_set_dc_weight(-1.0 if opts.get('dc_weight') is None else float(opts['dc_weight']))
    o.lib.orc_set_slack(int(opts.get('slack', 0)))
    try:
        return o.solve(k, **{key: v for key, v in opts.items() if key not in own})
    finally:
        o.lib.orc_set_recode(0, 0)
        o.lib.orc_set_tie(0, 0)
        o.lib.orc_set_dc_weight(-1.0)
        o.lib.orc_set_slack(0)


def record(p):
    return dict(digest=digest(p), cost=pipeline_cost_f32(p), adders=p.n_adders)


def main():
    plain = om.Oracle('port')
    out = {'source': 'oracle/cmvm_oracle.cc with every pick taking the largest (entry_rank_slack, tie_word) of cmvm_core.h, rank 0 not selectable (this script)',
           'cases': {}, 'mixed': {}}  # fmt: skip
    old = json.loads((ROOT / 'tests' / 'golden' / 'restarts_golden.json').read_text())['cases']
    newest = json.loads((ROOT / 'tests' / 'golden' / 'newest_golden.json').read_text())['cases']
    with tempfile.TemporaryDirectory() as d:
        o = patched_oracle(Path(d))
        # 1. slack 0, seed 0: the restatement
        for name, (mat, opts) in {**{n: (c[0], c[1]) for n, c in CASES.items()}, **{m: (v, SINGLE) for m, v in MIX_MATS.items()}}.items():
            k = int_matrix(*mat)
            base = {key: v for key, v in opts.items() if key != 'dc_weight'}  # (the restatement has the constants only)
            assert solve_at(o, k, base) == plain.solve(k, **base), name
        # 2. slack 0, seeds != 0: the recorded restarts of both tie orders
        for name, (mat, opts, n, seed) in {**restart_cases.CASES, **restart_cases.MIXED}.items():
            k = int_matrix(*mat)
            got = [digest(solve_at(o, k, dict(opts, seed=s))) for s in restart_seeds(n, seed)]
            assert got == old[name]['digests'], f'{name}: the copy at slack 0 does not give the digests of restarts_golden.json: {[a == b for a, b in zip(got, old[name]["digests"])]}'
            print('slack 0 reproduces restarts_golden', name, flush=True)
        for name, (mat, opts, n, seed) in newest_cases.CASES.items():
            k = int_matrix(*mat)
            got = [digest(solve_at(o, k, dict(opts, seed=s, tie_order='newest'))) for s in restart_seeds(n, seed)]
            assert got == newest[name]['digests'], f'{name}: the copy at slack 0 does not give the digests of newest_golden.json: {[a == b for a, b in zip(got, newest[name]["digests"])]}'
            print('slack 0 reproduces newest_golden', name, flush=True)
        # 3. the records
        for name, (mat, opts, n, seed, slack, extra) in CASES.items():
            k = int_matrix(*mat)
            pipes = [solve_at(o, k, ro) for ro in restart_options(name)]
            flat = [solve_at(o, k, ro) for ro in restart_options(name, slack=0)]
            assert all(np.array_equal(p.kernel, k) for p in pipes), name
            assert pipes[0] == flat[0], name  # restart 0 is solve
            recs = [record(p) for p in pipes]
            moved = [op_list(a) != op_list(b) for a, b in zip(pipes, flat)]
            assert any(moved) and len({r['digest'] for r in recs}) > 1, f'{name}: slack {slack} moves no restart: raise it in tests/slack_cases.py'
            costs = [r['cost'] for r in recs]
            out['cases'][name] = dict(matrix=list(mat), opts=opts, n_restarts=n, seed=seed, slack=slack, extra=extra, seeds=[str(s) for s in restart_seeds(n, seed)],
                                      best=first_strict_minimum(costs), digests=[r['digest'] for r in recs], costs=costs, adders=[r['adders'] for r in recs],
                                      moved=moved, adders_slack0=[p.n_adders for p in flat])  # fmt: skip
            print(name, out['cases'][name]['best'], out['cases'][name]['adders'], out['cases'][name]['adders_slack0'], moved, flush=True)
        for label, mat, opts in mixed_batch():
            k = int_matrix(*mat)
            p = solve_at(o, k, opts)
            assert np.array_equal(p.kernel, k), label
            if label.startswith('plain'):
                assert p == plain.solve(k, **opts), label
            out['mixed'][label] = record(p)
            print(label, out['mixed'][label]['adders'], flush=True)
    (ROOT / 'tests' / 'golden' / 'slack_golden.json').write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
