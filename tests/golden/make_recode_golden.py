"""Writes tests/golden/recode_golden.json: digest, float32 cost and adders of every point of the cases of tests/recode_cases.py, and of every
problem of the mixed call.

The reference always starts from the CSD digits, so these records have no counterpart there.  THEIR SOURCE IS A PATCHED COPY OF THE
RESTATEMENT: oracle/cmvm_oracle.cc is copied to a temporary directory and its csd_decompose post-processes the digits of every entry with
    digit_masks(x, mode, seed)
-- the product's own recoding from da4ml_amd/csrc/cmvm_core.h and nothing else of the product: no kernel, no table, no host code.  Under mode CSD
the copy does not even take the digits from it: it checks that they are the digits the restatement formed itself.  The tie word and the penalty
constants are made variables as tests/golden/make_newest_golden.py does (for the newest-order and the weighted chain of the mixed call).  The copy
is never committed.  Before anything is recorded:
  * the copy in mode CSD must equal oracle/liboracle.so on every case and every matrix of the mixed call;
  * pipeline.kernel == kernel must hold for every record;
  * the COMPACT adder counts of 32x32 3-bit single wmc chains (seeds 0, 1, 2) must be 579, 590, 578 and solve's 593, 598, 595: the figures the
    scan rule was measured with.  Other figures mean another rule than the one cmvm_core.h states.

Run from the repository root:  python tests/golden/make_recode_golden.py"""

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
from cases import int_matrix  # noqa: E402
from make_dc_weight_golden import HEAD as W_HEAD  # noqa: E402
from make_dc_weight_golden import PATCHES as W_PATCHES  # noqa: E402
from make_dc_weight_golden import TAIL as W_TAIL  # noqa: E402
from make_newest_golden import ANCHOR, HELPERS, PICK  # noqa: E402
from make_newest_golden import HEAD as T_HEAD  # noqa: E402
from make_newest_golden import TAIL as T_TAIL  # noqa: E402
from recode_cases import CASES, MIX_MATS, SINGLE, digest, mixed_batch, points  # noqa: E402

import oracle.oracle as om  # noqa: E402
from da4ml_amd._binary import RECODES, TIE_ORDERS  # noqa: E402
from da4ml_amd.cmvm import first_strict_minimum  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402

DIGITS = '    for (size_t k = 0; k < a.size(); ++k) csd_digits(xi[k], N, &csd[k * N]);\n'
RECODED = '''    for (size_t k = 0; k < a.size(); ++k) {
        csd_digits(xi[k], N, &csd[k * N]);
        uint32_t plus, minus;
        da::digit_masks(xi[k], g_recode_mode, g_recode_seed, plus, minus);
        if ((uint64_t)(plus | minus) >> N) throw std::runtime_error("digit_masks raised the top position");
        int64_t value = 0;
        for (int b = 0; b < N; ++b) {
            const int8_t d = (int8_t)((int)((plus >> b) & 1u) - (int)((minus >> b) & 1u));
            if (g_recode_mode == 0) {
                if (csd[k * N + b] != d) throw std::runtime_error("mode CSD is not the restatement's digits");
            } else
                csd[k * N + b] = d;
            value += (int64_t)d << b;
        }
        if (value != (int64_t)xi[k]) throw std::runtime_error("digit_masks changed a value");
    }
'''
HEAD = 'static uint32_t g_recode_mode = 0;\nstatic uint64_t g_recode_seed = 0;\n'
TAIL = '\nextern "C" void orc_set_recode(uint32_t mode, uint64_t seed) {\n    g_recode_mode = mode;\n    g_recode_seed = seed;\n}\n'
TABLE_32x32_3BIT = {0: (593, 579), 1: (598, 590), 2: (595, 578)}  # seed -> (solve, COMPACT) adders of a single wmc chain


def patched_oracle(tmp: Path):
    src = (om.HERE / 'cmvm_oracle.cc').read_text()
    for old, new in (*W_PATCHES, (DIGITS, RECODED)):
        assert src.count(old) == 1, f'{old!r} occurs {src.count(old)} times in oracle/cmvm_oracle.cc'
        src = src.replace(old, new)
    assert len(PICK.findall(src)) == 4, 'oracle/cmvm_oracle.cc no longer has four pick functions of the shape this script patches'
    src = PICK.sub(lambda m: f'if ({m.group(1)} > top || ({m.group(1)} == top && orc_tie_after(s, e.first, best))) {{', src)
    assert src.count(ANCHOR) == 1
    src = src.replace(ANCHOR, HELPERS + ANCHOR)
    (tmp / 'cmvm_oracle.cc').write_text(T_HEAD + W_HEAD + HEAD + src + W_TAIL + T_TAIL + TAIL)
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
    return o


def solve_at(o, k, opts):
    """one problem with solve_each's options"""
    own = ('seed', 'tie_order', 'dc_weight', 'recode', 'recode_seed')
    o.lib.orc_set_recode(RECODES[opts.get('recode', 'csd')], int(opts.get('recode_seed', 0)))
    o.lib.orc_set_tie(int(opts.get('seed', 0)), TIE_ORDERS[opts.get('tie_order', 'random')])
    o.lib.orc_set_dc_weight(-1.0 if opts.get('dc_weight') is None else float(opts['dc_weight']))
    try:
        return o.solve(k, **{key: v for key, v in opts.items() if key not in own})
    finally:
        o.lib.orc_set_recode(0, 0)
        o.lib.orc_set_tie(0, 0)
        o.lib.orc_set_dc_weight(-1.0)


def record(p):
    return dict(digest=digest(p), cost=pipeline_cost_f32(p), adders=p.n_adders)


def main():
    plain = om.Oracle('port')
    out = {'source': 'oracle/cmvm_oracle.cc with csd_decompose post-processing the digits of every entry with digit_masks(x, mode, seed) of cmvm_core.h (this script)',
           'cases': {}, 'mixed': {}}  # fmt: skip
    with tempfile.TemporaryDirectory() as d:
        o = patched_oracle(Path(d))
        # 1. mode CSD is the restatement (and the recoding's CSD digits are the restatement's: checked inside the copy, entry by entry)
        for name, (mat, opts) in {**{n: (c[0], c[1]) for n, c in CASES.items()}, **{m: (v, SINGLE) for m, v in MIX_MATS.items()}}.items():
            k = int_matrix(*mat)
            assert solve_at(o, k, dict(opts, recode='csd', recode_seed=12345)) == plain.solve(k, **opts), name
        # 2. the scan rule is the one that was measured
        for s, (want_plain, want_compact) in TABLE_32x32_3BIT.items():
            k = int_matrix(s, 32, 32, -4, 4)
            got = (solve_at(o, k, SINGLE).n_adders, solve_at(o, k, dict(SINGLE, recode='compact')).n_adders)
            assert got == (want_plain, want_compact), f'32x32 3 bit seed {s}: (solve, COMPACT) adders {got}, measured with the stated rule: {(want_plain, want_compact)}'
            print('32x32 3 bit, seed', s, got, flush=True)
        # 3. the records
        for name, (mat, opts, n, seed) in CASES.items():
            k = int_matrix(*mat)
            pts = points(n, seed)
            pipes = [solve_at(o, k, dict(opts, recode=mode, recode_seed=rs)) for mode, rs in pts]
            assert all(np.array_equal(p.kernel, k) for p in pipes), name
            recs = [record(p) for p in pipes]
            costs = [r['cost'] for r in recs]
            out['cases'][name] = dict(matrix=list(mat), opts=opts, n=n, seed=seed, points=[[mode, str(rs)] for mode, rs in pts], best=first_strict_minimum(costs),
                                      digests=[r['digest'] for r in recs], costs=costs, adders=[r['adders'] for r in recs])  # fmt: skip
            print(name, out['cases'][name]['best'], out['cases'][name]['adders'], flush=True)
        for label, mat, opts in mixed_batch():
            k = int_matrix(*mat)
            p = solve_at(o, k, opts)
            assert np.array_equal(p.kernel, k), label
            if label.startswith('plain'):
                assert p == plain.solve(k, **{key: v for key, v in opts.items() if key not in ('recode', 'recode_seed')}), label
            out['mixed'][label] = record(p)
            print(label, out['mixed'][label]['adders'], flush=True)
    (ROOT / 'tests' / 'golden' / 'recode_golden.json').write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
