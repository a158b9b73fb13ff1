"""Writes tests/golden/dc_weight_golden.json: digest, cost and latency of every case, method and weight of tests/dc_weight_cases.py, and the
front of solve_tradeoff on the narrow16 matrix as the product's kernels give it on the emulated device (tests/emu).

The reference fixes the latency-penalty weight of its -dc / -pdc selectors, so these records have no counterpart there.  THEIR SOURCE IS A PATCHED
COPY OF THE RESTATEMENT: oracle/cmvm_oracle.cc is copied to a temporary directory, its two constants (`float factor = 1e9f;` in pick_mc_dc,
`256 * std::abs(l0 - l1)` in pick_wmc_dc -- each must occur exactly once) are replaced by a variable behind an added setter, and the copy is
compiled with the oracle's own flags plus -ffp-contract=off (the multiply and the subtract of a score are rounded once each).  Before anything is
recorded the copy at the default weights must equal oracle/liboracle.so on every case.  The copy is never committed.

Run from the repository root:  python tests/golden/make_dc_weight_golden.py"""

import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
from cases import int_matrix  # noqa: E402
from dc_weight_cases import CASES, digest, latency_of, op_list, points, wkey  # noqa: E402

import oracle.oracle as om  # noqa: E402
from da4ml_amd.multi_gpu import pipeline_cost_f32  # noqa: E402

PATCHES = (
    ('float factor = 1e9f;', 'float factor = g_dc_weight_mc;'),
    ('256 * std::abs(l0 - l1)', 'g_dc_weight_wmc * std::abs(l0 - l1)'),
)
HEAD = 'static float g_dc_weight_mc = 1e9f, g_dc_weight_wmc = 256.0f;\n'
TAIL = '\nextern "C" void orc_set_dc_weight(float w) {  // negative: the constants\n    g_dc_weight_mc = w < 0 ? 1e9f : w;\n    g_dc_weight_wmc = w < 0 ? 256.0f : w;\n}\n'


def patched_oracle(tmp: Path):
    src = (om.HERE / 'cmvm_oracle.cc').read_text()
    for old, new in PATCHES:
        assert src.count(old) == 1, f'{old!r} occurs {src.count(old)} times in oracle/cmvm_oracle.cc'
        src = src.replace(old, new)
    (tmp / 'cmvm_oracle.cc').write_text(HEAD + src + TAIL)
    flags = re.search(r'^CXXFLAGS\s*\?=\s*(.*)$', (om.HERE / 'Makefile').read_text(), re.M).group(1).split()
    subprocess.run(['g++', *flags, '-ffp-contract=off', '-shared', '-o', str(tmp / 'liboracle.so'), str(tmp / 'cmvm_oracle.cc')], check=True)
    keep, om.HERE = om.HERE, tmp  # (Oracle('port') loads HERE / liboracle.so)
    try:
        o = om.Oracle('port')
    finally:
        om.HERE = keep
    o.lib.orc_set_dc_weight.argtypes = [C.c_float]
    return o


def solve_at(o, k, opts, w):
    o.lib.orc_set_dc_weight(-1.0 if w is None else float(w))
    try:
        return o.solve(k, **{key: v for key, v in opts.items() if key not in ('dc_weight', 'seed')})
    finally:
        o.lib.orc_set_dc_weight(-1.0)


def main():
    plain = om.Oracle('port')
    out = {'source': 'oracle/cmvm_oracle.cc with its two penalty constants made a variable (this script), compiled with -ffp-contract=off', 'cases': {}}
    with tempfile.TemporaryDirectory() as d:
        o = patched_oracle(Path(d))
        for name, (mat, _, _, _) in CASES.items():  # the copy at the default weights is the restatement
            k = int_matrix(*mat)
            for m, _, opts, q, l in points(name):
                full = dict(opts, **({'qintervals': q} if q is not None else {}), **({'latencies': l} if l is not None else {}))
                assert solve_at(o, k, full, None) == plain.solve(k, **{key: v for key, v in full.items() if key != 'dc_weight'}), (name, m)
        for name, (mat, _, _, _) in CASES.items():
            k = int_matrix(*mat)
            rec, lists = {}, set()
            for m, w, opts, q, l in points(name):
                full = dict(opts, **({'qintervals': q} if q is not None else {}), **({'latencies': l} if l is not None else {}))
                p = solve_at(o, k, full, w)
                assert np.array_equal(p.kernel, k), (name, m, w)
                rec.setdefault(str(m), {})[wkey(w)] = dict(digest=digest(p), cost=pipeline_cost_f32(p), latency=latency_of(p), adders=p.n_adders)
                lists.add(json.dumps(op_list(p)))
                print(name, m, wkey(w), rec[str(m)][wkey(w)]['cost'], rec[str(m)][wkey(w)]['latency'], flush=True)
            if name == 'narrow16':
                assert len(lists) >= 2, 'narrow16 gives one op list over all its weights: record (1, 32, 32, -128, 128) instead'
            out['cases'][name] = dict(matrix=list(mat), points=rec, distinct_op_lists=len(lists))
    # the front of solve_tradeoff(narrow16) with its default weights: the product's kernels on the emulated device (tests/emu), for the GPU test
    emu = ROOT / 'tests' / 'emu'
    subprocess.run(['make', '-s', '-C', str(emu)], check=True)
    r = subprocess.run([sys.executable, str(emu / 'dc_weight_worker.py'), 'tradeoff'], env=dict(os.environ, DA4ML_HIP_LIB=str(emu / 'libda4ml_emu.so'), DA4ML_HIP_UPD_BLOCKS='8'),
                       capture_output=True, text=True, cwd=str(ROOT), check=True)  # fmt: skip
    t = json.loads(r.stdout.strip().splitlines()[-1])
    assert t['kernel_ok'] and t['point0_is_solve']
    out['tradeoff_narrow16'] = dict(source='da4ml_amd.cmvm.solve_tradeoff(narrow16, **its options) on the emulated device; rows: cost, latency, method0, method1, dc_weight, digest', front=t['front'], points=t['points'])
    (ROOT / 'tests' / 'golden' / 'dc_weight_golden.json').write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
