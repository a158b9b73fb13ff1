"""Writes tests/golden/restarts_golden.json: digest and cost of every restart of the cases of tests/restart_cases.py.

The reference has no random restarts, so these records have no counterpart there: THEIR SOURCE IS THE PRODUCT'S OWN KERNELS ON THE EMULATED DEVICE
(tests/emu/libda4ml_emu.so: candidate lists of two entries, so most steps find their pick by a pass over the whole table and the others from the
lists of the step before).  What ties them to the reference: restart 0 of every case runs with seed 0, and its digest is checked here against
the reference's own sources (oracle/_ref/libref.so) -- the restatement where that build is absent; the file says which.

Run from the repository root, after the emulated library has been built (make -C tests/emu):
    DA4ML_HIP_LIB=tests/emu/libda4ml_emu.so DA4ML_HIP_UPD_BLOCKS=8 python tests/golden/make_restarts_golden.py"""

import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

from cases import int_matrix  # noqa: E402
from restart_cases import CASES, MIXED, digest  # noqa: E402

from da4ml_amd.cmvm import restart_seeds, solve_restarts  # noqa: E402
from oracle.oracle import HERE, Oracle  # noqa: E402

assert 'emu' in os.environ.get('DA4ML_HIP_LIB', ''), 'DA4ML_HIP_LIB must point at the emulated device (tests/emu/libda4ml_emu.so)'
have_ref = (HERE / '_ref' / 'libref.so').exists()
checker = Oracle('ref' if have_ref else 'port')
out = {'source': 'the kernels of da4ml_amd/csrc on the emulated device (tests/emu); the reference has no counterpart for restarts >= 1',
       'restart0_checked_against': 'the reference build (oracle/_ref/libref.so)' if have_ref else 'the restatement (oracle/cmvm_oracle.cc)', 'cases': {}}  # fmt: skip
only = sys.argv[1:]
path = ROOT / 'tests' / 'golden' / 'restarts_golden.json'
if only and path.exists():
    out['cases'] = json.loads(path.read_text())['cases']
for name, (mat, opts, n, seed) in {**CASES, **MIXED}.items():
    if only and name not in only:
        continue
    k = int_matrix(*mat)
    best, pipes, costs = solve_restarts(k, n, seed=seed, return_all=True, **opts)
    assert all((p.kernel == k).all() for p in pipes), name
    ref = checker.solve(k, **opts)
    assert digest(pipes[0]) == digest(ref), f'{name}: restart 0 is not the reference result'
    out['cases'][name] = dict(matrix=list(mat), opts=opts, n_restarts=n, seed=seed, seeds=[str(s) for s in restart_seeds(n, seed)], best=best,
                              digests=[digest(p) for p in pipes], costs=costs, adders=[p.n_adders for p in pipes])  # fmt: skip
    print(name, best, costs, flush=True)
    path.write_text(json.dumps(out, indent=1) + '\n')
