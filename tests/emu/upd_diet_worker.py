"""Worker of tests/test_upd_counts_emulated.py (DA4ML_HIP_LIB = tests/emu/libda4ml_emu.so: the kernels on the CPU) and of the fresh child processes of
tests/test_upd_counts_gpu.py (the product's library on the GPU, under the environment the test sets): the groups of tests/upd_diet_cases.py as one wmc
chain each, whole Pipeline against the oracle.  One JSON line on stdout.  usage: upd_diet_worker.py <group> [<group> ...]"""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / 'tests'))

import numpy as np  # noqa: E402
from cases import int_matrix  # noqa: E402
from upd_diet_cases import GROUPS, SINGLE, self_pairs  # noqa: E402

from da4ml_amd import _binary as hip  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


def main(groups):
    o = Oracle('port')
    bad, add, sub, n = [], 0, 0, 0
    for g in groups:
        for mat in GROUPS[g]:
            k = int_matrix(*mat)
            got, want = hip.solve(k, **SINGLE), o.solve(k, **SINGLE)
            if got != want or not np.all(got.kernel == k):
                bad.append([g, list(mat)])
            a, s = self_pairs(want)
            add, sub, n = add + a, sub + s, n + 1
    t = hip.timings()
    print(json.dumps(dict(bad=bad, n=n, self_add=add, self_sub=sub, retries=t['retries'], partners_per_step=t['partners'] / max(t['iterations'], 1))), flush=True)


if __name__ == '__main__':
    main(sys.argv[1:])
