"""Digests of the reference build's results on the inputs of tests/test_oracle.py::test_port_equals_reference_build and
tests/test_dais.py::test_against_live_reference_build, so that both tests compare with the reference also where its build
(oracle/_ref/, made by oracle/Makefile from the reference sources) is absent.  Run in the build container only:

    python tests/golden/make_live_reference_golden.py

Writes tests/golden/live_reference_golden.json.gz: per case the sha256 of the complete solver result (as in make_golden.py),
of csd_decompose and of kernel_decompose for each decompose_dc, and of the DAIS interpreter's outputs (cases.array_digest)."""
import ctypes as C
import gzip, hashlib, json, sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from cases import array_digest, odd_step_case, random_case  # noqa: E402
from dais_cases import random_program  # noqa: E402
from oracle.oracle import HERE as ORACLE_DIR, Oracle  # noqa: E402

CMVM_SEEDS, ODD_STEP_SEEDS, DAIS_SEEDS = range(1000, 1060), range(40), range(1000, 1300)
DECOMPOSE_DC = (-2, -1, 0, 1, 2)


def digest(p):
    dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))
    return hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest()


def dais_case(seed):
    prog, x = random_program(seed, n_ops=int(40 + seed % 90), n_samples=40)
    return prog, np.ascontiguousarray(x)


def main():
    R = Oracle('ref')
    out = {'source': 'oracle/_ref/libref.so and oracle/_ref/libdais_ref.so (the reference sources)', 'cmvm': {}, 'odd_step': {}, 'dais': {}}
    for seed in CMVM_SEEDS:
        k, opts, _ = random_case(seed)
        out['cmvm'][str(seed)] = {'solve': digest(R.solve(k, **opts)), 'csd_decompose': array_digest(*R.csd_decompose(k)),
                                  'kernel_decompose': [array_digest(*R.kernel_decompose(k, dc)) for dc in DECOMPOSE_DC]}  # fmt: skip
    for seed in ODD_STEP_SEEDS:
        k, opts = odd_step_case(seed)
        out['odd_step'][str(seed)] = digest(R.solve(k, **opts))
    D = C.CDLL(str(ORACLE_DIR / '_ref' / 'libdais_ref.so'))
    D.dref_run.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    for seed in DAIS_SEEDS:
        prog, x = dais_case(seed)
        want = np.zeros((x.shape[0], int(prog[3])))
        assert D.dref_run(prog.ctypes.data, prog.size, x.ctypes.data, x.shape[0], want.ctypes.data) == 0
        out['dais'][str(seed)] = array_digest(want)
    with gzip.open(HERE / 'live_reference_golden.json.gz', 'wt') as f:
        json.dump(out, f, separators=(',', ':'))
    print({k: len(v) for k, v in out.items() if isinstance(v, dict)})


if __name__ == '__main__':
    main()
