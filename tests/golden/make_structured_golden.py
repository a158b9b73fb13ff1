"""Golden records for the STRUCTURED matrices (cases.STRUCTURED at their medium sizes: all-ones, one value in every cell,
duplicate / negated / doubled rows and columns, ternary, rank 1, Toeplitz, checkerboards of zeros, one-hot rows), produced by the
reference's own sources (oracle/_ref/libref.so).  Run in the build container only:

    python tests/golden/make_structured_golden.py

Every family under the five option sets of cases.STRUCTURED_OPTS.  A record holds the case, the options, the cost, the
number of ops per stage and the sha256 digest of the complete result (every op's ids, opcode, shift, interval, latency,
cost; all output indices / shifts / signs) -- data only."""
import gzip, hashlib, json, sys, time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))

from cases import STRUCTURED, STRUCTURED_OPTS, structured_matrix  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402


def digest(p):
    dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))
    return hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest()


def main():
    R = Oracle('ref')
    out = {'source': 'oracle/_ref/libref.so = the reference build', 'digests': []}
    t0 = time.time()
    for name in STRUCTURED:
        k = structured_matrix(name)
        for oname, opts in STRUCTURED_OPTS.items():
            t1 = time.time()
            p = R.solve(k, **opts)
            out['digests'].append({'case': f'{name}/{oname}', 'shape': list(k.shape), 'kernel_sha256': hashlib.sha256(k.tobytes()).hexdigest(),
                                   'opts': opts, 'sha256': digest(p), 'cost': p.cost, 'n_ops': [len(s.ops) for s in p.solutions]})  # fmt: skip
            print(f'{name}/{oname}: cost {p.cost} ops {out["digests"][-1]["n_ops"]} {time.time() - t1:.2f} s', flush=True)
    with gzip.open(HERE / 'structured_golden.json.gz', 'wt') as f:
        json.dump(out, f, separators=(',', ':'))
    print('digests', len(out['digests']), f'{time.time() - t0:.0f} s')


if __name__ == '__main__':
    main()
