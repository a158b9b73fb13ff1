"""Golden records of wide kernels (2560 and 4095 output columns: more than the regular carve of the selection kernel's substitution block
holds) from oracle/_ref/libref.so, the reference's own sources, which spends up to minutes on each (usage: make_wide_golden.py [path]).
Writes tests/golden/wide_golden.json in the format of tall_golden.json: digest of the full result, cost, adders, ops per stage, wall time
per (shape, options).  The default search of the 2 x 4095 kernel solves a 4095 x 4095 chain in its second stage."""
import hashlib, json, sys, time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))
from cases import int_matrix  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
CASES = [
    ('2x2560_int4_seed1_single_chain', (1, 2, 2560, -8, 8), SINGLE),
    ('2x2560_int4_seed1_default', (1, 2, 2560, -8, 8), {}),
    ('2x2560_int8_seed1_single_chain', (1, 2, 2560, -128, 128), SINGLE),
    ('2x3400_int4_seed1_single_chain', (1, 2, 3400, -8, 8), SINGLE),
    ('3x4095_int4_seed1_single_chain', (1, 3, 4095, -8, 8), SINGLE),
    ('2x4095_int4_seed3_default', (3, 2, 4095, -8, 8), {}),
]

path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / 'wide_golden.json'
data = json.loads(path.read_text()) if path.exists() else {}
oracle = Oracle('ref')
for name, args, opts in CASES:
    if name in data:  # (delete a record to have it made again)
        continue
    t = time.time()
    k = int_matrix(*args)
    p = oracle.solve(k, **opts)
    dt = time.time() - t
    assert (p.kernel == k).all(), name
    dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))
    data[name] = {'sha256': hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest(), 'cost': p.cost, 'adders': p.n_adders,
                  'n_ops': [len(s.ops) for s in p.solutions], 'oracle_seconds': dt, 'matrix': list(args), 'opts': opts, 'oracle': 'oracle/_ref/libref.so'}
    path.write_text(json.dumps(data, indent=1))
    print(name, data[name], flush=True)
