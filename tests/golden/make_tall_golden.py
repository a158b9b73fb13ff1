"""Golden records of tall kernels (more input rows than the pair-table heuristic sized for: 768 and up) from oracle/_ref/libref.so,
the reference's own sources, for the ones too slow for a live check beside the GPU (usage: make_tall_golden.py [path]).
Writes tests/golden/tall_golden.json: digest of the full result, cost, adders, ops per stage, wall time per (shape, options)."""
import hashlib, json, sys, time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent.parent))
sys.path.insert(0, str(HERE.parent))
from cases import int_matrix  # noqa: E402
from oracle.oracle import Oracle  # noqa: E402

SINGLE = dict(method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False)
CASES = [('1024x16_int4_seed1_single_chain', (1, 1024, 16, -8, 8), SINGLE), ('1024x16_int4_seed1_default', (1, 1024, 16, -8, 8), {})]

path = Path(sys.argv[1]) if len(sys.argv) > 1 else HERE / 'tall_golden.json'
data = json.loads(path.read_text()) if path.exists() else {}
oracle = Oracle('ref')
for name, args, opts in CASES:
    t = time.time()
    p = oracle.solve(int_matrix(*args), **opts)
    dt = time.time() - t
    dump = json.loads(json.dumps(p, default=lambda o: o.to_dict()))
    data[name] = {'sha256': hashlib.sha256(json.dumps(dump, separators=(',', ':')).encode()).hexdigest(), 'cost': p.cost, 'adders': p.n_adders,
                  'n_ops': [len(s.ops) for s in p.solutions], 'oracle_seconds': dt, 'matrix': list(args), 'opts': opts, 'oracle': 'oracle/_ref/libref.so'}
    path.write_text(json.dumps(data, indent=1))
    print(name, data[name], flush=True)
