"""Throughput of the compiled DAIS executables against the one-shot device executor:  python tools/dais_exec_bench.py [samples] [repeats] [n ...]

For stage 0 of the seed-0 n x n int8 `wmc` single-chain solve (n = 64 and 256 by default), samples/s of
  (a) CombLogic.predict(executor='device')  -- the one-shot call: program built, decoded, slot-assigned, buffers allocated per call;
  (b) the compiled handle on the same host arrays (DA_DAIS_DEVICE: staged in tiles through the handle's buffers);
  (c) the compiled handle on torch tensors that live on the device (DA_DAIS_DEVICE_RESIDENT), synchronised for the timing.
Two warm-up rounds, then `repeats` rounds that run (a), (b), (c) one after the other, so that drift hits all three alike; printed:
median and [min, max] of the rounds, and the ratios of the medians.  Results are checked against the matrix product."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tests'))
import torch  # noqa: E402
from cases import int_matrix  # noqa: E402

from da4ml_amd.cmvm import solve  # noqa: E402

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 10**6
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(v) for v in sys.argv[3:]] or [64, 256]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, y


for n in sizes:
    stage = solve(int_matrix(0, n, n, -128, 128), method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False).solutions[0]
    x = np.random.default_rng(0).integers(-128, 128, (samples, n)).astype(np.float64)
    want = x @ stage.kernel.astype(np.float64)
    xd = torch.from_numpy(x).cuda()
    ex = stage.compile()
    out_d = torch.empty((samples, stage.shape[1]), dtype=torch.float64, device='cuda')
    out_h = np.zeros((samples, stage.shape[1]))
    runs = {
        'a one-shot predict, host arrays': lambda: stage.predict(x, executor='device'),
        'b handle, host arrays': lambda: ex(x, out=out_h, executor='device'),
        'c handle, device tensors': lambda: ex(xd, out=out_d),
    }
    times = {k: [] for k in runs}
    for r in range(2 + repeats):
        for name, fn in runs.items():
            dt, y = timed(fn)
            if r == 0:
                assert np.array_equal(y.cpu().numpy() if hasattr(y, 'cpu') else y, want), name
            if r >= 2:
                times[name].append(dt)
    info = ex.info
    print(f'{n}x{n} stage 0: {info["n_ops"]} statements, {info["n_slots"]} slots = {info["regfile_bytes_per_sample"]} B of register file per sample, '
          f'{samples} samples, {repeats} rounds', flush=True)
    med = {}
    for name, ts in times.items():
        med[name] = statistics.median(ts)
        print(f'  ({name}): median {samples / med[name]:.3e} samples/s  [{samples / max(ts):.3e}, {samples / min(ts):.3e}]  {med[name] * 1e3:.1f} ms', flush=True)
    a, b, c = (med[k] for k in runs)
    print(f'  b/a = {a / b:.2f}x, c/a = {a / c:.2f}x, spread of (a) = {(max(times[list(runs)[0]]) - min(times[list(runs)[0]])) / a * 100:.1f} % of its median', flush=True)
    ex.close()
