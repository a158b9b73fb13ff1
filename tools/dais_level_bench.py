"""Time per call of the compiled DAIS executables by execution mode and batch size:  python tools/dais_level_bench.py [repeats] [n ...]

For stage 0 of the seed-0 n x n int8 `wmc` single-chain solve (n = 64 and 256 by default), on torch tensors that live on the device
(DA_DAIS_DEVICE_RESIDENT, synchronised for the timing), at 1, 16, 256, 4 096, 65 536 and 10^6 rows:
  (sample)        mode='sample': k_dais_exec, one thread per sample, the statements in program order;
  (level-lds)     mode='level':  k_dais_exec_level with the value file in LDS -- where it fits; otherwise the column is the next one again;
  (level-global)  mode='level' under DA4ML_DAIS_LEVEL_LDS=0: the value file in global memory.
The protocol of tools/dais_exec_bench.py: two warm-up rounds, then `repeats` (7) rounds that run the modes one after the other, so that
drift hits all alike; printed: median [min, max] of ms per call and median samples/s.  Below 10^6 rows a timing is a burst of 10 calls
between two synchronisations, divided by 10: a single call of a few microseconds would time the clock.  AUTO may run `level` only where its median lies
below the MINIMUM of `sample` on both programs.  The first round's results are checked against the matrix product."""
import os
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

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
sizes = [int(v) for v in sys.argv[2:]] or [64, 256]
COUNTS = (1, 16, 256, 4096, 65536, 10**6)
MODES = (('sample', 'sample', None), ('level-lds', 'level', None), ('level-global', 'level', '0'))


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        y = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls, y


for n in sizes:
    stage = solve(int_matrix(0, n, n, -128, 128), method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False).solutions[0]
    x = np.random.default_rng(0).integers(-128, 128, (max(COUNTS), n)).astype(np.float64)
    kernel = stage.kernel.astype(np.float64)
    xd = torch.from_numpy(x).cuda()
    ex = stage.compile()
    out_d = torch.empty((max(COUNTS), stage.shape[1]), dtype=torch.float64, device='cuda')
    info = ex.info
    print(f'{n}x{n} stage 0: {info["n_ops"]} statements; program order {info["n_slots"]} slots; level order {info["n_levels"]} levels, widest '
          f'{info["level_width"]}, {info["level_slots"]} slots = {8 * info["level_slots"]} B of value file per sample; {repeats} rounds', flush=True)
    for rows in COUNTS:
        times, ran = {name: [] for name, _, _ in MODES}, {}
        for r in range(2 + repeats):
            for name, mode, lds in MODES:
                if lds is None:
                    os.environ.pop('DA4ML_DAIS_LEVEL_LDS', None)
                else:
                    os.environ['DA4ML_DAIS_LEVEL_LDS'] = lds
                dt, y = timed(lambda: ex(xd[:rows], out=out_d[:rows], mode=mode), 10 if rows < 10**6 else 1)
                if r == 0:
                    assert np.array_equal(y.cpu().numpy(), x[:rows] @ kernel), (name, rows)
                    ran[name] = f'{ex.info["last_run"]}, S={ex.info["level_S"]}' if mode == 'level' else ex.info['last_run']
                if r >= 2:
                    times[name].append(dt)
        os.environ.pop('DA4ML_DAIS_LEVEL_LDS', None)
        print(f'  n = {rows}', flush=True)
        floor = min(times['sample'])
        for name, _, _ in MODES:
            ts = times[name]
            med = statistics.median(ts)
            verdict = '' if name == 'sample' else '   below the minimum of sample' if med < floor else '   NOT below the minimum of sample'
            print(f'    ({name:12s}): {med * 1e3:10.3f} ms  [{min(ts) * 1e3:.3f}, {max(ts) * 1e3:.3f}]  {rows / med:.3e} samples/s  ran {ran[name]}{verdict}', flush=True)
    ex.close()
