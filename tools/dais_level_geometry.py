"""Block size and tile of k_dais_exec_level (mode='level' of the compiled DAIS executables):  python tools/dais_level_geometry.py

For stage 0 of the seed-0 64x64 and 256x256 `wmc` single-chain solves on device tensors, at 1, 256, 4 096, 65 536 and 10^6 rows: median ms
per call over 5 interleaved rounds after 2 warm-ups (bursts of 10 calls below 10^6 rows) of the library's geometry (blocks of 1 024 lanes, the
tile S it chooses), of blocks of 512 and 256 lanes (DA4ML_DAIS_LEVEL_TPB), and of twice and half its tile (DA4ML_DAIS_LEVEL_S; a tile the
value file does not allow falls back to the one that fits, as the printed S tells).  The choice of block and tile rests on this table
(profiles/dais_level_geometry.txt)."""
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

VARIANTS = [('tpb1024', {}), ('tpb512', {'DA4ML_DAIS_LEVEL_TPB': '512'}), ('tpb256', {'DA4ML_DAIS_LEVEL_TPB': '256'}),
            ('S2x', None), ('S/2', None)]
KN = ('DA4ML_DAIS_LEVEL_TPB', 'DA4ML_DAIS_LEVEL_S')

for n in (64, 256):
    stage = solve(int_matrix(0, n, n, -128, 128), method0='wmc', method1='wmc', decompose_dc=-1, search_all_decompose_dc=False).solutions[0]
    x = np.random.default_rng(0).integers(-128, 128, (10**6, n)).astype(np.float64)
    xd = torch.from_numpy(x).cuda()
    ex = stage.compile()
    out_d = torch.empty((10**6, stage.shape[1]), dtype=torch.float64, device='cuda')
    for rows in (1, 256, 4096, 65536, 10**6):
        ex(xd[:rows], out=out_d[:rows], mode='level')
        s0 = ex.info['level_S']
        times, ran = {}, {}
        for r in range(2 + 5):
            for name, env in VARIANTS:
                if env is None:
                    s = s0 * 2 if name == 'S2x' else max(1, s0 // 2)
                    env = {'DA4ML_DAIS_LEVEL_S': str(s)}
                for k in KN:
                    os.environ.pop(k, None)
                os.environ.update(env)
                calls = 10 if rows < 10**6 else 1
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    ex(xd[:rows], out=out_d[:rows], mode='level')
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / calls
                ran[name] = f'{ex.info["last_run"]} S={ex.info["level_S"]}'
                if r >= 2:
                    times.setdefault(name, []).append(dt)
        for k in KN:
            os.environ.pop(k, None)
        print(f'{n}x{n} n={rows}: ' + '  '.join(f'{k} {statistics.median(v) * 1e3:.3f} ({ran[k]})' for k, v in times.items()), flush=True)
    ex.close()
