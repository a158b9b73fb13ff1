"""Public CMVM surface -- mirrors the reference's ``da4ml.cmvm`` (src/da4ml/cmvm/__init__.py:7-29)."""

from collections.abc import Callable
from typing import TypedDict

import numpy as np

from .._binary import kernel_decompose, solve, solve_many
from ..types import CombLogic, Op, QInterval


class solver_options_t(TypedDict, total=False):
    method0: str
    method1: str
    hard_dc: int
    decompose_dc: int
    adder_size: int
    carry_size: int
    search_all_decompose_dc: bool
    offload_fn: None | Callable[[np.ndarray, object], np.ndarray]


_M64 = 0xFFFFFFFFFFFFFFFF


def splitmix64(x: int) -> int:
    """One output of the SplitMix64 generator for the state ``x`` (public-domain constants of Steele, Lea & Flood)."""
    z = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def restart_seeds(n_restarts: int, seed: int = 0) -> list[int]:
    """The tie seeds of ``solve_restarts``: restart 0 runs with 0 (the reference's order), restart r >= 1 with
    ``splitmix64(seed + r)``, 1 in place of a zero output."""
    if n_restarts < 1:
        raise ValueError('n_restarts must be at least 1')
    return [0] + [splitmix64((int(seed) + r) & _M64) or 1 for r in range(1, int(n_restarts))]


def first_strict_minimum(costs) -> int:
    """Index of the first strict minimum: the reference's rule for its ``decompose_dc`` candidates (api.cc:243-247)."""
    best = 0
    for i in range(1, len(costs)):
        if costs[i] < costs[best]:
            best = i
    return best


def solve_restarts(kernel, n_restarts: int, seed: int = 0, return_all: bool = False, **solve_options):
    """Best of ``n_restarts`` greedy searches of one matrix (addition to the reference API; ``solve_options`` as for ``solve``).

    Most greedy steps have several equally scored pairs, and the reference takes the last of them in its sorted table.
    Restart 0 does the same -- it IS ``solve(kernel, **solve_options)`` --, every other restart settles ties by a different strict
    total order (``restart_seeds``); scores are never touched.  All restarts go to the device in one call and run side by side;
    the stage-1 distances of the matrix are computed once.  The winner is the first strict minimum of the cost as the reference
    accumulates it (float32, op order: ``multi_gpu.pipeline_cost_f32``), so a tie returns restart 0 and the returned cost is
    never above ``solve``'s.  The same ``seed`` gives the same restarts on every run.

    ``return_all=True``: ``(best_index, [Pipeline, ...], [cost, ...])`` instead of the winning Pipeline."""
    from ..multi_gpu import pipeline_cost_f32

    seeds = restart_seeds(n_restarts, seed)
    per_kernel = {k: [v] * len(seeds) for k, v in solve_options.items() if k in ('qintervals', 'latencies') and v is not None}
    opts = {k: v for k, v in solve_options.items() if k not in ('qintervals', 'latencies')}
    pipes = solve_many([kernel] * len(seeds), seeds=seeds, **opts, **per_kernel)
    costs = [pipeline_cost_f32(p) for p in pipes]
    best = first_strict_minimum(costs)
    return (best, pipes, costs) if return_all else pipes[best]


__all__ = ['solve', 'solve_many', 'solve_restarts', 'QInterval', 'Op', 'CombLogic', 'kernel_decompose', 'solver_options_t']
