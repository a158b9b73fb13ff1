"""Public CMVM surface -- mirrors the reference's ``da4ml.cmvm`` (src/da4ml/cmvm/__init__.py:7-29)."""

from collections.abc import Callable
from typing import NamedTuple, TypedDict

import numpy as np

from .._binary import kernel_decompose, recode_code, slack_value, solve, solve_each, solve_many, tie_order_code
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


def solve_restarts(kernel, n_restarts: int, seed: int = 0, return_all: bool = False, order: str = 'random', recode: str = 'csd', slack: int = 0, **solve_options):
    """Best of ``n_restarts`` greedy searches of one matrix (addition to the reference API; ``solve_options`` as for ``solve``).

    Most greedy steps have several equally scored pairs, and the reference takes the last of them in its sorted table.
    Restart 0 does the same -- it IS ``solve(kernel, **solve_options)`` --, every other restart settles ties by a different strict
    total order (``restart_seeds``); scores are never touched.  All restarts go to the device in one call and run side by side;
    the stage-1 distances of the matrix are computed once.  The winner is the first strict minimum of the cost as the reference
    accumulates it (float32, op order: ``multi_gpu.pipeline_cost_f32``), so a tie returns restart 0 and the returned cost is
    never above ``solve``'s.  The same ``seed`` gives the same restarts on every run.

    ``order``: how a restart's seed orders tied pairs.  ``'random'`` (the default): which pair wins is random.  ``'newest'``: the pair
    with the newest row still wins, as in the reference -- that is what makes the reference's order a good one --, and the seed orders
    only what lies below (the older row of the pair, then shift and sign).  Restart 0 is ``solve`` itself under either; the seeds are the
    same.  At 64x64 and above no random restart beats ``solve`` while most newest-first restarts do (README).  Anything else is a
    ``ValueError``.

    ``recode``: the signed-digit form the restarts r >= 1 start from (``solve_recoded``).  ``'csd'`` (the default): the reference's digits,
    as every restart had them so far.  ``'compact'``: the compact digits.  ``'seeded'``: the restart's own seed also draws the coins of
    its digits.  Restart 0 stays ``solve``.  Anything else is a ``ValueError``.

    ``slack``: an int 0 .. 255 (anything else is a ``ValueError``); 0, the default: none.  The restarts r >= 1 discount the score of every
    pair by at most slack / 256 of it, a hash of (pair, key, the restart's seed): a pair whose score lies within that fraction of the best
    can win the step -- the restricted candidate list of a randomised greedy search, where the tie orders move equally scored pairs only.
    Restart 0 stays ``solve``, so the result is never dearer.  Small slacks (2 to 8) are the useful ones; 32 and more lose (README).

    ``return_all=True``: ``(best_index, [Pipeline, ...], [cost, ...])`` instead of the winning Pipeline."""
    from ..multi_gpu import pipeline_cost_f32

    tie_order_code(order)
    recode_code(recode)
    slack = slack_value(slack)
    seeds = restart_seeds(n_restarts, seed)
    if order != 'random':
        solve_options = {**solve_options, 'tie_order': order}
    if recode != 'csd':
        solve_options = {**solve_options, 'recode': recode}
    if slack:
        solve_options = {**solve_options, 'slack': slack}
    per_kernel = {k: [v] * len(seeds) for k, v in solve_options.items() if k in ('qintervals', 'latencies') and v is not None}
    opts = {k: v for k, v in solve_options.items() if k not in ('qintervals', 'latencies')}
    pipes = solve_many([kernel] * len(seeds), seeds=seeds, **opts, **per_kernel)
    costs = [pipeline_cost_f32(p) for p in pipes]
    best = first_strict_minimum(costs)
    return (best, pipes, costs) if return_all else pipes[best]


def solve_recoded(kernel, n: int = 8, seed: int = 0, return_all: bool = False, **solve_options):
    """Best of ``n`` greedy searches of one matrix that differ in the signed digits they start from (addition to the reference API;
    ``solve_options``: the keywords of ``solve`` and no others).

    Every chain of the reference starts from the CSD (non-adjacent) digits of the matrix.  That is one of several minimal signed-digit
    forms: 3 is ``4 - 1`` and also ``2 + 1``, with as many digits, and which form the search starts from changes which digit pairs
    repeat.  Point 0 is ``solve(kernel, **solve_options)`` itself; point 1 starts from the COMPACT digits (every ``s 0 -s`` of the CSD
    form, scanned from the top, becomes ``0 s s``); points 2 .. n-1 rewrite only the sites a coin picks, keyed by the coefficient's value
    and the seed ``restart_seeds(n, seed)[r]`` -- equal coefficients get equal digits wherever they stand.  All points keep the
    reference's tie order and run in one ``solve_each`` call; the stage-1 distances of the matrix are computed once.  The winner is the
    first strict minimum of the float32 cost (``multi_gpu.pipeline_cost_f32``), so the result is never dearer than ``solve``'s.

    At 3 to 5 bit weights the compact digits save 1 to 3 % of the adders; at 8 bits they lose (README): a restart dimension, not a
    default.  ``solve_restarts(..., recode=)`` combines a recoding with the tie-order restarts.

    ``return_all=True``: ``(best_index, [Pipeline, ...], [cost, ...])`` instead of the winning Pipeline."""
    from ..multi_gpu import pipeline_cost_f32

    for key in ('seed', 'tie_order', 'dc_weight', 'recode', 'recode_seed', 'slack'):  # (solve takes none of them: point 0 would no longer be solve(kernel, **solve_options))
        if key in solve_options:
            raise TypeError(f"solve_recoded() takes solve's keywords: {key!r} is not one of them")
    seeds = restart_seeds(n, seed)
    per_kernel = {k: [solve_options[k]] * len(seeds) for k in ('qintervals', 'latencies') if solve_options.get(k) is not None}
    base = {k: v for k, v in solve_options.items() if k not in ('qintervals', 'latencies')}
    options = [dict(base)]
    for r in range(1, len(seeds)):
        options.append({**base, 'recode': 'compact'} if r == 1 else {**base, 'recode': 'seeded', 'recode_seed': seeds[r]})
    pipes = solve_each([kernel] * len(seeds), options, **per_kernel)
    costs = [pipeline_cost_f32(p) for p in pipes]
    best = first_strict_minimum(costs)
    return (best, pipes, costs) if return_all else pipes[best]


class TradeoffPoint(NamedTuple):
    """One solve of ``solve_tradeoff``: ``method0`` / ``method1`` / ``dc_weight`` are ``None`` where the point left them to ``solve_options``
    (point 0) resp. to the method's own constant."""

    cost: float
    latency: float
    method0: str | None
    method1: str | None
    dc_weight: float | None
    pipeline: object


def pareto_front(points) -> list:
    """The points no other point beats in both cost and latency: ascending latency, strictly decreasing cost.  Of equal (cost, latency) the
    earliest point stays."""
    front = []
    for _, p in sorted(enumerate(points), key=lambda ip: (ip[1].latency, ip[1].cost, ip[0])):
        if not front or p.cost < front[-1].cost:
            front.append(p)
    return front


def solve_tradeoff(kernel, weights=(0.5, 1, 2, 4, 8, 16, 32, 64), methods=('wmc-pdc', 'wmc-dc'), return_all: bool = False, **solve_options):
    """The cost / latency trade-off of one matrix (addition to the reference API; ``solve_options``: the keywords of ``solve`` and no others --
    ``seed`` and ``dc_weight`` are a ``TypeError``).

    The ``*-dc`` / ``*-pdc`` selectors score a pair as its (weighted) count less ``w`` times the latency difference of its two rows; the
    reference fixes ``w`` (256 for ``wmc-*``, 1e9 for ``mc-*``), which leaves three points between cheap and shallow.  Smaller weights fill
    the gap, but not monotonically, so they are swept: point 0 is ``solve(kernel, **solve_options)`` itself, then for every method ``m`` of
    ``methods`` the solve with ``method0 = method1 = m`` at the method's own weight and at every weight of ``weights``.  All points go to
    the device in ONE call (``_binary.solve_each``) and run side by side; the stage-1 distances of the matrix are computed once.

    Cost is the float32 cost as the reference accumulates it (``multi_gpu.pipeline_cost_f32``), latency the largest output latency of the
    last stage.  Returns the Pareto front: a list of ``TradeoffPoint``, ascending latency, strictly decreasing cost; of equal (cost,
    latency) the earliest point stays, so point 0 is never displaced by an equal.  ``return_all=True``: ``(front, all points)``.
    ``cheapest_within(front, max_latency)`` picks from it."""
    from ..multi_gpu import pipeline_cost_f32

    for key in ('seed', 'dc_weight'):  # (solve takes neither: point 0 would no longer be solve(kernel, **solve_options))
        if key in solve_options:
            raise TypeError(f"solve_tradeoff() takes solve's keywords: {key!r} is not one of them")
    per_kernel = {k: solve_options[k] for k in ('qintervals', 'latencies') if solve_options.get(k) is not None}
    base = {k: v for k, v in solve_options.items() if k not in ('qintervals', 'latencies')}
    labels = [(None, None, None)]
    options = [dict(base)]
    for m in methods:
        for w in (None, *weights):
            labels.append((m, m, None if w is None else float(w)))
            options.append({**base, 'method0': m, 'method1': m, 'dc_weight': w})
    n = len(options)
    pipes = solve_each([kernel] * n, options, **{k: [v] * n for k, v in per_kernel.items()})
    points = [TradeoffPoint(pipeline_cost_f32(p), float(max(p.out_latencies, default=0.0)), *lab, p) for lab, p in zip(labels, pipes)]
    front = pareto_front(points)
    return (front, points) if return_all else front


def cheapest_within(front, max_latency: float):
    """The member of ``front`` (``solve_tradeoff``) of least cost whose latency is at most ``max_latency``; ``ValueError`` when there is none."""
    ok = [p for p in front if p.latency <= max_latency]
    if not ok:
        raise ValueError(f'no point with latency <= {max_latency}: the smallest latency available is {min(p.latency for p in front)}')
    return min(ok, key=lambda p: p.cost)


__all__ = ['solve', 'solve_many', 'solve_restarts', 'solve_recoded', 'solve_tradeoff', 'cheapest_within', 'TradeoffPoint', 'QInterval', 'Op', 'CombLogic', 'kernel_decompose', 'solver_options_t']
