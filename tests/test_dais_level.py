"""The level schedule of compiled DAIS executables (csrc/dais_exec.h: LevelSchedule; C ABI da_dais_exec_run_mode, da_dais_exec_info2,
da_dais_exec_level_schedule) on the host: the schedule's invariants against a longest-path computation made here from the program
words, and mode='level' of the host-scalar executor -- the level schedule over its own slots, every level back to front -- against the
host block executor.  Host code: runs without a GPU."""

import gzip
import json
from pathlib import Path

import numpy as np
import pytest
from dais_cases import random_program
from dais_exec_cases import compose, faulting_stage, random_chain, with_absent_output

ROOT = Path(__file__).resolve().parent.parent


def golden_cases():
    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'dais_golden.json.gz', 'rt'))
    for case in gold['cases']:
        prog = np.asarray(case['program'], dtype=np.int32)
        x = np.asarray([float.fromhex(v) for v in case['inputs']]).reshape(case['n_samples'], -1)
        want = np.asarray([float.fromhex(v) for v in case['outputs']]).reshape(case['n_samples'], -1)
        yield case['seed'], prog, x, want


def program(n_in, ops, out_idx, out_shift=None, out_neg=None, tables=()):
    """program words from statements [opcode, id0, id1, lo, hi, signed, integer bits, fractional bits] (docs of the format: dais_cases.py)"""
    n_out = len(out_idx)
    head = [1, 0, n_in, n_out, len(ops), len(tables)] + [0] * n_in + list(out_idx) + list(out_shift or [0] * n_out) + list(out_neg or [0] * n_out)
    return np.asarray(head + [w for op in ops for w in op] + [len(t) for t in tables] + [w for t in tables for w in t], dtype=np.int32)


def operands(op):
    """the statements a statement of the program words reads"""
    code, id0, id1, lo = int(op[0]), int(op[1]), int(op[2]), int(op[3])
    if code in (-1, 5):
        return []
    if code in (0, 1, 7, 10):
        return [id0, id1]
    if code in (6, -6):
        return [id0, id1, lo]
    assert code in (2, -2, 3, -3, 4, 8, 9, -9), code
    return [id0]


def longest_paths(progs):
    """(reads, level) of every statement of the chain, numbered through the stages in program order -- from the words alone: level 0 for a
    statement that reads nothing, else 1 + the largest level it reads; an input statement of a later stage reads the statement behind
    the output of the stage before it, or nothing when that output is absent"""
    reads, level, base, prev_out = [], [], 0, None
    for p in progs:
        n_in, n_out, n_ops = int(p[2]), int(p[3]), int(p[4])
        code0 = 6 + n_in + 3 * n_out
        for i in range(n_ops):
            op = p[code0 + 8 * i : code0 + 8 * i + 8]
            if int(op[0]) == -1 and prev_out is not None:
                r = [prev_out[int(op[1])]] if prev_out[int(op[1])] >= 0 else []
            else:
                r = [base + v for v in operands(op)]
            reads.append(r)
            level.append(1 + max(level[v] for v in r) if r else 0)
        prev_out = [base + int(o) if o >= 0 else -1 for o in p[6 + n_in : 6 + n_in + n_out]]
        base += n_ops
    return reads, level, prev_out


def check_schedule(progs):
    from da4ml_amd._binary import dais_compile

    reads, level, outs = longest_paths(progs)
    total = len(level)
    with dais_compile(progs) as ex:
        info = ex.info
        rows, out_slots = ex.level_schedule()
    assert rows.shape == (total, 6) and sorted(rows[:, 0].tolist()) == list(range(total)), 'every statement once'
    assert np.all(np.diff(rows[:, 1]) >= 0), 'the schedule is ordered by level'
    got_level, slot = np.zeros(total, np.int64), np.zeros(total, np.int64)
    got_level[rows[:, 0]], slot[rows[:, 0]] = rows[:, 1], rows[:, 2]
    assert got_level.tolist() == level, 'levels are the longest paths'
    assert info['n_levels'] == (max(level) + 1 if total else 0)
    assert info['level_width'] == (np.bincount(got_level).max() if total else 0)
    last = list(level)  # the level of a value's last reader; its own when nothing reads it
    for row in rows:
        v = int(row[0])
        assert all(level[r] < level[v] for r in reads[v]), 'an operand lies in a lower level than its reader'
        assert [int(s) for s in row[3:] if s >= 0] == [int(slot[r]) for r in reads[v]], 'operand fields hold the slots of the values read'
        for r in reads[v]:
            last[r] = max(last[r], level[v])
    for j, o in enumerate(outs):
        assert out_slots[j] == (slot[o] if o >= 0 else -1)
        if o >= 0:
            last[o] = info['n_levels']  # read after the last level
    assert 0 <= slot.min() and slot.max() < info['level_slots']
    # values that share a slot have disjoint closed intervals [level written, level last read]; the widest overlap needs that many slots
    by_slot = {}
    for v in range(total):
        by_slot.setdefault(int(slot[v]), []).append((level[v], last[v]))
    for s, spans in by_slot.items():
        spans.sort()
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), (s, spans)
    alive = np.zeros(info['n_levels'] + 2, np.int64)
    for v in range(total):
        alive[level[v] : last[v] + 1] += 1
    assert info['level_slots'] >= alive.max()
    return info


def chain_cases():
    for seed in range(12):
        yield random_chain(seed, 1 + seed % 3)[0]


def test_schedule_invariants_on_the_chains():
    deepest = 0
    for progs in chain_cases():
        info = check_schedule(progs)
        deepest = max(deepest, info['n_levels'])
        assert info['n_levels'] <= info['n_ops'] and info['level_width'] >= 1
    assert deepest > 3


def test_schedule_invariants_on_the_golden_programs():
    n = 0
    for _, prog, _, _ in golden_cases():
        check_schedule([prog])
        n += 1
    assert n > 40


def level_equals_host(progs, x):
    """host-scalar LEVEL (levels back to front, the schedule's own slots) == host-scalar program order == the host block executor"""
    from da4ml_amd._binary import dais_compile

    want = compose(progs, x)
    with dais_compile(progs) as ex:
        assert np.array_equal(ex(x, executor='host', mode='level'), want)
        assert np.array_equal(ex(x, executor='host-scalar', mode='sample'), want)
        got = ex(x, executor='host-scalar', mode='level', n_threads=2)
        assert np.array_equal(got, want)
        return ex.info


@pytest.mark.parametrize('n_stages', [1, 2, 3])
def test_host_scalar_level_on_random_chains(n_stages):
    for seed in range(25):
        progs, x = random_chain(seed, n_stages)
        level_equals_host(progs, x)


def test_host_scalar_level_on_the_golden_vectors():
    from da4ml_amd._binary import dais_compile

    for seed, prog, x, want in golden_cases():
        with dais_compile(prog) as ex:
            assert np.array_equal(ex(x, executor='host-scalar', mode='level'), want), seed


def test_a_dependent_chain_of_300_statements_is_300_levels():
    ops = [[-1, 0, -1, 0, 0, 1, 6, 2]] + [[4, i, -1, i + 1, 0, 1, 30, 2] for i in range(299)]
    prog = program(1, ops, [299, 150, 0])
    x = np.linspace(-20, 20, 33).reshape(-1, 1)
    info = level_equals_host([prog], x)
    assert (info['n_levels'], info['level_width']) == (300, 1)
    check_schedule([prog])


def test_2500_statements_in_one_level():
    rng = np.random.default_rng(5)
    n_in, n = 4, 2500
    ops = [[-1, j, -1, 0, 0, 1, 6, 3] for j in range(n_in)]
    for _ in range(n):
        a, b = (int(v) for v in rng.integers(0, n_in, 2))
        ops.append([int(rng.integers(0, 2)), a, b, int(rng.integers(-2, 3)), 0, 1, 12, 5])
    prog = program(n_in, ops, [n_in + int(v) for v in rng.choice(n, 40, replace=False)])
    x = rng.integers(-200, 200, (20, n_in)) / 8.0
    info = level_equals_host([prog], x)
    assert (info['n_levels'], info['level_width']) == (2, n)
    check_schedule([prog])


def test_a_last_reader_and_a_new_value_in_one_level_do_not_share_a_slot():
    """a and b are last read in level 2, where e and f are new: in program order e may take the slot of a once d has read it, and does; by
    level -- d, e and f run in no particular order -- it must not"""
    from da4ml_amd._binary import dais_compile

    fmt = [1, 12, 0]
    ops = [[-1, 0, -1, 0, 0, 1, 6, 0], [-1, 1, -1, 0, 0, 1, 6, 0],  # a, b            level 0
           [0, 0, 1, 0, 0, *fmt],                                   # c = a + b       level 1
           [0, 2, 0, 1, 0, *fmt],                                   # d = c + 2 a     level 2: last reader of a
           [1, 2, 2, 2, 0, *fmt],                                   # e = c - 4 c     level 2
           [0, 2, 1, 0, 0, *fmt],                                   # f = c + b       level 2: last reader of b
           [0, 3, 4, 0, 0, *fmt], [0, 6, 5, 0, 0, *fmt]]            # d + e, (d + e) + f
    prog = program(2, ops, [7, 3])
    x = np.array([[3.0, 5.0], [-7.0, 2.0], [31.0, -32.0]])
    level_equals_host([prog], x)
    check_schedule([prog])
    with dais_compile(prog) as ex:
        rows, _ = ex.level_schedule()
        slot = dict(zip(rows[:, 0].tolist(), rows[:, 2].tolist()))
        assert len({slot[v] for v in (0, 1, 2, 3, 4, 5)}) == 6
        assert ex.info['n_slots'] < ex.info['level_slots'], 'the program order re-uses a slot inside what is one level here'


def test_absent_negated_and_shifted_boundary_outputs():
    for seed in range(10):
        (p0, p1), x = random_chain(seed, 2)
        n_in, n_out = int(p0[2]), int(p0[3])
        p0 = with_absent_output(p0, seed % n_out)
        level_equals_host([p0, p1], x)
        (p0, p1), x = random_chain(seed, 2)
        j = (seed + 1) % n_out
        p0 = p0.copy()
        p0[6 + n_in + n_out + j] += 3 - seed % 5  # out_shift
        p0[6 + n_in + 2 * n_out + j] ^= 1  # out_neg
        level_equals_host([p0, p1], x)
        check_schedule([p0, p1])


def test_a_table_fault_in_level_order_raises_the_reference_message():
    from da4ml_amd._binary import dais_compile

    p0, x = random_program(11, n_in=3, n_ops=40, n_out=2)
    with dais_compile([p0, faulting_stage(2)]) as ex:
        with pytest.raises(RuntimeError, match=r'Logic lookup index out of bounds: index=\d+, table_size=4'):
            ex(x, executor='host-scalar', mode='level')


def test_an_unknown_mode_is_an_error():
    from da4ml_amd import _binary as hip

    progs, x = random_chain(0, 2)
    with hip.dais_compile(progs) as ex:
        for mode in ('levels', '', None, 2):
            with pytest.raises(ValueError, match='mode'):
                ex(x, executor='host', mode=mode)
        info = ex.info
        assert info['last_run'] == 'none' and info['level_S'] == 0 and info['level_slots'] >= 1
        out = np.zeros((len(x), ex.n_out))
        L = hip.lib()
        for mode, want in ((0, 0), (1, 0), (2, 0), (3, -1), (-1, -1)):  # DA_ERR_RUNTIME == -1
            rc = L.da_dais_exec_run_mode(ex._handle(), x.ctypes.data, 0, ex.n_in, len(x), out.ctypes.data, 0, ex.n_out, 1, 0, None, mode)
            assert rc == want, (mode, rc)
            if want:
                assert 'unknown mode' in L.da_dais_last_error().decode()
        v = np.full(8, -9, np.int64)
        assert L.da_dais_exec_info2(ex._handle(), v, 3) == 0 and v[3] == -9 and v[2] == info['level_slots']
        assert L.da_dais_exec_info2(ex._handle(), v, 8) == 0 and v[4] == 0 and v[5] == -9
