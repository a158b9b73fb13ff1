"""Compiled DAIS executables (da4ml_amd._binary.dais_compile, C ABI da_dais_compile / da_dais_exec_run) in the two host modes: the
block executor stage by stage ('host') and the device kernel's per-value path over the compiled chain with its slots
('host-scalar').  The reference of a chain is the stage-by-stage `dais_interp_run`.  Host code: runs without a GPU."""

import gzip
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
from dais_cases import random_program
from dais_exec_cases import compose, faulting_stage, pipeline_programs, random_chain, samples_for, with_absent_output

ROOT = Path(__file__).resolve().parent.parent
HOST_MODES = ('host', 'host-scalar')


def test_one_program_reproduces_the_golden_vectors():
    from da4ml_amd._binary import dais_compile

    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'dais_golden.json.gz', 'rt'))
    assert len(gold['cases']) > 40
    for case in gold['cases']:
        prog = np.asarray(case['program'], dtype=np.int32)
        x = np.asarray([float.fromhex(v) for v in case['inputs']]).reshape(case['n_samples'], -1)
        want = np.asarray([float.fromhex(v) for v in case['outputs']]).reshape(case['n_samples'], -1)
        with dais_compile(prog) as ex:
            assert (ex.n_stages, ex.n_in, ex.n_out) == (1, x.shape[1], want.shape[1])
            for mode in HOST_MODES:
                assert np.array_equal(ex(x, executor=mode), want), (case['seed'], mode)


@pytest.mark.parametrize('n_stages', [2, 3])
def test_random_chains_equal_the_stage_by_stage_composition(n_stages):
    """samples inside and far outside the declared input formats; the chain's slot count lies between the largest per-stage count and
    their sum"""
    from da4ml_amd._binary import dais_compile

    for seed in range(40):
        progs, x = random_chain(seed, n_stages)
        want = compose(progs, x)
        with dais_compile(progs) as ex:
            assert ex.n_stages == n_stages and ex.info['n_ops'] == sum(int(p[4]) for p in progs)
            for mode in HOST_MODES:
                assert np.array_equal(ex(x, executor=mode, n_threads=1 + seed % 3), want), (seed, mode)
            per_stage = [dais_compile(p).info['n_slots'] for p in progs]
            assert max(per_stage) <= ex.info['n_slots'] <= sum(per_stage), (seed, per_stage, ex.info['n_slots'])
            assert ex.info['regfile_bytes_per_sample'] == 8 * ex.info['n_slots']


def test_an_absent_output_at_a_boundary_feeds_zero():
    from da4ml_amd._binary import dais_compile, dais_interp_run

    for seed in range(10):
        (p0, p1), x = random_chain(seed, 2)
        j = seed % int(p0[3])
        p0 = with_absent_output(p0, j)
        mid = dais_interp_run(p0, x)
        assert np.all(mid[:, j] == 0.0)
        want = dais_interp_run(p1, mid)
        with dais_compile([p0, p1]) as ex:
            for mode in HOST_MODES:
                assert np.array_equal(ex(x, executor=mode), want), (seed, mode)


def _split_pipelines(oracle):
    """register-stage splits (to_pipeline, no retiming) of CMVM graphs: the reference's own splits from the committed golden file, and
    splits of a solver result into 2 and 3 and more stages"""
    from cases import int_matrix

    from da4ml_amd.trace import to_pipeline
    from da4ml_amd.types import Pipeline

    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'pipeline_golden.json.gz', 'rt'))
    pipes = [Pipeline.deserialize(it['result']) for it in gold['split'] if isinstance(it['result'], list) and it['solve'].startswith('c1_16x16')]
    pipes = [p for p in pipes if len(p.solutions) in (2, 3)][:6]
    assert {len(p.solutions) for p in pipes} == {2, 3}
    comb = oracle.solve(int_matrix(5, 12, 10, -64, 64), adder_size=1, carry_size=-1).solutions[0]
    for cut in (2.0, 3.0):
        pipes.append(to_pipeline(comb, cut, retiming=False, verbose=False))
    return comb, pipes


def test_to_pipeline_splits_as_one_executable(oracle):
    """the stages of a to_pipeline split as one chain: equal to the composition for samples inside and outside the input intervals, and --
    inside them -- to the unsplit graph, since the inner boundaries of a split are exact"""
    comb, pipes = _split_pipelines(oracle)
    rng = np.random.default_rng(3)
    for pipe in pipes:
        progs = pipeline_programs(pipe)
        x = np.concatenate([samples_for(pipe.solutions[0], rng, 40), samples_for(pipe.solutions[0], rng, 40, spread=50)])
        want = compose(progs, x)
        with pipe.compile() as ex:
            assert ex.n_stages == len(progs)
            for mode in HOST_MODES:
                assert np.array_equal(ex(x, executor=mode), want), mode
        assert np.array_equal(pipe.predict(x), want)
        assert np.array_equal(pipe.predict(x, executor='host-scalar'), want)
    for pipe in pipes[-2:]:
        assert len(pipe.solutions) >= 2
        x = samples_for(comb, rng, 64)
        assert np.array_equal(pipe.predict(x), comb.predict(x))
        assert np.array_equal(pipe.predict(x), x @ comb.kernel.astype(np.float64))


def test_comblogic_compile_equals_predict(oracle):
    from cases import int_matrix

    sol = oracle.solve(int_matrix(3, 12, 9, -64, 64), adder_size=1, carry_size=-1)
    rng = np.random.default_rng(0)
    for stage in sol.solutions:
        x = samples_for(stage, rng, 50, spread=3)
        with stage.compile() as ex:
            assert np.array_equal(ex(x, executor='host'), stage.predict(x))
    x = samples_for(sol.solutions[0], rng, 50)
    assert np.array_equal(sol.predict(x), sol.solutions[1].predict(sol.solutions[0].predict(x)))


def test_a_table_fault_in_the_second_stage_raises_the_reference_message():
    from da4ml_amd._binary import dais_compile

    p0, x = random_program(11, n_in=3, n_ops=40, n_out=2)
    with dais_compile([p0, faulting_stage(2)]) as ex:
        assert ex.info['has_tables']
        for mode in HOST_MODES:
            with pytest.raises(RuntimeError, match=r'Logic lookup index out of bounds: index=\d+, table_size=4'):
                ex(x, executor=mode)


def test_compile_errors():
    from da4ml_amd._binary import dais_compile

    p0, _ = random_program(1, n_in=3, n_ops=30, n_out=4)
    p1, _ = random_program(2, n_in=5, n_ops=30, n_out=2)
    with pytest.raises(RuntimeError, match='stage 0 has 4 outputs, stage 1 expects 5 inputs'):
        dais_compile([p0, p1])
    with pytest.raises(RuntimeError, match='size mismatch'):
        dais_compile([p0[:-1]])
    with pytest.raises(RuntimeError, match='size mismatch'):
        dais_compile([p0, p1[:-3]])
    bad = p0.copy()
    bad[0] = 2
    with pytest.raises(RuntimeError, match='DAIS version mismatch'):
        dais_compile(bad)
    with pytest.raises(RuntimeError):
        dais_compile([])


def test_strides_element_types_and_tiny_batches():
    from da4ml_amd._binary import dais_compile

    progs, x = random_chain(7, 2, n_samples=40)
    n_in, n_out = x.shape[1], int(progs[-1][3])
    want = compose(progs, x)
    with dais_compile(progs) as ex:
        for mode in HOST_MODES:
            # input rows inside a wider array; outputs into a slice of a wider array, the rest of which stays as it was
            wide = np.full((40, n_in + 3), np.nan)
            wide[:, 1 : 1 + n_in] = x
            out = np.full((40, n_out + 5), -7.0)
            got = ex(wide[:, 1 : 1 + n_in], out=out[:, 2 : 2 + n_out], executor=mode)
            assert np.array_equal(got, want) and np.shares_memory(got, out)
            assert np.all(out[:, :2] == -7.0) and np.all(out[:, 2 + n_out :] == -7.0)
            # float32 in: widened exactly; float32 out: the exact double rounded once
            x32 = x.astype(np.float32)
            want32 = compose(progs, x32.astype(np.float64))
            assert np.array_equal(ex(x32, executor=mode), want32)
            got32 = ex(x32, out_dtype=np.float32, executor=mode)
            assert got32.dtype == np.float32 and np.array_equal(got32, want32.astype(np.float32))
            # other layouts and types are converted; 0 and 1 samples
            assert np.array_equal(ex(np.asfortranarray(x), executor=mode), want)
            assert np.array_equal(ex(x[:1], executor=mode), want[:1])
            assert ex(x[:0], executor=mode).shape == (0, n_out)
            ints = np.round(x).astype(np.int64)
            assert np.array_equal(ex(ints, executor=mode), compose(progs, ints.astype(np.float64)))
        with pytest.raises(ValueError):
            ex(x[:, :-1], executor='host')
        with pytest.raises(ValueError):
            ex(x, out=np.zeros((40, n_out + 1)), executor='host')
        with pytest.raises(ValueError):
            ex(x, executor='tpu')
    with pytest.raises(RuntimeError, match='closed'):
        ex(x, executor='host')


def test_device_modes_need_a_gpu():
    from da4ml_amd import _binary as hip

    if hip.device_count() > 0:
        pytest.skip('a GPU is present')
    progs, x = random_chain(0, 2)
    with hip.dais_compile(progs) as ex:  # compiles without a device
        with pytest.raises(RuntimeError, match='no HIP device'):
            ex(x, executor='device')


def test_columnar_program_words_equal_to_binary():
    """solver results keep their statements as the C ABI's arrays (a lazy OpList): program_words() builds the program from the columns and
    must give the words of to_binary(), which builds an Op per statement"""
    from da4ml_amd._marshal import stage_from_arrays
    from da4ml_amd.types import CombLogic, Pipeline

    gold = json.load(gzip.open(ROOT / 'tests' / 'golden' / 'pipeline_golden.json.gz', 'rt'))
    seen = 0
    for it in gold['split'][::9]:
        if not isinstance(it['result'], list) or it['solve'].startswith('handmade'):
            continue
        for comb in Pipeline.deserialize(it['result']).solutions:
            if not all(op.opcode in (-1, 0, 1, 5) for op in comb.ops):
                continue
            ci = np.array([[op.id0, op.id1, op.opcode, op.data] for op in comb.ops], np.int64).reshape(-1, 4)
            ff = np.array([[*op.qint, op.latency, op.cost] for op in comb.ops], np.float32).reshape(-1, 5)
            lazy = stage_from_arrays(*comb.shape, comb.inp_shifts, comb.out_idxs, comb.out_shifts, comb.out_negs, ci, ff, comb.carry_size, comb.adder_size)
            assert lazy.ops._lazy()
            words = lazy.program_words()
            assert lazy.ops._lazy(), 'program_words built the Op objects'
            assert words.dtype == np.int32 and np.array_equal(words, lazy.to_binary())
            assert np.array_equal(words, CombLogic(*lazy[:5], list(lazy.ops), *lazy[6:]).program_words())
            seen += len(comb.ops)
    assert seen > 2000
    # intervals that are not on a power-of-two grid, wide immediates and negative data words: still the words of to_binary()
    ci = np.array([[0, -1, -1, 0], [1, -1, -1, 0], [0, 1, 0, -3], [0, 1, 1, 2], [-1, -1, 5, -(1 << 40) - 5]], np.int64)
    ff = np.array([[-8, 7.5, 0.5, 0, 0], [0, 0, 1, 0, 0], [-9, 7.5, 0.0625, 1, 2], [-40, 37.5, 0.5, 1, 2], [-3, -3, 0.75, 0, 0]], np.float32)
    lazy = stage_from_arrays(2, 2, [0, 1], [2, 3], [0, -1], [0, 1], ci, ff, -1, -1)
    assert np.array_equal(lazy.program_words(), lazy.to_binary())


def test_importing_the_package_leaves_torch_out():
    code = 'import sys; import da4ml_amd, da4ml_amd._binary, da4ml_amd.types; assert "torch" not in sys.modules; print("ok")'
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:]
