/* da4ml_hip.h -- C ABI of libda4ml_hip.so, the MI355X-native drop-in for da4ml's native CMVM module.
 *
 * Every entry point replaces one binding of the reference's nanobind module `cmvm_bin`
 * (reference src/da4ml/_binary/cmvm/bindings.cc:227-264, re-exported by src/da4ml/_binary/__init__.py:4 and
 * src/da4ml/cmvm/__init__.py:7).  Plain pointers and sizes only; no Python, torch or HIP types cross this
 * boundary.  All matrices are dense row-major; `kernel` is float32 [n_in, n_out] holding dyadic rationals
 * exactly (the reference's own contract, trace/fixed_variable_array.py:76).
 *
 * Error handling: functions returning int give 0 on success and a negative DA_ERR_* otherwise; functions returning
 * a handle give NULL on error.  da_last_error() returns the message of the calling thread's last failure
 * (the reference raises C++ exceptions that nanobind maps to Python exceptions, bindings.cc / api.cc:207-240).
 * The library never keeps pointers to caller memory after a call returns.
 *
 * Threading: calls are serialised per device by an internal mutex; solves of a batch run concurrently on the GPU.
 *
 * Size limits of a solve (DA_ERR_RUNTIME with a message beyond them): up to 2048 input rows are supported (pair tables of up to
 * 2^30 slots; a chain whose arena does not fit into the free device memory is refused with the MiB it needs and the MiB that are
 * free); up to 4095 output columns are supported, the limit of the row-reference format (from about 3300 columns on a chain runs the
 * many-column form of the selection kernel, which works on one of the two row lists in memory instead of LDS; DA4ML_HIP_MANYCOL_FROM=<n_out>
 * forces that form from a width on); a column-sharded chain (da_solve_sharded) keeps the regular form and so about 3300 columns per rank; a
 * chain holds fewer than 2^24 rows and 2^28 row-list entries; at most 30 CSD digits per entry.
 */
#ifndef DA4ML_HIP_H
#define DA4ML_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DA_OK 0
#define DA_ERR_RUNTIME (-1)  /* maps to Python RuntimeError (std::runtime_error in the reference) */
#define DA_ERR_VALUE (-2)    /* maps to Python ValueError   (std::invalid_argument in the reference) */
#define DA_ERR_NO_DEVICE (-3)

typedef struct da_result da_result; /* one solved Pipeline (two CombLogic stages) */

/* ---- library / device ------------------------------------------------------------------------------------ */
const char *da_last_error(void);
/* DA_ERR_* class of the calling thread's last failure -- which Python exception the reference would have raised
 * (std::invalid_argument -> ValueError, std::runtime_error -> RuntimeError; bindings.cc / state_opr.cc:70-72).  Needed
 * by the handle-returning entry points (da_solve returns NULL without a code). */
int da_last_error_code(void);
const char *da_version(void);
int da_device_count(void);     /* number of visible HIP devices (0 if none) */
int da_set_device(int device); /* device used by subsequent calls of this process (default 0) */

/* ---- scalar helpers -------------------------------------------------------------------------------------- */
/* cmvm_bin.get_lsb_loc (bindings.cc:229 -> bit_decompose.cc:10-20) */
int da_get_lsb_loc(float x);
/* cmvm_bin.iceil_log2 (bindings.cc:230 -> indexers.hh:12-18) */
int da_iceil_log2(float x);
/* cmvm_bin.cost_add (bindings.cc:25-41,249-263 -> state_opr.cc:31-67); q0,q1 = {min,max,step}; out2 = {latency,cost} */
int da_cost_add(const float *q0, const float *q1, int64_t shift, int sub, int adder_size, int carry_size, float *out2);

/* ---- decompositions (run on the GPU) --------------------------------------------------------------------- */
/* cmvm_bin.int_arr_to_csd (bindings.cc:43-61,228 -> bit_decompose.cc:22-42).  Returns the digit count N (>= 1) or a
 * negative error; `out` may be NULL to query N, otherwise int8 [n, N]. */
int da_int_arr_to_csd(const int32_t *x, int64_t n, int8_t *out);
/* cmvm_bin.csd_decompose (bindings.cc:63-103,231 -> bit_decompose.cc:45-62).  Returns N or a negative error; `csd`
 * (int8 [n_in, n_out, N]), `shift0` (int8 [n_in]), `shift1` (int8 [n_out]) may be NULL to query N. */
int da_csd_decompose(const float *kernel, int64_t n_in, int64_t n_out, int center, int8_t *csd, int8_t *shift0, int8_t *shift1);
/* cmvm_bin.kernel_decompose (bindings.cc:232-234 -> mat_decompose.cc:63-169): m0 float32 [n_in,n_out], m1 [n_out,n_out] */
int da_kernel_decompose(const float *kernel, int64_t n_in, int64_t n_out, int dc, float *m0, float *m1);

/* ---- solve ------------------------------------------------------------------------------------------------ */
/* cmvm_bin.solve (bindings.cc:184-225,235-248 -> api.cc:147-250).  `qintervals` is float32 [n_in,3] or NULL
 * (default (-128,127,1)), `latencies` float32 [n_in] or NULL (default 0).  Steps must be positive normal numbers (DA_ERR_VALUE
 * otherwise); they need not be powers of two (the latency model reads -log2f of any other step from a table the host builds with
 * its own libm, one row per distinct mantissa). */
da_result *da_solve(const float *kernel, int64_t n_in, int64_t n_out, const char *method0, const char *method1, int hard_dc,
                    int decompose_dc, const float *qintervals, const float *latencies, int adder_size, int carry_size,
                    int search_all_decompose_dc);

/* Batched form of da_solve (addition): `count` independent problems sharing the option
 * set are solved concurrently on the device.  kernels[i] is [n_in[i], n_out[i]]; qintervals / latencies may be NULL
 * or hold per-problem pointers (each possibly NULL).  results[i] receives a handle (to be freed with da_free).
 * Returns DA_OK, or an error in which case no handle is returned. */
int da_solve_batch(int count, const float *const *kernels, const int64_t *n_in, const int64_t *n_out, const char *method0,
                   const char *method1, int hard_dc, int decompose_dc, const float *const *qintervals,
                   const float *const *latencies, int adder_size, int carry_size, int search_all_decompose_dc,
                   da_result **results);

/* da_solve_batch with a tie seed per problem (addition, no reference counterpart): random restarts of the greedy search.  Most
 * greedy steps have several equally scored pairs; the reference takes the last of them in its sorted table.  A problem with
 * seeds[i] != 0 settles such ties by another strict total order, derived from the seed, in every greedy chain it runs (both stages,
 * every decompose_dc candidate and latency retry); scores are untouched, so the result is a greedy run of the same method.
 * Contract: seed 0 (or seeds == NULL) gives the reference's result, bit for bit -- da_solve_batch and da_solve are this call with
 * seeds == NULL; the same seed gives the same result on every run, in every batch composition and position; different seeds
 * are independent runs.  Running R seeds of one matrix in one call and keeping the cheapest result never does worse than the
 * reference when seed 0 is among them (da4ml_amd.cmvm.solve_restarts); the stage-1 distances of equal matrices are computed once
 * per call.  Column-sharded solves (da_solve_sharded) take no seed. */
int da_solve_batch_seeded(int count, const float *const *kernels, const int64_t *n_in, const int64_t *n_out, const char *method0,
                          const char *method1, int hard_dc, int decompose_dc, const float *const *qintervals,
                          const float *const *latencies, int adder_size, int carry_size, int search_all_decompose_dc,
                          const uint64_t *seeds /* [count], or NULL */, da_result **results);

/* da_solve_batch with the options of every problem in a struct of its own (addition, no reference counterpart): one call can mix methods,
 * latency budgets, tie seeds and penalty weights -- a sweep of the cost / latency trade-off of one matrix is one batch of chains.
 * dc_weight: the selectors mc-dc, mc-pdc, wmc-dc and wmc-pdc score a pair as float(count) - w |dlat| (mc-*) resp.
 * float(uint32 count * overlap) - w |dlat| (wmc-*), float32, the multiply and the subtract each rounded once; the reference's w is
 * 1e9 resp. 256.  A problem with dc_weight = w (finite, >= 0) uses w in every greedy chain whose resolved method is one of the four:
 * both stages, every decompose_dc candidate, every latency retry and the wmc-dc that hard_dc forces; mc, wmc and dummy ignore it.
 * Contract: DA_DC_WEIGHT_DEFAULT (or the constant of the method itself) gives the reference's result, bit for bit; any other negative
 * value, NaN or infinity gives DA_ERR_VALUE ("dc_weight must be a finite number >= 0"); the result of a problem depends on nothing but
 * its own matrix and options, whatever else the batch holds and wherever it stands in it.  da_solve_batch_seeded, da_solve_batch and
 * da_solve are this call with equal structs.  Small weights trade latency for adders between wmc and wmc-dc;
 * da4ml_amd.cmvm.solve_tradeoff sweeps them in one call and returns the Pareto front.  Column-sharded solves keep the constants.
 * tie_order (addition, no reference counterpart): which strict total order a problem with seed != 0 settles equal scores by.
 *   DA_TIE_RANDOM  the order of da_solve_batch_seeded: a keyed bijection of the whole row pair -- which pair wins a tie is random.
 *   DA_TIE_NEWEST  the reference lets the pair with the larger (id1, id0) win, i.e. the pair that re-uses the newest row; this order keeps
 *                  that -- the larger id1 still wins -- and orders the pairs of one id1, and the keys of one pair, by the seed.
 * Contract: with seed 0 the result is the reference's, bit for bit, whatever tie_order says; a (seed, tie_order) pair gives the same
 * result on every run, in every batch composition and position; any other tie_order gives DA_ERR_VALUE ("tie_order must be
 * DA_TIE_RANDOM or DA_TIE_NEWEST").  da_solve_batch_seeded stays the random order.  Column-sharded solves take neither.
 * struct_size must be sizeof(da_solve_opts), or DA_SOLVE_OPTS_SIZE_V1 -- the struct as it was before tie_order, its last field, was
 * added: tie_order is then not read and the problem runs DA_TIE_RANDOM.  Any other size gives DA_ERR_VALUE.  The structs of one call
 * lie struct_size bytes apart (an array of the caller's struct): all of one call have the same struct_size. */
#define DA_DC_WEIGHT_DEFAULT (-1.0f)
#define DA_TIE_RANDOM 0u
#define DA_TIE_NEWEST 1u
typedef struct da_solve_opts {
    uint32_t struct_size;
    const char *method0, *method1;
    int hard_dc, decompose_dc, adder_size, carry_size, search_all_decompose_dc;
    float dc_weight;
    uint64_t seed;
    uint32_t tie_order;
} da_solve_opts;
#define DA_SOLVE_OPTS_SIZE_V1 ((uint32_t)offsetof(da_solve_opts, tie_order))
int da_solve_batch_opts(int count, const float *const *kernels, const int64_t *n_in, const int64_t *n_out, const da_solve_opts *opts /* [count] */,
                        const float *const *qintervals, const float *const *latencies, da_result **results);

/* da_solve_batch_opts with a digit recoding per problem (addition, no reference counterpart).  Every greedy chain starts from the CSD
 * (non-adjacent form) digits of its matrix, as the reference does.  The NAF is one of several minimal signed-digit forms of a number
 * (3 = 4 - 1 = 2 + 1); which form the search starts from changes which digit pairs repeat, and with them the adder count.
 *   DA_RECODE_CSD      the NAF: the reference's digits.
 *   DA_RECODE_COMPACT  the NAF digits d scanned from (top position - 2) down to 0: a site d[p+2] = s != 0, d[p+1] = 0, d[p] = -s becomes
 *                      d[p+2] = 0, d[p+1] = s, d[p] = s (11 = 16 - 4 - 1 -> 8 + 4 - 1 -> 8 + 2 + 1).
 *   DA_RECODE_SEEDED   the same scan; a site is rewritten only when a coin keyed by (seed, |value|, p) says so.  Equal values get equal
 *                      digits wherever they stand, x and -x mirrored ones.
 * Every mode keeps the value, the digit count and the top position of every entry.  The mode goes into every chain of the problem: both
 * stages, every decompose_dc candidate, every latency retry, and the adder trees the minimal latency of hard_dc is measured on.
 * da_solve_opts cannot grow any further (its size is pinned), hence the second array.
 * Contract: recode == NULL, or mode DA_RECODE_CSD, is da_solve_batch_opts bit for bit; a mode other than the three, or a struct_size
 * other than sizeof(da_recode_opts), gives DA_ERR_VALUE; seed is read under DA_RECODE_SEEDED only; the result of a problem depends on
 * nothing but its own matrix and options, whatever else the batch holds and wherever it stands in it; the same inputs give the same
 * result on every run.  Compact digits save 1 to 3 % of the adders at 3 to 5 bit weights and lose at 8 bits: a restart dimension
 * (da4ml_amd.cmvm.solve_recoded), never a default.  Column-sharded chains start from the CSD digits only. */
#define DA_RECODE_CSD 0u
#define DA_RECODE_COMPACT 1u
#define DA_RECODE_SEEDED 2u
typedef struct {
    uint32_t struct_size;
    uint32_t mode;
    uint64_t seed;
} da_recode_opts;
int da_solve_batch_recode(int count, const float *const *kernels, const int64_t *n_in, const int64_t *n_out, const da_solve_opts *opts /* [count] */,
                          const da_recode_opts *recode /* [count] or NULL */, const float *const *qintervals, const float *const *latencies,
                          da_result **results);

/* da_solve_batch_recode with a score slack per problem (addition, no reference counterpart).  The greedy search takes the best-scored pair
 * at every step; a chain with a slack draws its pick from the pairs whose score lies within a small fraction of the best -- the restricted
 * candidate list of a randomised greedy search.  Every table entry gets a discount of at most slack / 256 of its score, a keyed hash of
 * (row pair, key, seed): with byte = slack_byte(id0, id1, key index, seed) in 0 .. 255 and base = count (mc family) or count * overlap (wmc
 * family), base becomes base - ((base * ((byte * slack) >> 8)) >> 8) when 0 < base < 2^24; the latency penalty, the cut of the -dc methods
 * and the tie order are what they were (entry_rank_slack, cmvm_core.h).  The slack goes into every greedy chain of the problem: both stages,
 * every decompose_dc candidate, every latency retry.  da_solve_opts and da_recode_opts cannot grow (their sizes are pinned), hence the third array.
 * Contract: search == NULL, or slack 0, is da_solve_batch_recode bit for bit; slack > 255, or a struct_size other than
 * sizeof(da_search_opts), gives DA_ERR_VALUE; slack != 0 with seed == 0 in the problem's da_solve_opts gives DA_ERR_VALUE (the seed keys the
 * discounts); the result of a problem depends on nothing but its own matrix and options, whatever else the batch holds and wherever it stands
 * in it; the same inputs give the same result on every run.  A restart dimension (da4ml_amd.cmvm.solve_restarts(..., slack=)), never a
 * default: a single slack chain is as often dearer than the reference's graph as cheaper.  Column-sharded chains take no slack. */
typedef struct {
    uint32_t struct_size;
    uint32_t slack; /* 0 .. 255; 0: none */
} da_search_opts;
int da_solve_batch_search(int count, const float *const *kernels, const int64_t *n_in, const int64_t *n_out, const da_solve_opts *opts /* [count] */,
                          const da_recode_opts *recode /* [count] or NULL */, const da_search_opts *search /* [count] or NULL */,
                          const float *const *qintervals, const float *const *latencies, da_result **results);

/* ---- column-sharded solve (BASELINE config C4; addition, no reference counterpart) ------------------------------------------
 * da_solve with every greedy chain sharded over the output COLUMNS of its matrix across `world` processes (one per GPU):
 * rank g holds the digits of columns [g n_out / world, (g+1) n_out / world), the pair-count table is replicated, and per
 * greedy step the ranks exchange two int32 slabs by all-reduce(sum) -- the loops it shards are column-outermost in the
 * reference (state_opr.cc:117,249,307; adder trees cmvm_core.cc:103).  Every rank calls this with identical arguments and
 * receives the identical, complete result (= da_solve's).  The library does not link a communication library: the host
 * process supplies the collective (RCCL through torch.distributed in da4ml_amd.multi_gpu.solve_column_sharded).
 * `allreduce(ctx, buf, count, on_device)`: in-place sum of `count` int32 at `buf` over all ranks; `buf` is device memory
 * of the current device when on_device != 0 (the producing kernels have completed), host memory otherwise; returns when
 * the result is in place.  stats3 (may be NULL) = {sharded chains, greedy steps, all-reduce calls}.  Latency-bound by
 * construction (two collectives per greedy step); the layout that scales is one matrix per rank (da_solve_batch). */
typedef void (*da_allreduce_i32)(void *ctx, void *buf, int64_t count, int on_device);
da_result *da_solve_sharded(const float *kernel, int64_t n_in, int64_t n_out, const char *method0, const char *method1, int hard_dc,
                            int decompose_dc, const float *qintervals, const float *latencies, int adder_size, int carry_size,
                            int search_all_decompose_dc, int rank, int world, da_allreduce_i32 allreduce, void *ctx, int64_t *stats3);
/* The same with the library's own RCCL transport (csrc/cmvm_rccl.*): `ncclAllReduce` in place on the library's HIP stream,
 * stream-ordered with the kernels that produce and consume the exchange buffers -- no callback, no host synchronisation per
 * exchange.  librccl.so is opened at run time (no link-time dependency).  Rank 0 obtains the 128-byte unique id
 * (da_rccl_unique_id = ncclGetUniqueId) and hands it to every rank by its own means (da4ml_amd.multi_gpu broadcasts it through
 * torch.distributed); every rank then calls da_solve_sharded_rccl with identical arguments.  The communicator of an id is kept
 * for further calls -- callers hand the SAME id to every solve of a process group (a fresh id per call would build, and keep, a
 * new communicator each time); da_rccl_shutdown destroys the kept communicators (ncclCommDestroy; every rank calls it, no solve
 * running, the process group still alive) and returns their number, -1 on error. */
int da_rccl_unique_id(void *id128);
int da_rccl_shutdown(void);
da_result *da_solve_sharded_rccl(const float *kernel, int64_t n_in, int64_t n_out, const char *method0, const char *method1, int hard_dc,
                                 int decompose_dc, const float *qintervals, const float *latencies, int adder_size, int carry_size,
                                 int search_all_decompose_dc, int rank, int world, const void *id128, int64_t *stats3);
/* To be called by the all-reduce callback's owner when a collective failed (the callback returns nothing and must not unwind
 * through the library): the running da_solve_sharded stops at the next exchange and fails with a runtime error instead of
 * continuing with a buffer that was not reduced. */
void da_comm_abort(void);
/* int32 elements handed to all-reduce(sum) by the last da_solve_sharded / da_solve_sharded_rccl of this process (x 4 = bytes per rank and
 * exchange direction): the exchange volume of a column-sharded solve, for bench.py's c4 workload. */
int64_t da_shard_exchanged_elements(void);

/* ---- result access (da4ml.types.Pipeline / CombLogic / Op, bindings.cc:106-151) ---------------------------- */
int da_n_stages(const da_result *r);
/* index of the winning decompose_dc candidate when search_all_decompose_dc was set, else -1 */
int da_picked(const da_result *r);
/* info[0..4] = n_in, n_out, n_ops, carry_size, adder_size */
int da_stage_info(const da_result *r, int stage, int64_t *info);
/* inp_shifts[n_in], out_idxs[n_out], out_shifts[n_out], out_negs[n_out] (0/1), ops_i[n_ops,4] = id0,id1,opcode,data,
 * ops_f[n_ops,5] = qint.min,qint.max,qint.step,latency,cost */
int da_stage_copy(const da_result *r, int stage, int64_t *inp_shifts, int64_t *out_idxs, int64_t *out_shifts, int64_t *out_negs,
                  int64_t *ops_i, float *ops_f);
/* stats[0..7] = greedy iterations, initial digits, -, selection rounds, peak pair blocks, re-read table slots,
 * partner rows updated, substituted digits -- summed over the chains run for this problem.  "Peak pair blocks" follows the
 * table only when the environment variable DA4ML_HIP_STATS=1 is set at the call (the update kernel then tallies the blocks it
 * creates and deletes: instrumentation, 1.8 % of a greedy step); without it the figure is the initial block count. */
int da_result_stats(const da_result *r, int64_t *stats);
/* Releases a result handle (NULL is ignored).  The op lists of the result are kept by the library for the next solve
 * (at most 1 GiB in total) instead of being returned to the allocator. */
void da_free(da_result *r);

/* ---- DAIS program executor (host) -------------------------------------------------------------------------- */
/* dais_bin.run_interp (reference src/da4ml/_binary/dais/bindings.cc:30-131 -> DAISInterpreter.cc:10-388; program layout
 * docs/dais.md:70-95 = CombLogic.to_binary()).  Integer-exact execution of `program` (int32 [n_words]) on `n_samples`
 * input rows (float64 [n_samples, n_in], row-major) into `outputs` (float64 [n_samples, n_out]); n_threads <= 0 = all
 * host threads, samples are split in chunks of at least 32 like the reference.  Runs on the host (the reference's does
 * too): the functional checker of solver results behind CombLogic.predict, not part of the solver path.
 * Returns DA_OK or DA_ERR_RUNTIME (message: da_dais_last_error, calling thread). */
int da_dais_run(const int32_t *program, int64_t n_words, const double *inputs, int64_t n_samples, double *outputs, int n_threads);
const char *da_dais_last_error(void);
/* Same execution with the executor chosen by `where`:
 *   DA_DAIS_HOST        the host block executor above;
 *   DA_DAIS_DEVICE      HIP kernel k_dais_run on the current device: one thread per sample, register file
 *                       [slot][sample] in HBM with liveness-compacted slots (csrc/dais_gpu.hip); fails without a GPU;
 *   DA_DAIS_HOST_SCALAR the device executor's per-value code (csrc/dais_core.h) run sample by sample on the host --
 *                       test aid that pins the shared arithmetic without a GPU.
 * No reference counterpart (the reference's interpreter is host-only); results are identical for all three. */
#define DA_DAIS_HOST 0
#define DA_DAIS_DEVICE 1
#define DA_DAIS_HOST_SCALAR 2
int da_dais_run_on(const int32_t *program, int64_t n_words, const double *inputs, int64_t n_samples, double *outputs, int n_threads,
                   int where);

/* ---- compiled DAIS executables: compile once, run many times ------------------------------------------------------ */
/* A handle for one DAIS program or a chain of `n_stages` of them (n_out of program s = n_in of program s+1); no reference
 * counterpart.  The result of a run is bit for bit that of running the programs one after the other with da_dais_run: the outputs
 * of stage s, (double)(neg ? -v : v) * out_scale and 0.0 for an absent output, are the raw inputs of stage s+1, quantised and
 * wrapped by its input statements -- for any input, in range or not (csrc/dais_core.h computes every value on every path).
 * da_dais_compile decodes and validates every program (the reference's messages; "stage s has n outputs, stage s+1 expects m
 * inputs"), assigns register slots once over the WHOLE chain -- an input statement of stage s+1 reads the value behind the
 * producing stage's output, so the register file is as large as the largest live set of the chain -- and, with a device present,
 * uploads statements, outputs and tables to the current device.  Without a device it compiles all the same; only the two device
 * modes of a run fail then.  Returns NULL on error (message: da_dais_last_error, calling thread). */
typedef struct da_dais_exec da_dais_exec;
da_dais_exec *da_dais_compile(int n_stages, const int32_t *const *programs, const int64_t *n_words);
/* info8 = stages, n_in, n_out, statements in total, slots, register-file variant chosen (0: HBM, the only one), register-file
 * bytes per sample, has table statements */
int da_dais_exec_info(const da_dais_exec *h, int64_t *info8);
/* scratch3 = address of the handle's register-file scratch on the device (0: none yet), its bytes, device
 * allocations made by runs so far: a steady run allocates nothing */
int da_dais_exec_scratch(const da_dais_exec *h, int64_t *scratch3);
/* Runs `n_samples` rows.  in / out: element type DA_DAIS_F64 or DA_DAIS_F32 (float inputs are widened exactly, float outputs are
 * the exact double rounded once), row strides in elements (>= n_in / n_out; the elements of a row are contiguous; elements
 * between the rows of `out` are left alone).  `where`:
 *   DA_DAIS_HOST, DA_DAIS_HOST_SCALAR  host pointers; the host block executor stage by stage / the device's per-value path over
 *                            the compiled chain and its slots (test aid, as for da_dais_run_on); `n_threads` as da_dais_run;
 *   DA_DAIS_DEVICE           host pointers, staged tile by tile through the handle's buffers; returns when the results are there;
 *   DA_DAIS_DEVICE_RESIDENT  device pointers of the current device (the one of da_dais_compile), used in place.  Everything is
 *                            queued on `stream` (a hipStream_t) and the call returns without waiting -- except that with
 *                            stream == NULL the handle's own stream is used and waited for, and that a chain with table
 *                            statements is waited for to turn the kernel's fault word into "Logic lookup index out of bounds".
 * Kernel k_dais_exec (csrc/dais_gpu.hip): one thread per sample, all stages in one launch per tile, nothing of an inner stage
 * goes to memory as a double.  Register file [slot][sample] in HBM: scratch of the handle, allocated at the first run, grown
 * only for a larger tile; tiles capped as for da_dais_run_on, DA4ML_DAIS_TILE honoured.
 * Runs of one handle are serialised by a mutex of the handle and share its scratch: hand one handle's resident runs to one
 * stream at a time.  Different handles are independent.  Returns DA_OK or DA_ERR_RUNTIME (da_dais_last_error). */
#define DA_DAIS_F64 0
#define DA_DAIS_F32 1
#define DA_DAIS_DEVICE_RESIDENT 3
int da_dais_exec_run(da_dais_exec *h, const void *in, int in_type, int64_t in_row_stride, int64_t n_samples, void *out, int out_type,
                     int64_t out_row_stride, int n_threads, int where, void *stream);
/* The same with an execution mode (da_dais_exec_run is this call with DA_DAIS_MODE_AUTO); every mode gives the same bits.
 *   DA_DAIS_MODE_SAMPLE  the statements in program order: kernel k_dais_exec, one thread per sample.  The duration of a call follows
 *                        the LENGTH of the statement list whatever n_samples is;
 *   DA_DAIS_MODE_LEVEL   the statements by dependency level: kernel k_dais_exec_level, a workgroup runs a tile of S samples (a power of
 *                        two, at most 16) with its lanes over (statement of the level, sample of the tile) and one barrier between
 *                        levels, so the duration of a small call follows the DEPTH of the graph.  Level of a statement: 0 when it reads
 *                        no value, else 1 + the largest level it reads (an inner stage's input reads the producing stage's output value).
 *                        The schedule has slots of its own: a slot is released when the level of its last reader is complete and handed
 *                        out to later levels only.  Value file [slot][S] in the workgroup's LDS when it fits beside the kernel's static
 *                        LDS, otherwise in a global scratch of the handle (allocated at the first such run, grown only when needed);
 *                        DA4ML_DAIS_LEVEL_LDS=0, read at every run, forces the global file;
 *   DA_DAIS_MODE_AUTO    LEVEL for n_samples <= 65 536 when the chain has at least 4 955 statements and at least 495 statements per level
 *                        on average, SAMPLE otherwise: the region in which the measurement (profiles/dais_level.txt, DESIGN.md section
 *                        10a) shows LEVEL faster -- 1.4x at 65 536 rows to 170x at one row; at 10^6 rows SAMPLE is 1.2x to 2.4x faster.
 *                        DA4ML_DAIS_MODE=sample|level, read at every run, decides in place of this rule; it does not touch an explicit
 *                        mode.
 * The mode applies to DA_DAIS_DEVICE and DA_DAIS_DEVICE_RESIDENT.  With DA_DAIS_HOST_SCALAR, LEVEL runs the level schedule over its slots
 * on the host, every level back to front (test aid); DA_DAIS_HOST ignores the mode.  An unknown mode is DA_ERR_RUNTIME. */
#define DA_DAIS_MODE_AUTO 0
#define DA_DAIS_MODE_SAMPLE 1
#define DA_DAIS_MODE_LEVEL 2
int da_dais_exec_run_mode(da_dais_exec *h, const void *in, int in_type, int64_t in_row_stride, int64_t n_samples, void *out, int out_type,
                          int64_t out_row_stride, int n_threads, int where, void *stream, int mode);
/* Writes min(n, 5) values: levels of the level schedule, statements in its widest level, its slots, what the last device run of the
 * handle was (-1: none yet, 0: sample, 1: level with the value file in LDS, 2: level with the global file), samples per tile S of the
 * last level run (0: none yet) */
int da_dais_exec_info2(const da_dais_exec *h, int64_t *out, int n);
/* The level schedule, for inspection: rows6 = [statements in total][6] in the schedule's order = statement number in program order over
 * the whole chain, level, slot written, slots read (operand a -- for an inner stage's input the producing output's value --, b, c; -1:
 * none); out_slots (may be NULL) = [n_out] slots of the last stage's outputs (-1: absent) */
int da_dais_exec_level_schedule(const da_dais_exec *h, int64_t *rows6, int64_t *out_slots);
void da_dais_exec_free(da_dais_exec *h);

/* ---- instrumentation for the benchmark harness ------------------------------------------------------------- */
/* t[31] = chains summed over the sampled launches; t[30] = capacity retries; t[18..29] = shader-clock cycles per kernel phase (7 of k_iter_select, 5 of k_iter_update);
 * t[0..17] = loop_ms (HIP events around the greedy-loop launches), dist_ms, total_ms, lockstep iterations,
 * greedy iterations, table groups re-read, partner rows, chains, table bytes, arena bytes, sampled k_iter_select ms,
 * sampled k_iter_update ms, number of samples, count blocks found, count blocks inserted, partner cells read,
 * count-block bytes (2K per touched block), partner-cell bytes -- accumulated since the last reset */
int da_timings(double *t, int reset);  /* (blocks found / created are tallied only under DA4ML_HIP_STATS=1, see da_result_stats) */
/* Further engine counters, same accumulation and reset as da_timings (call BEFORE a resetting da_timings); writes min(n, 16) values:
 * out[0] algorithmic bytes of k_iter_select (device-counted), out[1] host ms spent queueing greedy-loop
 * launches, out[14] chains that ran the many-column form of the selection kernel, the others reserved; returns the number written */
int da_engine_stats(double *out, int n);

#ifdef __cplusplus
}
#endif
#endif /* DA4ML_HIP_H */
