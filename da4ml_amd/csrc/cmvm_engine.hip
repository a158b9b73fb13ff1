// cmvm_engine.hip -- hand-written HIP kernels (gfx950 / CDNA4, wave64) for the CMVM greedy engine.  No CUDA
// compatibility layer, no dual paths: this file only targets MI355X.
// DEVICE CODE ONLY: bench.py's source_digest() hashes this file as what the kernels are compiled from, so a host edit must not
// touch it.  The HIP implementation of da::Backend that launches them is in the hip_*.h headers included at the end of the file.
//
// Reference loops replaced:
//   k_prepare        _center + global digit width            bit_decompose.hh:25-34, bit_decompose.cc:22-27
//   k_init_cells     CSD recoding + SparseExpr build          bit_decompose.cc:28-42, state_opr.cc:93-112
//                    (the digits are digit_masks' of cmvm_core.h: the CSD form, or another minimal signed-digit form a chain asks for)
//   k_init_pairs     all-pairs enumeration / FreqMap::initialize   state_opr.cc:117-143, types.hh:73-100
//   k_iter_select2   idx_mc / idx_mc_dc / idx_wmc / idx_wmc_dc + update_expr   indexers.cc:6-90, state_opr.cc:227-283
//                    (two workgroups per chain: the search finds the next pick one step AHEAD, beside the substitution of the current one;
//                    ordinary and column-sharded chains alike -- the one-block k_iter_select of rounds 1-5 is gone)
//   k_iter_update    update_stats (purge + regenerate) as an exact incremental update   state_opr.cc:285-345
//   k_extract        digit gather of to_solution             cmvm_core.cc:103-113
//   k_col_dist       stage-1 CSD Hamming distances           mat_decompose.cc:75-93
//
// Data layout in HBM, per chain (all arrays carved from one arena, see carve_chain in hip_chain_setup.h):
//   rlist   row lists: every row is a list of (column, cell) entries sorted by column.  The n_in input rows are DENSE
//           (n_out entries, entry j = column j); every later row is SPARSE: it only ever holds the columns it was
//           created with (digits only disappear from a row), so a typical row is one 128-byte line.  A cell holds the
//           digits of (row, column) as two position bitmasks (cmvm_core.h).  Narrow layout (n_out <= 256, <= 12 digits):
//           one u32 per entry = col:8 | minus:12 | plus:12; wide layout: 16 bytes = u64 cell + u32 col.
//   rowoff  [rcap] {offset, length} of every row's list (bump-allocated in creation order)
//   rows    [rcap]         RowInfo interval + latency of every row
//   collist [n_out][lcap]  u64     rows that have (had) digits in a column, ascending: row:24 | len:12 | off:28 (digit
//                                  gather at the end; the column-sharded chain's flags)
//   colbits [n_out][rcap/32]       bit r of column j: row r has digits in column j NOW; the partner rows of a greedy step are
//                                  the OR of the substituted columns' bitmaps
//   table   C slots (power of two), open addressing on (id0,id1):
//             hkey[C] u64 (16 keys = one 128-byte line = one probe bucket), hrank[C] u32 (selection rank of the block's
//             best key, 0 = none; the array the selection re-reads), hblk[C] one PAYLOAD LINE per slot:
//             {n_overlap, |dlat|, rank copy, index of the best key, K x u16 exact occurrence counts} -- a block update
//             reads and writes ONE line instead of four arrays; hidx[C] u8 behind hrank: the best key's index once more, dense (the search
//             reads rank, key and index of a whole group from three dense arrays)
//   grec    [C / GS]       32 B    per group of GS consecutive slots: bound word (rank << 32 | tie_word >> 23) of its best entry, the highest value an
//                                  update lowered in the group (glow), the best entry's exact tie word, flag "tie word unknown" (GroupRec)
//
// The reference keeps a sorted table of all pairs with count >= 2, purges every entry touching the two
// substituted rows and regenerates their pairs against ALL rows every iteration.  Here the counts are
// maintained exactly by subtracting, for every "partner" row that shares a substituted column, the pair
// occurrences of the consumed digits, and by creating the blocks of the new row -- O(consumed digits x
// column population) instead of O(row digits x all rows) per iteration.  Selection never scans the table:
// it keeps per-group bounds of the rank -- tight ones: an update that lowers a group's best entry leaves a mark (glow) that the next
// selection acts on --, and a step changes only entries of its pick's rows, so the best entry it leaves untouched is the next pick unless
// one of the few entries the update lists beats it (k_iter_select2).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <numeric>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "cmvm_core.h"
#include "cmvm_geometry.h"
#include "cmvm_gpu.h"
#include "cmvm_host.h"

namespace da {
namespace gpu {

constexpr uint64_t KEY_EMPTY = ~0ull;
// Tombstones carry the low two bits of the launch that wrote them (KEY_TOMB - id, id = 0..3).  A slot freed in a
// launch is never re-used within the SAME launch: the deleting wave's stores to the slot (counts, rank, tombstone)
// and a re-using wave's stores would otherwise be unordered (different waves, possibly different XCD L2s).  Kernel
// boundaries order everything, so the slot is claimable from the next launch on.
constexpr uint64_t KEY_TOMB = ~0ull - 1;
constexpr uint64_t KEY_TOMB_LO = KEY_TOMB - 3;  // keys >= KEY_TOMB_LO and != KEY_EMPTY are tombstones
constexpr int WAVE = 64;
constexpr int UPD_THREADS = 256;   // k_iter_update block
constexpr int UPD_WAVES = UPD_THREADS / WAVE;
#ifndef DA_MAX_GROUPS
#define DA_MAX_GROUPS 2048  // group records the search sweeps every step (16 waves x 64 lanes x 2).  Measured (MI355X, round 6, C3 batch / one chain, us per step; slots of a
                            // group read held in registers: DA_SEL_RK x 64): 4096 x 512 slots (RK 8) 34.4 / 23.0; 2048 x 1024 (RK 16) 33.1 / 22.2, (RK 8) 40.5 / 25.3; 1024 x 2048 (RK 16) 47.4 / 28.1
#endif
constexpr int MAX_GROUPS = DA_MAX_GROUPS;
#ifndef DA_IDS_LDS
#define DA_IDS_LDS 2048  // partner row ids of a step staged in LDS by the substitution block (tests/emu builds with 16: its problems are small, both paths run)
#endif

// Per-phase shader-clock timers of k_iter_select2 / k_iter_update (tests/gpu_profile.py).  They cost SGPRs, VALU time and --
// every s_memtime is followed by a wait for all outstanding LDS and scalar operations -- latency on the dependent chain of
// the select kernel (eight of them per launch), so they are compiled in only with -DDA_PHASE_TIMERS (make PHASE_TIMERS=1).
#ifdef DA_PHASE_TIMERS
#define UPD_TIMER_DECL long long up[5] = {0, 0, 0, 0, 0}, u0 = clock64(), u1;
#define UPD_TIMER_MARK(i) \
    u1 = clock64();       \
    up[i] += u1 - u0;     \
    u0 = u1;
#ifndef DA_TIMER_STEP_LO
#define DA_TIMER_STEP_LO 0  // the phase timers accumulate over the steps [LO, HI) of a chain (a window of the chain: -DDA_TIMER_STEP_LO=.. -DDA_TIMER_STEP_HI=..)
#endif
#ifndef DA_TIMER_STEP_HI
#define DA_TIMER_STEP_HI 0x7FFFFFFF
#endif
#define DA_TIMED_STEP(t) ((t) >= DA_TIMER_STEP_LO && (t) < DA_TIMER_STEP_HI)
#define UPD_TIMER_FLUSH \
    if (lane == 0 && DA_TIMED_STEP(g->iter - 1))      \
        for (int q = 0; q < 5; ++q) atomicAdd(&g->st_phase[7 + q], (unsigned long long)up[q]);
#define SEL_TIMER_DECL long long tp[8];
#define SEL_TIMER_MARK(i) tp[i] = clock64();
#define SEL_TIMER_FLUSH \
    if (DA_TIMED_STEP(iter)) for (int q = 0; q < 7; ++q) g->st_phase[q] += (unsigned long long)(tp[q + 1] - tp[q]);
#define UPD_TIMER_PASS_END UPD_TIMER_MARK(4)
#elif defined(DA_UPD_TAIL)
// -DDA_UPD_TAIL (diagnostic build, tools/gpu_tail.py): how long the passes of k_iter_update's wavefronts last, by kind -- st_phase[7] cycles of all
// passes, [8] passes, [9] cycles / [10] number of the passes with a rare case (a key beyond its first bucket, a creation in a full bucket), [11] passes
// with a block creation and no rare case, st_qdiag[0] their cycles, [1] / [4] passes longer than 20 k / 40 k cycles, [5] lanes of groups with a rare case
#ifndef DA_TIMER_STEP_LO
#define DA_TIMER_STEP_LO 0
#endif
#ifndef DA_TIMER_STEP_HI
#define DA_TIMER_STEP_HI 0x7FFFFFFF
#endif
#define DA_TIMED_STEP(t) ((t) >= DA_TIMER_STEP_LO && (t) < DA_TIMER_STEP_HI)
#define UPD_TIMER_DECL long long up[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, u0 = clock64(), u1;
#define UPD_TIMER_MARK(i)
#define UPD_TIMER_PASS_END                                                        \
    {                                                                             \
        u1 = clock64();                                                           \
        const long long dt = u1 - u0;                                             \
        const bool cr = __ballot(gnew) != 0;                                      \
        up[0] += dt, up[1] += 1;                                                  \
        if (rare) up[2] += dt, up[3] += 1, up[8] += __popcll(rare);               \
        if (!rare && cr) up[4] += 1, up[5] += dt;                                 \
        up[6] += dt > 20000, up[7] += dt > 40000;                                 \
        u0 = clock64();                                                           \
    }
#define UPD_TIMER_FLUSH                                                           \
    if (lane == 0 && DA_TIMED_STEP(g->iter - 1)) {                                \
        for (int q = 0; q < 5; ++q) atomicAdd(&g->st_phase[7 + q], (unsigned long long)up[q]); \
        atomicAdd(&g->st_qdiag[0], (unsigned long long)up[5]);                    \
        atomicAdd(&g->st_qdiag[1], (unsigned long long)up[6]);                    \
        atomicAdd(&g->st_qdiag[4], (unsigned long long)up[7]);                    \
        atomicAdd(&g->st_qdiag[5], (unsigned long long)up[8]);                    \
    }
#define SEL_TIMER_DECL
#define SEL_TIMER_MARK(i)
#define SEL_TIMER_FLUSH
#else
#define UPD_TIMER_DECL
#define UPD_TIMER_MARK(i)
#define UPD_TIMER_PASS_END
#define UPD_TIMER_FLUSH
#define SEL_TIMER_DECL
#define SEL_TIMER_MARK(i)
#define SEL_TIMER_FLUSH
#endif

// -DDA_STEP_CLOCKS (diagnostic build): where a chain's step goes -- the two kernels' durations as the chain sees them (first block start to last
// block end) and the two gaps between them (kernel boundary + the wait for a place on a CU), in ticks of the 100 MHz real-time counter, summed over
// the steps into st_qdiag[0] (select), [1] (select -> update), [4] (update), [5] (update -> next select), [7] (steps counted)
#ifdef DA_STEP_CLOCKS
#define CLK_NOW() ((unsigned long long)__builtin_amdgcn_s_memrealtime())
#define CLK_MARK(g, par, slot, inverted) atomicMax(&(g)->clk[par][slot], (inverted) ? ~CLK_NOW() : CLK_NOW())
#ifndef DA_CLK_STEP_LO
#define DA_CLK_STEP_LO 0  // the sums cover the steps [LO, HI) of every chain (a window of the chain)
#endif
#ifndef DA_CLK_STEP_HI
#define DA_CLK_STEP_HI 0x7FFFFFFF
#endif
#define CLK_TIMED_STEP(t) ((t) >= DA_CLK_STEP_LO && (t) < DA_CLK_STEP_HI)
#else
#define CLK_MARK(g, par, slot, inverted)
#endif

// header of a pair block's payload line (16 bytes, followed by the K u16 counts)
struct BlkHdr {
    int ov;         // n_overlap of the two rows (indexers.cc:36-56)
    float dl;       // |latency difference| of the two rows
    uint32_t rank;  // copy of hrank[slot]
    uint32_t idx;   // key index of the block's best key
};

// Pointers read from a chain descriptor are "generic" pointers to the compiler, which emits FLAT memory instructions
// for them.  FLAT operations count in BOTH vmcnt and lgkmcnt, so every LDS wait (lgkmcnt(0)) would also wait for all
// global loads in flight and serialise the software-pipelined loads of the greedy-loop kernels.  The hot kernels
// therefore keep their table / row / list pointers in the global address space (GLOBAL instructions, vmcnt only).
#define DA_GLOBAL __attribute__((address_space(1)))
template <class T> __device__ __forceinline__ T *gen(DA_GLOBAL T *p) { return (T *)p; }  // for the HIP atomic API
// Wave-uniform values pinned into scalar registers at this point of the program.  The greedy-loop kernels read ~30 fields
// of their chain descriptor; left alone, the compiler sinks each scalar load behind the early-exit branch that first needs
// it and the prologue becomes a chain of 4-6 dependent scalar round trips to L2 (ISA reading, round 2).  Loading every
// field first and pinning the values before the first branch makes it ONE round trip: an empty asm that "uses" the
// register is a point the load cannot be moved past.
// (the explicit v_readfirstlane moves a value that the compiler fetched with a vector load of a uniform address into a scalar
// register; on a value that already lives in one it folds away)
template <class T> __device__ __forceinline__ T da_uniform(T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "pinned descriptor fields are 32- or 64-bit values");
    if constexpr (sizeof(T) == 4) {
        const int r = __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v));
        return __builtin_bit_cast(T, r);
    } else {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)u), hi = (unsigned int)__builtin_amdgcn_readfirstlane((int)(unsigned int)(u >> 32));
        return __builtin_bit_cast(T, ((unsigned long long)hi << 32) | lo);
    }
}
#define DA_PIN_ASM(x) do { x = da_uniform(x); asm volatile("" : "+s"(x)); } while (0)
template <class T> __device__ __forceinline__ void pin_one(T &v) { DA_PIN_ASM(v); }
template <class... T> __device__ __forceinline__ void pin_sgpr(T &...v) { (pin_one(v), ...); }
// The same for per-lane values, and a compiler-level fence for memory operations.  "Load early, use late": a loaded value
// that is first touched after pin_vgpr() / behind load_fence() is not waited for before that point, and loads in front of
// the fence are not sunk behind it -- the loads of a phase leave together instead of one round trip after the other.
#define DA_PIN_VASM(x) asm volatile("" : "+v"(x))
template <class T> __device__ __forceinline__ void pin_vone(T &v) { DA_PIN_VASM(v); }
template <class... T> __device__ __forceinline__ void pin_vgpr(T &...v) { (pin_vone(v), ...); }
__device__ __forceinline__ void load_fence() {
    asm volatile("" ::: "memory");         // the optimiser does not move memory operations across
    __builtin_amdgcn_sched_barrier(0);      // nor does the instruction scheduler move anything (e.g. a wait + v_readfirstlane of
}                                           // the first loaded value in front of the other loads)
__host__ __device__ __forceinline__ size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
typedef float da_f4 __attribute__((ext_vector_type(4)));
typedef int da_i4 __attribute__((ext_vector_type(4)));
typedef unsigned int da_u2 __attribute__((ext_vector_type(2)));
typedef unsigned long long da_ul2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ RowInfo load_row(const DA_GLOBAL RowInfo *rows, size_t i) {
    const da_f4 v = *reinterpret_cast<const DA_GLOBAL da_f4 *>(rows + i);
    return RowInfo{v.x, v.y, v.z, v.w};
}
__device__ __forceinline__ RowInfo pick_row(bool first, const RowInfo &a, const RowInfo &b) {  // field by field: the records stay in registers
    return RowInfo{first ? a.lo : b.lo, first ? a.hi : b.hi, first ? a.step : b.step, first ? a.lat : b.lat};
}
__device__ __forceinline__ void store_row(DA_GLOBAL RowInfo *rows, size_t i, const RowInfo &r) {
    *reinterpret_cast<DA_GLOBAL da_f4 *>(rows + i) = da_f4{r.lo, r.hi, r.step, r.lat};
}

// Row-list entry formats.  Narrow: u32 = col:8 | minus:12 | plus:12 (32 entries per 128-byte line); wide: 16 bytes.
template <class Cell> struct RowFmt;
template <> struct RowFmt<uint32_t> {
    using Entry = uint32_t;
    static __device__ __forceinline__ Entry pack(uint32_t col, uint32_t cell) { return (col << 24) | ((cell >> 16) << 12) | (cell & 0xFFFu); }
    static __device__ __forceinline__ uint32_t col(Entry e) { return e >> 24; }
    static __device__ __forceinline__ uint32_t cell(Entry e) { return (((e >> 12) & 0xFFFu) << 16) | (e & 0xFFFu); }
    static __device__ __forceinline__ Entry none() { return 0u; }
};
template <> struct RowFmt<uint64_t> {
    using Entry = da_ul2;  // x = cell, y = column
    static __device__ __forceinline__ Entry pack(uint32_t col, uint64_t cell) { return Entry{(unsigned long long)cell, (unsigned long long)col}; }
    static __device__ __forceinline__ uint32_t col(Entry e) { return (uint32_t)e.y; }
    static __device__ __forceinline__ uint64_t cell(Entry e) { return (uint64_t)e.x; }
    static __device__ __forceinline__ Entry none() { return Entry{0ull, 0ull}; }
};
// reference to a row as stored in the column lists and the partner list: row:24 | len:12 | off:28
constexpr int REF_ROW_BITS = 24, REF_LEN_BITS = 12, REF_OFF_BITS = 28;
__host__ __device__ __forceinline__ unsigned long long ref_pack(uint32_t row, uint32_t len, uint32_t off) {
    return (unsigned long long)row | ((unsigned long long)len << REF_ROW_BITS) | ((unsigned long long)off << (REF_ROW_BITS + REF_LEN_BITS));
}
__device__ __forceinline__ uint32_t ref_row(unsigned long long r) { return (uint32_t)r & ((1u << REF_ROW_BITS) - 1u); }
__device__ __forceinline__ uint32_t ref_len(unsigned long long r) { return (uint32_t)(r >> REF_ROW_BITS) & ((1u << REF_LEN_BITS) - 1u); }
__device__ __forceinline__ uint32_t ref_off(unsigned long long r) { return (uint32_t)(r >> (REF_ROW_BITS + REF_LEN_BITS)); }

// A table entry together with what a substitution needs of its two rows: the best entry a search found (64 bytes = one
// s_load_dwordx16 of the block that takes it up)
struct SpecPick {
    unsigned long long word;  // bound word of the entry (rank << 32 | tie >> 23); 0 = none / not usable
    unsigned long long tie;   // its full tie word (id1, id0, key index)
    da_u2 refA, refB;         // {offset, length} of the lists of rows id0 and id1
    RowInfo ra, rb;           // their records
};
static_assert(sizeof(SpecPick) == 64, "SpecPick is read as sixteen words");
struct CandEntry {  // a table entry by value: selection rank and tie word (id1, id0, key index)
    unsigned long long rank, tie;
};
#ifndef DA_CAND_CAP
#define DA_CAND_CAP 16  // measured (tools/spec_probe.cc, 64 / 128 square): never more than 8 of either.  (tests/emu builds with 2: its steps
#endif                  // overflow the lists often, so that the path on which the search block publishes the pick runs there all the time)
constexpr int CAND_CAP = DA_CAND_CAP, TOUCH_CAP = DA_CAND_CAP;

// Per-chain descriptor in device memory.  Pointers are raw device addresses into the arena.
// Per group of GS consecutive table slots (the search sweeps all of them every step):
struct alignas(32) GroupRec {
    unsigned long long ub;    // bound word (rank << 32 | tie_word >> 23) of the group's best entry: tight unless `glow` reaches it
    unsigned long long glow;  // the highest bound word a block's best entry had before an update LOWERED it, since the group was last verified: reaching the
                              // group's bound it says the bound is stale (group_note)
    unsigned long long gtie;  // full tie word of the group's best entry (valid while the group is clean)
    uint32_t dirty;           // 0: the tie word is exact (and the bound, unless glow reaches it); 1: an entry rose, the tie word is unknown
    uint32_t pad;
};
static_assert(sizeof(GroupRec) == 32, "group record");
struct ChainDev {
    // geometry (constant after set-up)
    int n_in, n_out, n_bits, K, Kpad, method, adder_size, carry_size;
    int rcap, lcap, gs_log2, n_groups;
    uint32_t C, cmask;
    // inputs
    const float *kernel;
    const float *qints;
    const float *lats;
    int32_t *xint;  // centred integer matrix [n_in][n_out]
    int8_t *shift0, *shift1;
    // state
    void *rlist;        // row-list entries (RowFmt<Cell>::Entry)
    da_u2 *rowoff;      // [rcap] {offset, length} of every row's list
    uint32_t rl_cap, rl_used;
    RowInfo *rows;
    uint32_t *stamp;
    unsigned long long *collist;
    int *collen;
    unsigned long long *hkey;
    uint32_t *hrank;
    unsigned char *hblk;  // [C] payload lines of (1 << pb_log2) bytes
    int pb_log2;
    GroupRec *grec;  // [n_groups] one 32-byte record per group of slots (two 16-byte loads per group in the search's sweep; an update's marks of a group land in ONE line)
    // per-iteration hand-off select -> update
    int *mcol;
    uint16_t *cmap;    // [n_out] 1 + index of a column among the substituted columns of this step, 0 = not substituted
    uint32_t *colbits; // [n_out][cb_words] bit r of column j: row r has digits in column j NOW.  The partner rows of a step are the
                       // OR of the substituted columns' bitmaps -- no list reads, no de-duplication, no stale entries
    int cb_words;
    uint32_t *pl_ids;  // [rcap] partner row ids of the step (before their list references are attached)
    void *mA, *mB;
    unsigned long long *plist;
    int m, n_partners;
    int claim_words;   // words of the optional LDS area in which the substitution block combines the row bitmaps of a young chain (0: none)
    uint32_t A, B, Nw;
    int pk_shift, pk_sub;  // the pick's key (shift, sub): the consumed B-role digits are the A-role ones moved by `shift`, signs flipped when `sub` (k_iter_update)
    // progress
    int n_rows, iter, done, error, unknown_hit;
    unsigned int n_live, n_used, live_peak;
    int4 *picks;
    // results of k_prepare
    int prep_nbits, prep_maxdcol;
    long long prep_digits, prep_pairs;
    // extraction
    uint32_t *fin_row;
    unsigned long long *fin_cell;
    uint32_t *fin_count;
    uint32_t *fin_start;           // [n_out + 1] exclusive prefix of fin_count
    uint32_t *pk_row;              // packed surviving digits, column major ...
    unsigned long long *pk_cell;   // ... and their cells
    float *pk_lat;                 // [n_rows] latency of every row
    int pk_cap;
    uint32_t pk_total;             // digits packed by k_pack (= fin_start[n_out])
    // column-sharded chains (cmvm_shard.h): the matrix handed to k_prepare has pn_out columns of which this chain holds
    // [col0, col0 + n_out); exchange buffers of the greedy step.  Ordinary chains: pn_out == n_out, col0 == 0.
    int pn_out, col0;
    int32_t *cs_init;             // [n_pairs][K] partial initial pair counts (summed over the ranks in place)
    int32_t *cs_flags;            // [(rcap + 3) / 4] 8-bit fields: row shares a substituted column
    uint32_t *cs_uni;             // [rcap] union of the partner rows of all ranks, ascending
    int cs_nuni;
    int32_t *cs_slab;             // [(3 cs_nuni + 6)][K] partial / summed count changes
    // statistics
    unsigned long long st_rescans, st_partners, st_matches, st_found, st_inserts, st_cells;
    // -log2f of non-power-of-two input steps (StepLog2, cmvm_core.h): table built by the host libm, nullptr / 0 when all steps are powers of two
    const uint32_t *step_mant;
    const float *step_tab;
    int n_step_mant;
    unsigned long long st_sel_bytes;  // algorithmic bytes of the selection steps (all but the group re-reads, which st_rescans prices)
    unsigned long long st_phase[12];  // shader-clock cycles per kernel phase (select: 0-6, update: 7-11)
    // ---- the next pick, known one step ahead (k_iter_select2: search_body / pick_body)
    SpecPick spec[2];              // [t & 1]: the best entry of the table of step t that touches neither row of step t's pick -- step t
                                   // does not change it --, left by the search block of step t for step t + 1 (word 0: none, or l_list overflowed)
    unsigned int c_n[2], l_n[2];   // [t & 1]: entries in c_list / l_list (c_n counts on past the capacity: an overflow is visible)
    CandEntry c_list[2][CAND_CAP]; // [t & 1]: every entry that touches a row of step t's pick or its new row and whose bound word reaches
                                   // spec[t & 1].word, as it stands AFTER step t: appended by the update of step t (zeroed by the selection of step t)
    CandEntry l_list[2][TOUCH_CAP];// [t & 1]: the entries of the table of step t that touch exactly one row of the pick and reach spec[t & 1].word,
                                   // listed by the search block: the update of step t passes on those it does not re-evaluate
    uint32_t *sp_cnt;              // [6][Kpad] exact counts of the six pairs among {A, B, new row}: select -> update
    unsigned long long st_fast;    // steps whose pick was known before the step began
    unsigned long long st_qphase[4];  // shader-clock cycles of the search block: bounds, arg-max (steps without a known pick), search, steps timed
#ifdef DA_STEP_CLOCKS
    unsigned long long clk[2][4];     // [step & 1]: ~(first select block start), last select block end, ~(first update block start), last update block end (s_memrealtime, 100 MHz)
#endif
    unsigned long long st_qdiag[9];   // (phase-timer builds) [5] steps whose work list held > 32 groups, [6] the longest work list, [7] passes over the whole table (pick not known ahead), [8] work-list entries in all; group re-reads that found a stale bound below the floor / of clean groups with an excluded
                                      // best entry; [2],[3] scratch; [4] sum over the steps of the longest wave's re-read rounds
    unsigned long long tie_seed;      // 0: ties are settled as the reference settles them; else the chain's seeded tie order (cmvm_core.h) -- a random restart.  Read by
                                      // the SEEDED instantiations of the kernels only (last field: the offsets the others use are what they were)
    float dc_weight;                  // latency-penalty weight of the -dc / -pdc methods (entry_rank, cmvm_core.h); the host always fills it, by default with the method's
                                      // constant.  Read by the WEIGHTED instantiations only: the others keep the constant as a literal (last field, as tie_seed was)
    uint32_t tie_order;               // which seeded tie order a chain with tie_seed != 0 runs (TIE_ORDER_*, cmvm_core.h).  Read by the SEEDED instantiations only (last field again)
    uint32_t slack;                   // score slack of the chain (entry_rank_slack, cmvm_core.h), 0 .. 255; 0: none.  Read by the SLACK instantiations only (last field again)
};

__constant__ Log2Table c_log2;

// ------------------------------------------------------------------------------------------------ wave helpers
__device__ __forceinline__ int lane_id() { return threadIdx.x & (WAVE - 1); }
__device__ __forceinline__ int wave_id() { return threadIdx.x / WAVE; }

// Wave-wide reductions on the DPP path (row shifts inside the 16-lane rows, then the two row broadcasts of gfx9): six
// VALU operations per 32-bit word and no LDS round trip.  (The __shfl_xor butterflies they replace go through
// ds_bpermute -- about 900 cycles per 64-bit reduction, which dominated the arg-max loop of the selection.)
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint32_t dpp_u32(uint32_t identity, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)identity, (int)v, CTRL, ROW_MASK, 0xF, false);
}
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;
#define DA_DPP_REDUCE32(v, ident, OP)                                   \
    v = OP(v, dpp_u32<DPP_ROW_SHR1, 0xF>(ident, v));                    \
    v = OP(v, dpp_u32<DPP_ROW_SHR2, 0xF>(ident, v));                    \
    v = OP(v, dpp_u32<DPP_ROW_SHR4, 0xF>(ident, v));                    \
    v = OP(v, dpp_u32<DPP_ROW_SHR8, 0xF>(ident, v));                    \
    v = OP(v, dpp_u32<DPP_ROW_BCAST15, 0xA>(ident, v));                 \
    v = OP(v, dpp_u32<DPP_ROW_BCAST31, 0xC>(ident, v));
__device__ __forceinline__ uint32_t uadd32(uint32_t a, uint32_t b) { return a + b; }
// inclusive prefix sum over the wave (the same DPP sequence leaves the running sums in every lane)
__device__ __forceinline__ uint32_t wave_scan_add_u32(uint32_t v) {
    DA_DPP_REDUCE32(v, 0u, uadd32)
    return v;
}
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t smin32(uint32_t a, uint32_t b) { return (int)a < (int)b ? a : b; }
__device__ __forceinline__ int wave_min_i32(int v) {
    uint32_t x = (uint32_t)v;
    DA_DPP_REDUCE32(x, 0x7FFFFFFFu, smin32)
    return __builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    DA_DPP_REDUCE32(v, 0u, umax32)
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned long long dpp_max_u64(unsigned long long v) {
    const uint32_t lo = dpp_u32<CTRL, ROW_MASK>(0u, (uint32_t)v), hi = dpp_u32<CTRL, ROW_MASK>(0u, (uint32_t)(v >> 32));
    const unsigned long long t = ((unsigned long long)hi << 32) | lo;
    return t > v ? t : v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    v = dpp_max_u64<DPP_ROW_SHR1, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_SHR2, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_SHR4, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_SHR8, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_BCAST15, 0xA>(v);
    v = dpp_max_u64<DPP_ROW_BCAST31, 0xC>(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}
// Make this wave's LDS traffic visible to its own lanes: wait for outstanding LDS operations only (lgkmcnt(0));
// global loads stay in flight.  LDS operations of one wave complete in order, so no wider fence is needed for the
// per-wave counters; the wave barriers stop the compiler from moving LDS accesses across.
__device__ __forceinline__ void lds_fence() {
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
}

// Slot hash of a row pair.  32-bit arithmetic only: since the partner rows moved from wavefronts to 16-lane groups the
// hash is computed in vector registers (twice per group and pass), and the 64-bit multiplies of a 64-bit finaliser were
// ~15 % of the update kernel's vector instructions.  Two odd multipliers combine the ids, then the "lowbias32" finaliser;
// the placement of a block never influences a result, only probe lengths.
__device__ __forceinline__ uint32_t hash_pair(uint32_t lo, uint32_t hi) {
    uint32_t h = lo * 0x9E3779B1u + hi * 0x85EBCA77u;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ unsigned long long pack_pair(uint32_t lo, uint32_t hi) {
    return ((unsigned long long)hi << 32) | lo;
}
// group bound word: selection rank in the high half, the 32 most significant bits of the tie word below it, so
// that among equal ranks only groups holding the newest rows have to be inspected
__device__ __forceinline__ unsigned long long bound_word(uint32_t rank, unsigned long long tie) {
    return ((unsigned long long)rank << 32) | (tie >> 23);
}

// ------------------------------------------------------------------------------------------------ table ops
// Register-resident copy of the constant part of a chain descriptor (wave-uniform, lives in SGPRs); `g` is used
// for the few mutable counters only.
struct Ctx {
    int n_out, n_bits, K, Kpad, method, gs_log2, pb_log2;
    uint32_t cmask, windows;
    DA_GLOBAL unsigned long long *hkey;
    DA_GLOBAL uint32_t *hrank;
    DA_GLOBAL unsigned char *hblk;
    DA_GLOBAL GroupRec *grec;
    const DA_GLOBAL RowInfo *rows;
    ChainDev *g;  // derived from the kernel argument: already known to be global
    unsigned long long tomb;  // this launch's tombstone value
    unsigned long long rword;  // k_iter_update: bound word of the best entry this step leaves untouched (0: none); the best entry of every block
    unsigned int *cn;          // written or re-evaluated whose bound word reaches it is appended to cl[(*cn)++] (fold_entry): together with that
    CandEntry *cl;             // entry they are all the next selection has to compare
    unsigned long long seed;   // the chain's tie seed in the SEEDED instantiations (never 0 there), the constant 0 in the others
};

// ---- tie order of a chain.  SEEDED is a template parameter of every kernel that forms, compares or takes apart a tie word, as MANYCOL is of the
// selection kernel: the unseeded instantiations are instruction for instruction what they were, a seeded chain pays one 48-bit multiply per word.
// A seeded chain runs one of two orders (TIE_ORDER_*, cmvm_core.h): `order`, uniform per chain, read from the descriptor by the SEEDED instantiations
// only and held beside the chain context -- by the block evaluator in the kernels that write blocks, in a scalar of its own in the selection --, not
// in it: the unseeded kernels are built from the same Ctx and carry none of it.  Both orders are one expression (tie_pair_mix with an order); the
// within-block order (blk_pos) is the same for both.
// Every site goes through these three (the code that writes blocks: through the block evaluator below, which is built on them): a tie word
// formed one way and compared with one formed the other gives picks that are valid adder graphs but not the maximum of the chain's order.
template <bool SEEDED> __device__ __forceinline__ unsigned long long tie_of(uint32_t id0, uint32_t id1, int idx, unsigned long long seed, uint32_t order) {
    if constexpr (SEEDED)
        return tie_word_seeded(id0, id1, idx, seed, order);
    else
        return tie_word(id0, id1, idx);
}
template <bool SEEDED> __device__ __forceinline__ void tie_rows(unsigned long long tie, unsigned long long seed, uint32_t order, uint32_t &id0, uint32_t &id1) {
    unsigned long long h = tie >> 7;
    if constexpr (SEEDED) h = tie_pair_unmix(h, seed, order);
    id0 = (uint32_t)(h & 0xFFFFFFu);
    id1 = (uint32_t)(h >> 24);
}
// key index <-> position in the within-block order (the low byte of a block's `rank << 8 | position` maximum): an involution
template <bool SEEDED> __device__ __forceinline__ uint32_t blk_pos(uint32_t k, unsigned long long seed) {
    if constexpr (SEEDED)
        return tie_block_pos(k, seed);
    else
        return k;
}

// ---- rank of a table entry.  WEIGHTED is a template parameter of the kernels that form ranks (k_init_pairs, k_iter_update), as SEEDED is: a chain
// whose weight is its method's constant runs the instantiations that hold the constant as a literal -- register for register what they were --,
// a chain with another weight carries its bits (`dcw`) in a scalar register: read from the descriptor with the other fields of the step, held by
// the block evaluator below (the chain context stays what it was: the selection kernel, which forms no rank, is built from it too).
// The evaluator is the only caller: a rank formed past it, on the constant, gives valid graphs whose picks depend on where a block lies in the table.
template <bool WEIGHTED> __device__ __forceinline__ uint32_t rank_of(const Ctx &c, uint32_t dcw, uint32_t n, int ov, float dl) {
    if constexpr (WEIGHTED)
        return entry_rank(n, ov, dl, c.method, u2f(dcw));
    else
        return entry_rank(n, ov, dl, c.method);
}

// ---- block evaluator: how the counts of a pair block become its best entry.  Every code path that writes a block's counts (table_insert, table_update,
// and in update_partners the side-by-side re-evaluation and the block creation) forms its candidates, keeps the best and takes it apart HERE, so the
// chain's rank (weight) and tie order (seed) are threaded through one place.  It carries what a rank needs: the chain context and the weight bits.
// SLACK: the chain scores with a slack (entry_rank_slack, cmvm_core.h).  Such a chain always has a seed and reads its weight from the descriptor
// (the host fills in the method's constant where the job sets none): the SLACK instantiations exist with SEEDED and WEIGHTED only.  A rank then
// depends on the block's rows as well: `pw`, the per-block word of slack_pair_word, formed once per block by the code that walks its keys (0 and
// dead code in the other instantiations, which are instruction for instruction what they were).
template <bool SEEDED, bool WEIGHTED, bool SLACK = false> struct BlockEval {
    static_assert(!SLACK || (SEEDED && WEIGHTED), "a slack chain has a seed and carries its weight");
    const Ctx &c;
    uint32_t dcw;  // bits of the chain's latency-penalty weight in the WEIGHTED instantiations, unused (0) in the others
    uint32_t ord;  // the chain's seeded tie order (TIE_ORDER_*) in the SEEDED instantiations, unused (0) in the others
    uint32_t slk;  // the chain's score slack (1 .. 255) in the SLACK instantiations, unused (0) in the others
    // the per-block word of the slack's hash for the block of rows lo <= hi
    __device__ __forceinline__ uint32_t pair_word(uint32_t lo, uint32_t hi) const {
        if constexpr (SLACK)
            return slack_pair_word(lo, hi, c.seed);
        else
            return 0u;
    }
    // candidate word of key `k` with count `n` in a block of rows with overlap `ov`, latency difference `dl` and pair word `pw`: rank << 8 |
    // position in the within-block order, 0 = not selectable
    __device__ __forceinline__ unsigned long long candidate(uint32_t n, uint32_t k, int ov, float dl, uint32_t pw) const {
        uint32_t r;
        if constexpr (SLACK)
            r = entry_rank_slack(n, ov, dl, c.method, u2f(dcw), slk, slack_word_byte(pw, k));
        else
            r = rank_of<WEIGHTED>(c, dcw, n, ov, dl);
        return r ? (((unsigned long long)r << 8) | blk_pos<SEEDED>(k, c.seed)) : 0ull;
    }
    static __device__ __forceinline__ void fold(unsigned long long &best, unsigned long long cand) { best = cand > best ? cand : best; }
    // a block's best candidate word (the maximum over its keys) -> rank and key index of its best entry
    static __device__ __forceinline__ uint32_t rank_of_best(unsigned long long best) { return (uint32_t)(best >> 8); }
    __device__ __forceinline__ uint32_t idx_of_best(unsigned long long best) const { return blk_pos<SEEDED>((uint32_t)(best & 0xFF), c.seed); }
    // tie word and bound word (0: nothing selectable) of the best entry (rank, idx) of the block of rows lo <= hi
    __device__ __forceinline__ unsigned long long tie(uint32_t lo, uint32_t hi, uint32_t idx) const { return tie_of<SEEDED>(lo, hi, (int)idx, c.seed, ord); }
    __device__ __forceinline__ unsigned long long word(uint32_t lo, uint32_t hi, uint32_t rank, uint32_t idx) const {
        return rank ? bound_word(rank, tie(lo, hi, idx)) : 0ull;
    }
};

// launch_id: 2 * iteration for k_iter_select2, 2 * iteration + 1 for k_iter_update (only the low two bits are used)
template <bool SEEDED = false> __device__ __forceinline__ Ctx make_ctx_raw(ChainDev *g, int launch_id) {
    Ctx c;
    c.tomb = KEY_TOMB - (unsigned long long)(launch_id & 3);
    c.n_out = g->n_out;
    c.n_bits = g->n_bits;
    c.K = g->K;
    c.Kpad = g->Kpad;
    c.method = g->method;
    c.gs_log2 = g->gs_log2;
    c.pb_log2 = g->pb_log2;
    c.cmask = g->cmask;
    c.windows = g->C;  // raw here (nothing is computed between the descriptor loads: they leave as ONE batch); ctx_finish() scales it
    c.hkey = (DA_GLOBAL unsigned long long *)g->hkey;
    c.hrank = (DA_GLOBAL uint32_t *)g->hrank;
    c.hblk = (DA_GLOBAL unsigned char *)g->hblk;
    c.grec = (DA_GLOBAL GroupRec *)g->grec;
    c.rows = (const DA_GLOBAL RowInfo *)g->rows;
    c.g = g;
    c.rword = 0;
    c.cn = nullptr;
    c.cl = nullptr;
    if constexpr (SEEDED)
        c.seed = g->tie_seed;
    else
        c.seed = 0;
    return c;
}
__device__ __forceinline__ void ctx_finish(Ctx &c) { c.windows = c.windows / WAVE ? c.windows / WAVE : 1; }  // after the fields are pinned
template <bool SEEDED = false> __device__ __forceinline__ Ctx make_ctx(ChainDev *g, int launch_id) {
    Ctx c = make_ctx_raw<SEEDED>(g, launch_id);
    ctx_finish(c);
    return c;
}
// payload line of a slot: 16-byte header, then the counts
__device__ __forceinline__ DA_GLOBAL unsigned char *blk_ptr(const Ctx &c, int slot) { return c.hblk + ((size_t)(uint32_t)slot << c.pb_log2); }
__device__ __forceinline__ BlkHdr load_hdr(const Ctx &c, int slot) {
    const da_i4 v = *reinterpret_cast<const DA_GLOBAL da_i4 *>(blk_ptr(c, slot));
    return BlkHdr{v.x, __int_as_float(v.y), (uint32_t)v.z, (uint32_t)v.w};
}
__device__ __forceinline__ void store_hdr(const Ctx &c, int slot, int ov, float dl, uint32_t rank, uint32_t idx) {
    *reinterpret_cast<DA_GLOBAL da_i4 *>(blk_ptr(c, slot)) = da_i4{ov, __float_as_int(dl), (int)rank, (int)idx};
}
__device__ __forceinline__ void store_best(const Ctx &c, int slot, uint32_t rank, uint32_t idx) {  // rank copy + best key index
    *reinterpret_cast<DA_GLOBAL da_u2 *>(blk_ptr(c, slot) + 8) = da_u2{rank, idx};
}
__device__ __forceinline__ uint32_t load_best_idx(const Ctx &c, uint32_t slot) { return *reinterpret_cast<const DA_GLOBAL uint32_t *>(blk_ptr(c, (int)slot) + 12); }
__device__ __forceinline__ DA_GLOBAL uint16_t *blk_cnt(const Ctx &c, int slot) { return reinterpret_cast<DA_GLOBAL uint16_t *>(blk_ptr(c, slot) + 16); }

// All table operations are executed by one full wavefront.  The table is probed in BUCKETS of 16 slots (one 128-byte
// line of keys), starting at the bucket the hash points into and continuing with the following buckets.  A key is
// always stored in the first bucket of its sequence that had a free slot, and slots never return to EMPTY, so a
// look-up stops at the first bucket that contains the key or an EMPTY slot.
constexpr uint32_t BUCKET = 16;

// look-up continuing at bucket number `first_bucket` of the sequence, 4 buckets (64 lanes) per step; slot or -1
__device__ int table_find_from(const Ctx &c, unsigned long long key, uint32_t h, uint32_t first_bucket) {
    const int lane = lane_id();
    const uint32_t b0 = (h & ~(BUCKET - 1)) + first_bucket * BUCKET;
    for (uint32_t w = 0; w < c.windows + 1; ++w) {
        uint32_t s = (b0 + w * WAVE + lane) & c.cmask;
        unsigned long long kk = c.hkey[s];
        unsigned long long hit = __ballot(kk == key);
        if (hit) return (int)((b0 + w * WAVE + (__ffsll((long long)hit) - 1)) & c.cmask);
        if (__ballot(kk == KEY_EMPTY)) return -1;
    }
    return -1;
}
__device__ __forceinline__ int table_find(const Ctx &c, unsigned long long key, uint32_t h) { return table_find_from(c, key, h, 0); }
// claim a slot for a key that is known to be absent: the first free (EMPTY or TOMB) slot in bucket order; -1 = full
__device__ int table_claim(const Ctx &c, unsigned long long key, uint32_t h) {
    const int lane = lane_id();
    const uint32_t b0 = h & ~(BUCKET - 1);
    for (uint32_t w = 0; w < c.windows + 1; ++w) {
        uint32_t s = (b0 + w * WAVE + lane) & c.cmask;
        unsigned long long kk = c.hkey[s];
        unsigned long long avail = __ballot(kk == KEY_EMPTY || (kk >= KEY_TOMB_LO && kk != c.tomb));
        while (avail) {
            int l = __ffsll((long long)avail) - 1;
            avail &= avail - 1;
            int ok = 0;
            if (lane == l) {
                ok = atomicCAS(gen(&c.hkey[s]), kk, key) == kk;
            }
            ok = __shfl(ok, l);
            if (ok) return (int)((b0 + w * WAVE + l) & c.cmask);
        }
    }
    return -1;
}

// A block's best (rank, key) changed from bound word `w_old` to `w_new` (0 = not selectable).  Invariant kept: a group's bound is TIGHT (the
// bound word of its best entry) unless glow[grp] reaches it; flags 0 = the stored tie word is exact too.
//   * the entry rose: it may be the group's best now -- raise the bound, tie word unknown (flag);
//   * it fell: remember the highest value that fell (glow).  If that reaches the group's bound, the group's best may have been lowered and the
//     bound is stale -- the selection sees it when it reads the bounds and re-reads such groups early, in wavefronts that would idle otherwise.
//     (Left to be found lazily, stale bounds pile up below the selection's floor and are all met together when the floor drops a rank class:
//     work lists of up to 4000 groups, 1 % of the launches > 140 us, measured in round 5.  Deciding it HERE needs the group's bound in the update
//     kernel: two more loads and four more registers per partner pass, + 1.5 .. 4 us per launch, measured.)
// Fire-and-forget atomics, nothing is read.
__device__ __forceinline__ void group_note(const Ctx &c, int slot, unsigned long long w_old, unsigned long long w_new) {
    const int grp = slot >> c.gs_log2;
    if (w_new > w_old) {
        atomicMax(gen(&c.grec[grp].ub), w_new);
        atomicOr(gen(&c.grec[grp].dirty), 1u);  // (a plain store of the flag and the lazy scheme without glow were A/B variants of round 6: profiles/r06_ab_engine.txt)
    } else {
        atomicMax(gen(&c.grec[grp].glow), w_old);
    }
}
// one lane: the best entry (rank > 0) of a block as it stands after this launch -- a candidate for the next pick if it reaches the
// entry the step leaves untouched (rare by construction: at most a handful per step)
__device__ __forceinline__ void fold_entry(const Ctx &c, uint32_t rank, unsigned long long tie) {
    if (c.rword && bound_word(rank, tie) >= c.rword) {
        const unsigned int at = atomicAdd(c.cn, 1u);
        if (at < (unsigned int)CAND_CAP) {
            c.cl[at].rank = rank;
            c.cl[at].tie = tie;
        }
    }
}
// best-key index of every slot as a dense byte array behind hrank (the selection's search reads ranks, keys and indices of a whole
// group in one round trip; the copy in the payload header is what the update kernel reads with the counts)
__device__ __forceinline__ DA_GLOBAL uint8_t *hidx_ptr(const Ctx &c) { return reinterpret_cast<DA_GLOBAL uint8_t *>(c.hrank + ((size_t)c.cmask + 1)); }

// one lane: publish a block just created in `slot` (its counts are stored by the lanes that hold them) -- header, rank and best-key index, the
// group's bound, the candidate list of the next pick.  `best`: the block's best candidate word
template <bool SEEDED, bool WEIGHTED, bool SLACK>
__device__ __forceinline__ void publish_new_block(const BlockEval<SEEDED, WEIGHTED, SLACK> &ev, int slot, uint32_t lo, uint32_t hi, int ov, float dl, unsigned long long best) {
    const Ctx &c = ev.c;
    const uint32_t rank = ev.rank_of_best(best), idx = ev.idx_of_best(best);
    store_hdr(c, slot, ov, dl, rank, idx);
    c.hrank[slot] = rank;
    hidx_ptr(c)[slot] = (uint8_t)idx;
    if (rank) {  // (the tie word is spelled at both uses: held in a variable it costs the SEEDED instantiations of k_iter_update two more VGPRs)
        group_note(c, slot, 0ull, bound_word(rank, ev.tie(lo, hi, idx)));
        fold_entry(c, rank, ev.tie(lo, hi, idx));
    }
}

// Store a complete block.  cnt_of(k) gives the count of key k; returns false when the table is full.
// Precondition: at least one count >= 2 (checked by the caller), key absent.  ra / rb: intervals of rows lo / hi.
// `tally`: count the new block in the chain's n_live here, with a device atomic.  k_iter_update passes false and adds its creations and deletions
// ONCE PER WORKGROUP: in the first thousands of steps of a chain hundreds of blocks are created and deleted per step, and one atomic each on the
// same line of the chain descriptor serialises in the L2 at ~12 ns apiece -- behind which every later load of the issuing wave waits (vmcnt is
// in-order): measured in round 6, k_iter_update of steps 0 - 2000 took 24.8 us for one chain where the late steps take 6.7.
template <bool SEEDED, bool WEIGHTED, bool SLACK, class CntFn>
__device__ bool table_insert(const BlockEval<SEEDED, WEIGHTED, SLACK> &ev, uint32_t lo, uint32_t hi, const RowInfo &ra, const RowInfo &rb, CntFn cnt_of, bool tally = true) {
    const Ctx &c = ev.c;
    int lane = lane_id();
    unsigned long long key = pack_pair(lo, hi);
    int slot = table_claim(c, key, hash_pair(lo, hi));
    if (slot < 0) {
        if (lane == 0) c.g->error = E_TABLE_CAPACITY;
        return false;
    }
    int ov = n_overlap(ra, rb);
    float dl = fabsf(ra.lat - rb.lat);
    unsigned long long best = 0;
    DA_GLOBAL uint16_t *cnt = blk_cnt(c, slot);
    const uint32_t pw = ev.pair_word(lo, hi);
    for (int k = lane; k < c.Kpad; k += WAVE) {
        uint32_t n = k < c.K ? cnt_of(k) : 0u;
        if (n > 65535u) c.g->error = E_COUNT_OVERFLOW;
        cnt[k] = (uint16_t)n;
        ev.fold(best, ev.candidate(n, (uint32_t)k, ov, dl, pw));
    }
    best = wave_max_u64(best);
    if (lane == 0) {
        publish_new_block(ev, slot, lo, hi, ov, dl, best);
        if (tally) atomicAdd(&c.g->n_live, 1u);  // no return value: fire-and-forget (the peak is sampled by the selection)
    }
    return true;
}

// one lane: publish the re-evaluated best key of a block (or delete the block when no count >= 2 is left)
// `best`: the block's best candidate word, 0 = nothing selectable
template <bool SEEDED, bool WEIGHTED, bool SLACK>
__device__ __forceinline__ void block_commit(const BlockEval<SEEDED, WEIGHTED, SLACK> &ev, int slot, unsigned long long key, const BlkHdr &h, unsigned long long best, int alive, bool tally = true) {
    const Ctx &c = ev.c;
    const uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
    const unsigned long long w_old = ev.word(lo, hi, h.rank, h.idx);  // bound word of the block's best entry as its header holds it
    if (!alive) {
        c.hrank[slot] = 0;
        c.hkey[slot] = c.tomb;
        if (tally) atomicSub(&c.g->n_live, 1u);  // (see table_insert)
        if (h.rank) group_note(c, slot, w_old, 0ull);
        return;
    }
    const uint32_t rank = ev.rank_of_best(best), idx = ev.idx_of_best(best);
    if (rank != h.rank) c.hrank[slot] = rank;
    if (rank != h.rank || idx != h.idx) store_best(c, slot, rank, idx);
    if (idx != h.idx) hidx_ptr(c)[slot] = (uint8_t)idx;
    if (rank != h.rank || (rank && idx != h.idx)) group_note(c, slot, w_old, ev.word(lo, hi, rank, idx));
    if (rank) fold_entry(c, rank, ev.tie(lo, hi, idx));  // changed or not: the block touches a row of the step
}

// Re-evaluate a block after its counts changed (new_cnt(k, old) -> new count); deletes it when no count >= 2 is left and returns true then (wave-uniform).
template <bool SEEDED, bool WEIGHTED, bool SLACK, class CntFn>
__device__ bool table_update(const BlockEval<SEEDED, WEIGHTED, SLACK> &ev, int slot, unsigned long long key, CntFn new_cnt, bool tally = true) {
    const Ctx &c = ev.c;
    int lane = lane_id();
    const BlkHdr h = load_hdr(c, slot);
    DA_GLOBAL uint16_t *cnt = blk_cnt(c, slot);
    unsigned long long best = 0;
    int alive = 0;
    const uint32_t pw = ev.pair_word((uint32_t)key, (uint32_t)(key >> 32));
    for (int k = lane; k < c.K; k += WAVE) {
        uint32_t old = cnt[k];
        uint32_t n = new_cnt(k, old);
        if (n != old) cnt[k] = (uint16_t)n;
        alive |= n >= 2;
        ev.fold(best, ev.candidate(n, (uint32_t)k, h.ov, h.dl, pw));
    }
    best = wave_max_u64(best);
    alive = __any(alive);
    if (lane == 0) block_commit(ev, slot, key, h, best, alive, tally);
    return !alive;
}

// one wave: a block exists while one of its counts is >= 2.  `cnt`: a count vector wherever it lies (LDS or global u32, an int32 slab of a sharded chain)
template <class CntPtr> __device__ __forceinline__ bool wave_any_ge2(CntPtr cnt, int K) {
    int f = 0;
    for (int k = lane_id(); k < K; k += WAVE) f |= cnt[k] >= 2;
    return __any(f);
}

// The six pairs among the rows a step modified -- A, B and the new row N --, by the row of the exact count vectors the substitution leaves for them
// (sp_cnt; the head of a sharded chain's slab): (A,A) (A,B) (B,B) (A,N) (B,N) (N,N).  `existed`: the pair may have a block already (the ones with N
// are new); `active`: the pair is one of its own (when the pick is a row with itself, those with B repeat those with A).
struct SpecialPair {
    uint32_t lo, hi;
    bool existed, active;
};
__device__ __forceinline__ SpecialPair special_pair(int row, uint32_t A, uint32_t B, uint32_t Nw) {
    const bool same = A == B;
    switch (row) {
    case 0: return SpecialPair{A, A, true, true};
    case 1: return SpecialPair{A, B, true, !same};
    case 2: return SpecialPair{B, B, true, !same};
    case 3: return SpecialPair{A, Nw, false, true};
    case 4: return SpecialPair{B, Nw, false, !same};
    default: return SpecialPair{Nw, Nw, false, true};
    }
}
// One wave: the block of such a pair is replaced by its exact counts `cnt` -- re-counted where it exists (deleted when no count >= 2 is left),
// created where it does not and a count reaches 2.  ra / rb: records of rows lo / hi.  Either way the block's best entry is passed to fold_entry.
template <bool SEEDED, bool WEIGHTED, bool SLACK, class CntPtr>
__device__ __forceinline__ void replace_block(const BlockEval<SEEDED, WEIGHTED, SLACK> &ev, const SpecialPair &p, const RowInfo &ra, const RowInfo &rb, CntPtr cnt) {
    const unsigned long long key = pack_pair(p.lo, p.hi);
    const int slot = p.existed ? table_find(ev.c, key, hash_pair(p.lo, p.hi)) : -1;
    if (slot >= 0)
        table_update(ev, slot, key, [&](int k, uint32_t) { return (uint32_t)cnt[k]; });
    else if (wave_any_ge2(cnt, ev.c.K))
        table_insert(ev, p.lo, p.hi, ra, rb, [&](int k) { return (uint32_t)cnt[k]; });
}

// ------------------------------------------------------------------------------------------------ k_prepare
// One block per chain: centring shifts, centred integer matrix, digit width, digit statistics.
__global__ void __launch_bounds__(256) k_prepare(ChainDev *chains) {
    ChainDev &ch = chains[blockIdx.x];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int *s_dcol = reinterpret_cast<int *>(smem);  // [n_out]
    __shared__ unsigned int s_max;
    __shared__ unsigned long long s_digits, s_pairs;
    __shared__ int s_maxd;
    const int n_in = ch.n_in, n_out = ch.pn_out;  // the whole matrix (a column-sharded chain holds a slice of it)
    const float *k = ch.kernel;
    if (threadIdx.x == 0) {
        s_max = 0;
        s_digits = 0;
        s_pairs = 0;
        s_maxd = 0;
    }
    for (int j = threadIdx.x; j < n_out; j += blockDim.x) {
        int low = 127;
        for (int i = 0; i < n_in; ++i) low = min(low, lsb_loc(k[(size_t)i * n_out + j]));
        ch.shift1[j] = (int8_t)low;
        s_dcol[j] = 0;
    }
    __syncthreads();
    int nw = blockDim.x / WAVE;
    for (int i = wave_id(); i < n_in; i += nw) {
        int low = 127;
        for (int j = lane_id(); j < n_out; j += WAVE) low = min(low, lsb_loc(ldexpf(k[(size_t)i * n_out + j], -(int)ch.shift1[j])));
        low = wave_min_i32(low);
        if (lane_id() == 0) ch.shift0[i] = (int8_t)low;
        bool dead = ch.qints[3 * i] == 0.0f && ch.qints[3 * i + 1] == 0.0f;
        unsigned int mx = 0;
        for (int j = lane_id(); j < n_out; j += WAVE) {
            float v = ldexpf(ldexpf(k[(size_t)i * n_out + j], -(int)ch.shift1[j]), -low);
            int32_t x = (int32_t)v;
            ch.xint[(size_t)i * n_out + j] = x;
            mx = max(mx, (unsigned int)(x < 0 ? -x : x));
            if (!dead && x != 0) atomicAdd(&s_dcol[j], naf_weight(x));
        }
        mx = wave_max_u32(mx);
        if (lane_id() == 0) atomicMax(&s_max, mx);
    }
    __syncthreads();
    unsigned long long dig = 0, pairs = 0;
    int maxd = 0;
    for (int j = threadIdx.x; j < n_out; j += blockDim.x) {
        int d = s_dcol[j];
        dig += d;
        pairs += (unsigned long long)d * (d > 0 ? d - 1 : 0) / 2;
        maxd = max(maxd, d);
    }
    atomicAdd(&s_digits, dig);
    atomicAdd(&s_pairs, pairs);
    atomicMax(&s_maxd, maxd);
    __syncthreads();
    if (threadIdx.x == 0) {
        ch.prep_nbits = csd_width(s_max);
        ch.prep_digits = (long long)s_digits;
        ch.prep_pairs = (long long)s_pairs;
        ch.prep_maxdcol = s_maxd;
    }
}

// ------------------------------------------------------------------------------------------------ k_init_cells
// grid (ceil(n_out / 4), n_chains): one wave per column builds the entries of that column in the (dense) lists of the
// input rows and the column's row list.
// grid (blocks, chains): the state every chain starts from -- claim stamps, ranks, group bounds and row bitmaps zero, keys
// EMPTY (all ones), every group dirty.  16-byte stores; every array starts on a 256-byte boundary of the arena and is followed
// by padding up to the next one (Carver), so the last, partial 16 bytes of an array may be written whole.
__device__ __forceinline__ void fill16(void *p, size_t bytes, uint32_t v, size_t t0, size_t stride) {
    da_i4 *q = reinterpret_cast<da_i4 *>(p);
    const da_i4 w = da_i4{(int)v, (int)v, (int)v, (int)v};
    for (size_t i = t0, n = (bytes + 15) / 16; i < n; i += stride) q[i] = w;
}
__global__ void __launch_bounds__(256) k_init_state(ChainDev *chains) {
    const ChainDev &ch = chains[blockIdx.y];
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    fill16(ch.stamp, sizeof(uint32_t) * (size_t)ch.rcap, 0u, t0, stride);
    fill16(ch.hkey, sizeof(unsigned long long) * (size_t)ch.C, 0xFFFFFFFFu, t0, stride);
    fill16(ch.hrank, sizeof(uint32_t) * (size_t)ch.C, 0u, t0, stride);
    for (size_t i = t0; i < (size_t)ch.n_groups; i += stride) ch.grec[i] = GroupRec{0ull, 0ull, 0ull, 1u, 0u};
    fill16(ch.colbits, sizeof(uint32_t) * (size_t)ch.n_out * ch.cb_words, 0u, t0, stride);
}

// `recode`: the digit recoding of every chain of the launch (digit_masks, cmvm_core.h), in the order of `chains`; nullptr: all CSD.  A side
// array and not a field of ChainDev: the layout of the descriptor is code to every other kernel (DESIGN.md sections 4a, 4b, 4c).
struct ChainRecode {
    unsigned long long seed;
    uint32_t mode, pad;
};
template <class Cell> __global__ void __launch_bounds__(256) k_init_cells(ChainDev *chains, const ChainRecode *recode) {
    using O = CellOps<Cell>;
    using F = RowFmt<Cell>;
    ChainDev &ch = chains[blockIdx.y];
    const uint32_t rc_mode = recode ? recode[blockIdx.y].mode : RECODE_CSD;
    const uint64_t rc_seed = recode ? recode[blockIdx.y].seed : 0;
    int j = blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (j >= ch.n_out) return;
    auto *rl = reinterpret_cast<typename F::Entry *>(ch.rlist);
    int lane = lane_id(), len = 0;
    for (int base = 0; base < ch.n_in; base += WAVE) {
        int i = base + lane;
        Cell c = 0;
        if (i < ch.n_in) {
            bool dead = ch.qints[3 * i] == 0.0f && ch.qints[3 * i + 1] == 0.0f;
            uint32_t p, m;
            digit_masks(ch.xint[(size_t)i * ch.pn_out + ch.col0 + j], rc_mode, rc_seed, p, m);
            c = dead ? (Cell)0 : O::make(p, m);
            rl[(size_t)i * ch.n_out + j] = F::pack((uint32_t)j, c);  // dense row: entry j is column j, empty cells included
        }
        unsigned long long nz = __ballot(c != 0);
        if (lane < 2 && base + 32 * lane < ch.n_in) ch.colbits[(size_t)j * ch.cb_words + (base >> 5) + lane] = (uint32_t)(nz >> (32 * lane));
        if (c != 0)
            ch.collist[(size_t)j * ch.lcap + len + __popcll(nz & ((1ull << lane) - 1))] = ref_pack((uint32_t)i, (uint32_t)ch.n_out, (uint32_t)i * (uint32_t)ch.n_out);
        len += __popcll(nz);
    }
    if (lane == 0) ch.collen[j] = len;
    if (j == 0)
        for (int i = lane; i < ch.n_in; i += WAVE) {
            ch.rows[i] = RowInfo{ch.qints[3 * i], ch.qints[3 * i + 1], ch.qints[3 * i + 2], ch.lats[i]};
            ch.rowoff[i] = da_u2{(uint32_t)i * (uint32_t)ch.n_out, (uint32_t)ch.n_out};
        }
}

// exact pair counts of one pair of INPUT rows (dense lists) over all columns into LDS counters (one wave)
template <class Cell>
__device__ __forceinline__ void count_row_pair(const Ctx &c, const typename RowFmt<Cell>::Entry *rl, uint32_t lo, uint32_t hi, uint32_t *cnt) {
    using F = RowFmt<Cell>;
    int lane = lane_id();
    for (int k = lane; k < c.Kpad; k += WAVE) cnt[k] = 0;
    lds_fence();
    const auto *el = rl + (size_t)lo * c.n_out, *eh = rl + (size_t)hi * c.n_out;
    for (int j = lane; j < c.n_out; j += WAVE) {
        Cell a = F::cell(el[j]);
        if (!a) continue;
        if (lo == hi)
            for_pairs_self<Cell>(a, c.n_bits, [&](int k) { atomicAdd(&cnt[k], 1u); });
        else {
            Cell b = F::cell(eh[j]);
            if (b) for_pairs_cross<Cell>(a, b, c.n_bits, [&](int k) { atomicAdd(&cnt[k], 1u); });
        }
    }
    lds_fence();
}
// one wave per pair of input rows: pair index p = hi (hi + 1) / 2 + lo  ->  (lo, hi), lo <= hi
__device__ __forceinline__ void pair_of_index(long long p, uint32_t &lo, uint32_t &hi) {
    long long i1 = (long long)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (i1 * (i1 + 1) / 2 > p) --i1;
    while ((i1 + 1) * (i1 + 2) / 2 <= p) ++i1;
    hi = (uint32_t)i1, lo = (uint32_t)(p - i1 * (i1 + 1) / 2);
}

// ------------------------------------------------------------------------------------------------ k_init_pairs
// grid (ceil(n_pairs / 4), n_chains): one wave per initial row pair (i0 <= i1).
template <class Cell, bool SEEDED = false, bool WEIGHTED = false, bool SLACK = false> __global__ void __launch_bounds__(256) k_init_pairs(ChainDev *chains) {
    ChainDev *g = &chains[blockIdx.y];
    if (g->method == M_DUMMY) return;
    const Ctx c = make_ctx<SEEDED>(g, 0);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *cnt = reinterpret_cast<uint32_t *>(smem) + (size_t)wave_id() * c.Kpad;
    long long n_in = g->n_in;
    long long n_pairs = n_in * (n_in + 1) / 2;
    long long p = (long long)blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (p >= n_pairs) return;
    uint32_t lo, hi;
    pair_of_index(p, lo, hi);
    const auto *rl = reinterpret_cast<const typename RowFmt<Cell>::Entry *>(g->rlist);
    count_row_pair<Cell>(c, rl, lo, hi, cnt);
    if (!wave_any_ge2(cnt, c.K)) return;
    if (c.method < 0) {  // unknown method string with a non-empty table: the reference throws here
        if (lane_id() == 0) g->unknown_hit = 1;
        return;
    }
    table_insert(BlockEval<SEEDED, WEIGHTED, SLACK>{c, WEIGHTED ? f2u(g->dc_weight) : 0u, SEEDED ? g->tie_order : 0u, SLACK ? g->slack : 0u}, lo, hi, load_row(c.rows, lo), load_row(c.rows, hi), [&](int k) { return cnt[k]; });
}

// ================================================================================= k_iter_select2: the next pick, one step ahead
// A greedy step changes only table entries that touch the two rows of its pick (A, B) or the row it creates (N).  So the
// best entry R_t of the table of step t that touches neither A_t nor B_t is still in the table of step t + 1, unchanged, and
// the pick of step t + 1 is the largest of R_t and the entries that touch A_t, B_t or N_t.  Of those only the ones that reach
// R_t matter, and there are hardly ever any (tools/spec_probe.cc: none in 88 % of the steps, never more than 8).  The selection
// of a step is split into two workgroups per chain that run side by side:
//   * the SEARCH block (search_body, blockIdx.y == 0) looks for R_t -- the lazy arg-max over the group bounds with the entries
//     of A_t / B_t left out -- and lists the entries that touch exactly one of A_t / B_t and reach R_t (l_list): spec[t & 1];
//   * the update of step t appends the best entry of every block it writes or re-evaluates (partner blocks, the six blocks among
//     {A, B, N}) that reaches R_t to c_list[t & 1], changed or not (fold_entry), and passes on the entries of l_list whose block
//     it does not visit (the other row is not a partner row: the entry is unchanged);
//   * the SUBSTITUTION block (pick_body, blockIdx.y == 1) of step t + 1 takes the largest of R_t and c_list[t & 1] as its pick:
//     no bounds, no arg-max in front of the substitution.  Only when there is no R_t or a list overflowed (the first step of a chain) does it
//     find the pick itself -- a plain arg-max over the dense rank array (table_argmax_block) --, as does the search block for its own purpose
//     (through the bounds): the two blocks never wait for each other.
// Exactness: an entry of the table of step t + 1 either touches none of A_t, B_t, N_t -- then it is at most R_t --, or its block
// was written / re-evaluated by the update -- then its best entry is in c_list if it reaches R_t --, or it touches A_t or B_t
// and its block was not visited -- then it is unchanged since the search saw it, and in l_list -> c_list if it reaches R_t.
// "Reaches" is decided on bound words (rank << 32 | tie >> 23), which order coarser than (rank, tie): a superset; the pick is
// the maximum by (rank, tie) of the listed entries and R_t.
// Only the search block reads or writes group bounds; the table itself is not written by this kernel at all (the six special
// blocks moved to k_iter_update), so the two blocks share nothing but the descriptor fields named above.
constexpr uint32_t ROW_NONE = 0xFFFFFFFFu;
#ifndef DA_SEL2_THREADS
#define DA_SEL2_THREADS 1024  // measured (MI355X, round 5): 512 threads are slower, alone and in the batch (fewer waves share the group reads)
#endif
constexpr int SEL2_THREADS = DA_SEL2_THREADS;  // threads of a k_iter_select2 block (both roles); MAX_GROUPS / SEL2_THREADS group bounds per lane of the search
static_assert(MAX_GROUPS % SEL2_THREADS == 0 && SEL2_THREADS % WAVE == 0 && SEL2_THREADS >= 256, "k_iter_select2 geometry");
#ifndef DA_AB_REPAIR_ROUNDS
#define DA_AB_REPAIR_ROUNDS 8  // measured (MI355X, C3 batch / one chain, us per step): 0: 36.0 / 24.9, 1: 35.5 / 24.0, 2: 34.9 / 23.6, 4: 34.4 / 23.1, 8: 34.4 / 22.9
#endif
#ifndef DA_SEL_RK
#define DA_SEL_RK 16  // (see DA_MAX_GROUPS)
#endif
constexpr int QL_CAP = DA_CAND_CAP * 4;  // entries touching the pick's rows the search may meet above its rising floor before it gives up (LDS)

#ifdef DA_PHASE_TIMERS
#define Q_TIMER_DECL long long qp[4];
#define Q_TIMER_MARK(i) qp[i] = clock64();
#else
#define Q_TIMER_DECL
#define Q_TIMER_MARK(i)
#endif

// The table's best entry -- highest rank, then highest tie word -- by ONE WORKGROUP and a plain pass over the dense rank array: no bounds, nothing
// written.  For the substitution block of a step whose pick is not known ahead (the first step of a chain; an overflowed candidate list): 4 bytes per
// slot twice (8 + 8 MB for a 256x256 chain, once per chain).  rank 0: nothing selectable.  red_*: one LDS word per wave.  Ends with a block barrier.
template <bool SEEDED = false>
__device__ __forceinline__ void table_argmax_block(ChainDev *g, unsigned long long seed, uint32_t order, uint32_t &rank, unsigned long long &tie, uint32_t *red_rank, unsigned long long *red_tie) {
    const DA_GLOBAL uint32_t *hrank = (const DA_GLOBAL uint32_t *)g->hrank;
    const DA_GLOBAL unsigned long long *hkey = (const DA_GLOBAL unsigned long long *)g->hkey;
    const uint32_t C = g->C;
    const DA_GLOBAL uint8_t *hidx = reinterpret_cast<const DA_GLOBAL uint8_t *>(hrank + (size_t)C);
    const int tid = threadIdx.x, nthr = blockDim.x, lane = lane_id(), wid = wave_id(), nw = nthr / WAVE;
    typedef unsigned int da_u4 __attribute__((ext_vector_type(4)));
    const DA_GLOBAL da_u4 *hr4 = reinterpret_cast<const DA_GLOBAL da_u4 *>(hrank);  // (C is a multiple of 256, the array starts on a 256-byte boundary)
    uint32_t best = 0;
    for (uint32_t i = (uint32_t)tid; i < C / 4; i += (uint32_t)nthr) {
        const da_u4 v = hr4[i];
        best = max(max(best, v.x), max(max(v.y, v.z), v.w));
    }
    best = wave_max_u32(best);
    if (lane == 0) red_rank[wid] = best;
    __syncthreads();
    best = wave_max_u32(lane < nw ? red_rank[lane] : 0u);
    unsigned long long bt = 0;
    if (best != 0)
        for (uint32_t i = (uint32_t)tid; i < C / 4; i += (uint32_t)nthr) {
            const da_u4 v = hr4[i];
            const uint32_t r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (r[q] == best) {
                    const uint32_t sl = 4 * i + (uint32_t)q;
                    const unsigned long long k = hkey[sl];
                    const unsigned long long tw = tie_of<SEEDED>((uint32_t)k, (uint32_t)(k >> 32), (int)hidx[sl], seed, order);
                    bt = tw > bt ? tw : bt;
                }
        }
    bt = wave_max_u64(bt);
    if (lane == 0) red_tie[wid] = bt;
    __syncthreads();
    bt = wave_max_u64(lane < nw ? red_tie[lane] : 0ull);
    rank = best;
    tie = bt;
    __syncthreads();
}

// The pick of a step from what the previous step left: the best entry it did not touch (spec) against the candidates its update
// listed.  Every wave computes the same (one round trip when there are candidates, none otherwise).  false: no such entry, or a list
// overflowed -- the step finds its pick the long way.
__device__ __forceinline__ bool resolve_pick(const DA_GLOBAL CandEntry *cl, unsigned long long sp_word, unsigned long long sp_tie, unsigned int cn, unsigned long long &tie,
                                             bool &from_spec) {
    tie = sp_tie;
    from_spec = true;
    if (sp_word == 0 || cn > (unsigned int)CAND_CAP) return false;
    if (cn) {
        const int lane = lane_id();
        uint32_t r = 0;
        unsigned long long t = 0;
        if (lane < (int)cn) {
            r = (uint32_t)cl[lane].rank;
            t = cl[lane].tie;
        }
        const uint32_t br = wave_max_u32(r);
        const unsigned long long bt = wave_max_u64(r == br ? t : 0ull);
        const uint32_t rr = (uint32_t)(sp_word >> 32);
        if (br > rr || (br == rr && bt > sp_tie)) {
            tie = bt;
            from_spec = false;
        }
    }
    return true;
}

template <class Cell, bool SEEDED = false> __device__ __forceinline__ void search_body(ChainDev *g, int step) {
    constexpr int NW = SEL2_THREADS / WAVE, GPL = MAX_GROUPS / SEL2_THREADS;  // waves; group bounds per lane
    constexpr int RKN = DA_SEL_RK;  // slots per lane of a group read that are held in registers (x 64 lanes: groups of up to 512 slots in one round trip)
    const int par = step & 1;
    int was_done = g->done, had_error = g->error, n_groups = g->n_groups;
    unsigned long long sp_word = g->spec[par ^ 1].word, sp_tie = g->spec[par ^ 1].tie;
    unsigned int cn_prev = g->c_n[par ^ 1];
    Ctx c = make_ctx_raw<SEEDED>(g, 2 * step);
    uint32_t ord = 0;  // the chain's seeded tie order (SEEDED instantiations)
    if constexpr (SEEDED) ord = g->tie_order;
    const DA_GLOBAL da_u2 *rowoff = (const DA_GLOBAL da_u2 *)g->rowoff;
    const DA_GLOBAL CandEntry *cl_prev = (const DA_GLOBAL CandEntry *)&g->c_list[par ^ 1][0];
    DA_GLOBAL CandEntry *ll_out = (DA_GLOBAL CandEntry *)&g->l_list[par][0];
    pin_sgpr(was_done, had_error, n_groups, sp_word, sp_tie, cn_prev);
    pin_sgpr(c.gs_log2, c.cmask, c.hkey, c.hrank, c.grec, c.rows);
    pin_sgpr(rowoff, cl_prev, ll_out);
    if constexpr (SEEDED) pin_sgpr(c.seed, ord);
    if (was_done || had_error != E_OK) return;  // (the substitution block stops the chain)
    __shared__ unsigned long long q_floor, q_red_tie[NW], q_ub[GPL][SEL2_THREADS];
    __shared__ uint32_t q_work[MAX_GROUPS];  // groups still to be read after round 0: index into q_ub | dirty << 31
    __shared__ uint32_t q_sl[MAX_GROUPS];    // groups whose bound is stale (their best entry was lowered): index into q_ub
    __shared__ unsigned int q_wn, q_sn, q_stake;
    __shared__ uint32_t q_red_rank[NW];
    __shared__ CandEntry q_L[QL_CAP];
    __shared__ unsigned int q_Ln, q_Lout;
    const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
    const int gs = 1 << c.gs_log2;
    const DA_GLOBAL uint8_t *hidx = hidx_ptr(c);
    Q_TIMER_DECL
    Q_TIMER_MARK(0)
    const int GPW = (n_groups + NW - 1) / NW;  // wave w owns the groups [w * GPW, (w + 1) * GPW)
    unsigned long long pk_tie;
    bool from_spec;
    const bool fast = resolve_pick(cl_prev, sp_word, sp_tie, cn_prev, pk_tie, from_spec);
    uint32_t exA = ROW_NONE, exB = ROW_NONE;  // rows whose entries the pass leaves out
    if (fast) tie_rows<SEEDED>(pk_tie, c.seed, ord, exA, exB);
    unsigned int rescans = 0;
#ifdef DA_PHASE_TIMERS
    unsigned int q_stale = 0, q_touch = 0, q_rounds = 0;
#endif
    for (int pass = fast ? 1 : 0; pass < 2; ++pass) {
        // pass 0 (only when the pick is not known yet): the arg-max over the whole table -> the pick, published for the substitution block;
        // pass 1: the same with the entries of the pick's rows left out -> R; the entries that touch exactly one of the rows and reach the
        // floor of the moment are collected on the way (q_L)
        if (tid == 0) {
            q_floor = 0;
            q_Ln = 0;
            q_Lout = 0;
            q_wn = 0;
            q_sn = 0;
            q_stake = 0;
        }
        uint32_t nr = 0;  // this lane's best entry so far outside the excluded rows
        unsigned long long nt = 0;
        // returns the entry's bound word if it counts towards the floor, else 0; fl = the floor at the time (entries of the excluded rows are listed from there on)
        auto offer = [&](uint32_t r, unsigned long long tw, unsigned long long fl, bool list) -> unsigned long long {
            uint32_t i0, i1;
            tie_rows<SEEDED>(tw, c.seed, ord, i0, i1);
            const bool t0 = i0 == exA || i0 == exB, t1 = i1 == exA || i1 == exB;
            if (!(t0 || t1)) {
                if (r > nr || (r == nr && tw > nt)) {
                    nr = r;
                    nt = tw;
                }
                return bound_word(r, tw);
            }
            if (list && t0 != t1 && bound_word(r, tw) >= fl) {
                const unsigned int at = atomicAdd(&q_Ln, 1u);
                if (at < (unsigned int)QL_CAP) q_L[at] = CandEntry{(unsigned long long)r, tw};
            }
            return 0ull;
        };
        // ---- ONE vector round trip: bound, dirty flag and stored tie word of this lane's (up to GPL) groups; unconditional loads, index clamped
        // (behind an `in ? load : 0` the compiler waits for each load inside its own branch).  A clean group's bound and tie word are exact: its best entry is a candidate right away, or -- if it touches an
        // excluded row -- the group has to be read.  (The second pass of a launch reads what the first one tightened: fenced below.)
        // Groups that may have to be read -- dirty, or clean with an excluded best entry -- keep their bound in LDS (q_ub[u][tid], 0 = nothing to
        // read); a lane holds only its highest one in registers (top, top_u) and one bit per group: dirty.
        unsigned long long cl = 0, top = 0;
        int top_u = 0;
        uint32_t dmask = 0, rmask = 0;  // per group of this lane: not verified (a read tightens it) / bound stale (read in any case)
        {
            unsigned long long ubv[GPL], gtr[GPL], glv[GPL];
            uint32_t dv[GPL];
#pragma unroll
            for (int u = 0; u < GPL; ++u) {
                const int q = wid * GPW + lane + u * WAVE;
                const int qc = (lane + u * WAVE < GPW && q < n_groups) ? q : 0;
                const DA_GLOBAL da_i4 *rp = reinterpret_cast<const DA_GLOBAL da_i4 *>(&c.grec[qc]);  // the record as two 16-byte loads
                const da_i4 r0 = rp[0], r1 = rp[1];
                ubv[u] = ((unsigned long long)(uint32_t)r0.y << 32) | (uint32_t)r0.x;
                glv[u] = ((unsigned long long)(uint32_t)r0.w << 32) | (uint32_t)r0.z;
                gtr[u] = ((unsigned long long)(uint32_t)r1.y << 32) | (uint32_t)r1.x;
                dv[u] = (uint32_t)r1.z;
            }
#pragma unroll
            for (int u = 0; u < GPL; ++u) {
                const int q = wid * GPW + lane + u * WAVE;
                const bool in = lane + u * WAVE < GPW && q < n_groups;
                unsigned long long cand = 0;  // bound of a group that may have to be read
                if (in && ubv[u] != 0 && glv[u] >= ubv[u]) {  // an entry that had reached the bound was lowered: the bound may be stale.  Read by a wave that has nothing else to do (or, like any
                    cand = ubv[u] ? ubv[u] : 1ull;  // group, when the bound reaches the floor): the backlog stays short and never arrives all at once
                    dmask |= 1u << u;
                    rmask |= 1u << u;
                } else if (in && ubv[u] != 0) {
                    if (dv[u]) {
                        cand = ubv[u];
                        dmask |= 1u << u;
                    } else if (ubv[u] >= cl) {  // (a clean group below this lane's best so far cannot matter, whatever rows its best entry touches)
                        const unsigned long long w = offer((uint32_t)(ubv[u] >> 32), gtr[u], 0ull, false);  // (an excluded best entry is listed when its group is read)
                        if (w)
                            cl = max(cl, w);
                        else
                            cand = ubv[u];
                    }
                }
                q_ub[u][tid] = cand;
                if (cand > top && !(rmask >> u & 1u)) {  // (round 0 takes the highest group that has to reach the floor; the stale ones go to the work list)
                    top = cand;
                    top_u = u;
                }
            }
        }
        if (pass == (fast ? 1 : 0)) { Q_TIMER_MARK(1) }
        __syncthreads();  // q_floor and the list counters zeroed
        cl = wave_max_u64(cl);
        if (lane == 0 && cl) atomicMax(&q_floor, cl);
#pragma unroll
        for (int u = 0; u < GPL; ++u)
            if (rmask >> u & 1u) q_sl[atomicAdd(&q_sn, 1u)] = (uint32_t)(u * SEL2_THREADS + tid);
        __syncthreads();
        // read one group (by one wavefront): every slot whose rank reaches the floor's is a candidate (or, touching an excluded row, listed); a
        // dirty group's bound is tightened.  (All ranks, keys and indices in ONE round trip was measured too: 114 registers per thread, and a
        // 1024-thread block of this kernel then needs a CU without a single k_iter_update block -- in the batch 1 % of the launches waited
        // > 200 us for one.  This form fits the 64 registers of eight waves per SIMD.)
        auto read_group = [&](const uint32_t grp, const bool dirty, const unsigned long long /*bound*/, const unsigned long long fl) {
            const uint32_t base = grp * gs;
            // ---- round trip 1: the ranks of all slots (one dense array, coalesced; 8 slots per lane)
            uint32_t rk[RKN], grank = 0;
#pragma unroll
            for (int u = 0; u < RKN; ++u) {
                const int o = lane + u * WAVE;
                rk[u] = c.hrank[base + (o < gs ? o : 0)];
            }
            load_fence();
#pragma unroll
            for (int u = 0; u < RKN; ++u) {
                pin_vgpr(rk[u]);
                if (lane + u * WAVE >= gs) rk[u] = 0;
                grank = max(grank, rk[u]);
            }
            for (int o = lane + RKN * WAVE; o < gs; o += WAVE) grank = max(grank, c.hrank[base + o]);
            grank = wave_max_u32(grank);
            // only slots whose rank reaches the floor's can matter (the floor's own rank included: the tie word decides)
            // (a group that is not verified is left exact: at least its best slots are read)
            const uint32_t fr = (uint32_t)(fl >> 32), thr0 = fr ? fr : 1u, thr = dirty && grank != 0 && grank < thr0 ? grank : thr0;
            unsigned long long gt = 0, lw = 0;
            if (grank >= thr) {  // (wave-uniform: a clean group whose excluded best entry was all it held that high costs nothing beyond the ranks)
                // ---- round trip 2: key and best-key index of those slots -- a lane takes its slots one per turn, all lanes' loads of a turn in
                // flight together (nearly always a single turn: a handful of the 512 slots qualify)
                uint32_t want = 0;
#pragma unroll
                for (int u = 0; u < RKN; ++u) want |= rk[u] >= thr ? 1u << u : 0u;
                while (__any(want != 0)) {
                    if (want) {
                        const int u = ctz32(want);
                        want &= want - 1;
                        uint32_t r = rk[0];
#pragma unroll
                        for (int v = 1; v < RKN; ++v) r = u == v ? rk[v] : r;
                        const uint32_t sl = base + (uint32_t)(lane + u * WAVE);
                        const unsigned long long k = c.hkey[sl];
                        const unsigned long long tw = tie_of<SEEDED>((uint32_t)k, (uint32_t)(k >> 32), (int)hidx[sl], c.seed, ord);
                        if (r == grank) gt = tw > gt ? tw : gt;
                        lw = max(lw, offer(r, tw, fl, pass != 0));
                    }
                }
                for (int o = lane + RKN * WAVE; o < gs; o += WAVE) {
                    const uint32_t r2 = c.hrank[base + o];
                    if (r2 >= thr) {
                        const unsigned long long k2 = c.hkey[base + o];
                        const unsigned long long tw = tie_of<SEEDED>((uint32_t)k2, (uint32_t)(k2 >> 32), (int)hidx[base + o], c.seed, ord);
                        if (r2 == grank) gt = tw > gt ? tw : gt;
                        lw = max(lw, offer(r2, tw, fl, pass != 0));
                    }
                }
                if (lw > fl) atomicMax(&q_floor, lw);
            }
            if (dirty) {  // the group's bound and tie word, exact again
                gt = wave_max_u64(gt);
                if (lane == 0) {
                    const unsigned long long nbw = grank ? bound_word(grank, gt) : 0ull;
                    DA_GLOBAL da_i4 *wp = reinterpret_cast<DA_GLOBAL da_i4 *>(&c.grec[grp]);  // {bound, glow = 0} | {tie word, flag = 0}: two 16-byte stores
                    wp[0] = da_i4{(int)(uint32_t)nbw, (int)(uint32_t)(nbw >> 32), 0, 0};
                    wp[1] = da_i4{(int)(uint32_t)gt, (int)(uint32_t)(gt >> 32), 0, 0};
                }
            }
            ++rescans;
#ifdef DA_PHASE_TIMERS
            q_stale += dirty && grank < thr0;
            q_touch += !dirty;
#endif
        };
        // ---- round 0: every wave reads its highest group that is dirty (bound possibly stale) or whose best entry is excluded, if that
        // bound reaches the floor of the clean groups.  The floor rises to (nearly) the answer.
        {
            const unsigned long long fl = __hip_atomic_load(&q_floor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const unsigned long long wtop = wave_max_u64(top);
            if (wtop != 0 && wtop >= fl) {
                const int owner = __ffsll((long long)__ballot(top == wtop)) - 1;
                const int own_u = __builtin_amdgcn_readlane(top_u, owner);
                const bool own_dirty = (((uint32_t)__builtin_amdgcn_readlane((int)dmask, owner) >> own_u) & 1u) != 0;
                read_group((uint32_t)(wid * GPW + owner + own_u * WAVE), own_dirty, wtop, fl);
                if (lane == owner) q_ub[own_u][tid] = 0;
            } else {  // nothing of its own to read: one of the groups with a stale bound, if there are any (A/B of round 6: profiles/r06_ab_engine.txt)
                unsigned int k = 0;
                if (lane == 0) k = atomicAdd(&q_stake, 1u);
                k = (unsigned int)__builtin_amdgcn_readfirstlane((int)k);
                if (k < q_sn) {
                    const uint32_t at = q_sl[k];
                    const int u = (int)(at / SEL2_THREADS), t = (int)(at % SEL2_THREADS);
                    read_group((uint32_t)((t / WAVE) * GPW + (t % WAVE) + u * WAVE), true, 0ull, fl);
                }
            }
        }
        __syncthreads();
        // ---- the groups that still reach the floor, from all waves into one work list, dealt out evenly: a wave that owns several of them
        // no longer reads them one after the other while the others idle (the launch lasts as long as its slowest wave)
        {
            const unsigned long long fl = __hip_atomic_load(&q_floor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
            for (int u = 0; u < GPL; ++u) {
                const unsigned long long v = q_ub[u][tid];
                if (v != 0 && v >= fl && !(rmask >> u & 1u)) q_work[atomicAdd(&q_wn, 1u)] = (uint32_t)(u * SEL2_THREADS + tid) | (((dmask >> u) & 1u) << 31);
            }
        }
        __syncthreads();
        {
            const unsigned int wn = q_wn;
#ifdef DA_PHASE_TIMERS
            if (tid == 0) {
                if (wn > 32) g->st_qdiag[5] += 1;
                if (wn > g->st_qdiag[6]) g->st_qdiag[6] = wn;
                if (pass == 0) g->st_qdiag[7] += 1;
                g->st_qdiag[8] += wn;
            }
#endif
            // the work list, then the stale groups round 0 left: those ride in the rounds the work list needs anyway (waves that would idle), beyond
            // that only the ones whose bound reaches the floor are read now
            const unsigned int sn = q_sn, taken = min(q_stake, sn), rounds = max((wn + NW - 1) / NW, min((unsigned int)DA_AB_REPAIR_ROUNDS, (sn - taken) / 48u));  // (a long backlog -- the first steps of a chain -- may get rounds of its own)
            for (unsigned int i = (unsigned int)wid; i < wn + (sn - taken); i += NW) {  // (wave-uniform)
                const bool listed = i < wn;
                const uint32_t info = listed ? q_work[i] : q_sl[taken + (i - wn)], at = info & 0x7FFFFFFFu;
                const int u = (int)(at / SEL2_THREADS), t = (int)(at % SEL2_THREADS);
                const unsigned long long bound = q_ub[u][t];
                const unsigned long long fl = __hip_atomic_load(&q_floor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (bound < fl && (listed || i / NW >= rounds)) continue;  // the floor has risen past it meanwhile / a stale group that can wait
                read_group((uint32_t)((t / WAVE) * GPW + (t % WAVE) + u * WAVE), !listed || (info >> 31) != 0, bound, fl);
#ifdef DA_PHASE_TIMERS
                if (pass) ++q_rounds;
#endif
            }
        }
        // the wave's best entry outside the excluded rows (highest rank, then highest tie word among its holders)
        const uint32_t wnr = wave_max_u32(nr);
        const unsigned long long wnt = wave_max_u64(nr == wnr ? nt : 0ull);
        // every wave fetches list references and records of ITS candidate's rows now (in flight across the reduction)
        uint32_t cA = 0u, cB = 0u;
        if constexpr (SEEDED) {
            if (wnr) tie_rows<SEEDED>(wnt, c.seed, ord, cA, cB);
        } else {
            cA = wnr ? (uint32_t)((wnt >> 7) & 0xFFFFFFu) : 0u, cB = wnr ? (uint32_t)(wnt >> 31) : 0u;
        }
        const RowInfo cand_ra = load_row(c.rows, cA), cand_rb = load_row(c.rows, cB);
        const da_u2 cand_refA = rowoff[cA], cand_refB = rowoff[cB];
        if (lane == 0) {
            q_red_rank[wid] = wnr;
            q_red_tie[wid] = wnt;
        }
        __syncthreads();
        uint32_t best_rank;
        unsigned long long best_tie;
        {
            const uint32_t r = lane < NW ? q_red_rank[lane] : 0u;
            const unsigned long long t = lane < NW ? q_red_tie[lane] : 0ull;
            best_rank = wave_max_u32(r);
            best_tie = wave_max_u64(r == best_rank ? t : 0ull);
        }
        const bool mine = best_rank != 0 && wnr == best_rank && wnt == best_tie;  // exactly one wave holds the winner (tie words are unique)
        if (pass == 0) {
            Q_TIMER_MARK(2)
            // (the substitution block of this launch finds the same pick by itself -- table_argmax_block: the two blocks never wait for each other)
            if (best_rank == 0) {
                if (tid == 0) {
                    g->spec[par].word = 0;
                    g->l_n[par] = 0;
                }
                if (lane == 0 && rescans) atomicAdd(&g->st_rescans, (unsigned long long)rescans);
                return;  // the table holds nothing selectable: the chain ends
            }
            tie_rows<SEEDED>(best_tie, c.seed, ord, exA, exB);
            __threadfence();  // the bounds this pass tightened are re-read by the next one: stores complete, this CU's L1 dropped
            __syncthreads();
        } else {
            // R for the next step, and with it the entries of the pick's rows that reach it (all scans ended before the barrier above: q_Ln is final)
            const unsigned long long r0 = best_rank ? bound_word(best_rank, best_tie) : 0ull;
            const unsigned int met = q_Ln;
            if (best_rank != 0 && met != 0 && met <= (unsigned int)QL_CAP) {  // (block-uniform)
                if (tid < (int)met) {
                    const CandEntry e = q_L[tid];
                    if (bound_word((uint32_t)e.rank, e.tie) >= r0) {
                        const unsigned int at = atomicAdd(&q_Lout, 1u);
                        if (at < (unsigned int)TOUCH_CAP) {
                            ll_out[at].rank = e.rank;
                            ll_out[at].tie = e.tie;
                        }
                    }
                }
                __syncthreads();
            }
            const unsigned int kept = q_Lout;
            const bool usable = best_rank != 0 && met <= (unsigned int)QL_CAP && kept <= (unsigned int)TOUCH_CAP;
            if (best_rank == 0) {
                if (tid == 0) {
                    g->spec[par].word = 0;
                    g->l_n[par] = 0;
                }
            } else if (mine && lane == 0) {
                SpecPick sp;
                sp.word = usable ? r0 : 0ull;
                sp.tie = best_tie;
                sp.refA = cand_refA;
                sp.refB = cand_refB;
                sp.ra = cand_ra;
                sp.rb = cand_rb;
                g->spec[par] = sp;
                g->l_n[par] = usable ? kept : 0u;
            }
        }
    }
    Q_TIMER_MARK(3)
    if (lane == 0 && rescans) atomicAdd(&g->st_rescans, (unsigned long long)rescans);
    if (tid == 0) {
#ifdef DA_PHASE_TIMERS
        if (DA_TIMED_STEP(step)) {
            g->st_qphase[0] += (unsigned long long)(qp[1] - qp[0]);
            if (!fast) g->st_qphase[1] += (unsigned long long)(qp[2] - qp[1]);
            g->st_qphase[2] += (unsigned long long)(qp[3] - (fast ? qp[1] : qp[2]));
            g->st_qphase[3] += 1;
        }
#endif
    }
#ifdef DA_PHASE_TIMERS
    if (lane == 0) {  // per wave: re-reads that found the bound stale and below the floor / of clean groups for an excluded best entry; the longest wave's rounds
        atomicAdd(&g->st_qdiag[0], (unsigned long long)q_stale);
        atomicAdd(&g->st_qdiag[1], (unsigned long long)q_touch);
        atomicMax(&g->st_qdiag[2 + (step & 1)], (unsigned long long)q_rounds);  // (max over the waves of this step; folded by the next-but-one step below)
    }
    if (tid == 0) {
        g->st_qdiag[4] += g->st_qdiag[2 + ((step + 1) & 1)];
        g->st_qdiag[2 + ((step + 1) & 1)] = 0;
    }
#endif
}

// pick_body: the substitution block of a step (see above): substitution of the pick in the
// lists of rows A and B, exact recount of the six pairs among {A, B, new} (their counts go to sp_cnt: the blocks are written by
// k_iter_update), partner rows -- behind a pick that is either read from the descriptor (known one step ahead) or found by the block itself
// (table_argmax_block).  SHARDED (cmvm_shard.h): the chain holds a slice of the columns and a replica of the pair table -- the six count vectors are
// PARTIAL and go to the head of the exchange slab, and the block leaves one flag per row that shares a substituted column instead of a partner list.
// MANYCOL: the carve for chains of up to 4095 columns, chosen by the host when the regular one does not fit beside the kernel's static arrays
// (sel2_manycol, hip_chain_setup.h): 10 bytes per column instead of 36 in the wide layout.  B's list is not copied to LDS -- pass 1 reads and rewrites
// the entry of a column where it lies in memory (every column is in A's list at most once, so no two threads touch the same entry; the barriers
// that end the chunks of pass 1 order it before pass 2, which reads the entries back) --, the per-column arrays that hold values of at most n_out
// are 16-bit, and the list length of a matched column is read from `collen` at the hit (it grows only after pass 1).
// Returns 1 when the chain is (or just became) finished.
template <class Cell, bool SHARDED = false, bool MANYCOL = false, bool SEEDED = false> __device__ __forceinline__ int pick_body(ChainDev *g, unsigned int *n_done, int step) {
    static_assert(!(SHARDED && SEEDED), "column-sharded chains keep the reference's tie order");
    using O = CellOps<Cell>;
    using F = RowFmt<Cell>;
    using Entry = typename F::Entry;
    const int par = step & 1, iter = step;
    // ---- ONE scalar round trip: every descriptor field the block needs, the entry left by the previous step's search included
    int was_done = g->done, had_error = g->error, lcap = g->lcap, claim_words = g->claim_words;
    int n_rows0 = g->n_rows, rcap = g->rcap, cbw = g->cb_words, adder_size = g->adder_size, carry_size = g->carry_size;
    uint32_t offN = g->rl_used, rl_cap = g->rl_cap, n_live0 = g->n_live, live_peak0 = g->live_peak;
    const uint32_t *step_mant = g->step_mant;
    const float *step_tab = g->step_tab;
    int n_step_mant = g->n_step_mant;
    unsigned long long sp_word = g->spec[par ^ 1].word, sp_tie = g->spec[par ^ 1].tie;
    unsigned int cn_prev = g->c_n[par ^ 1];
    const DA_GLOBAL CandEntry *cl_prev = (const DA_GLOBAL CandEntry *)&g->c_list[par ^ 1][0];
    uint32_t sp_ax = g->spec[par ^ 1].refA.x, sp_ay = g->spec[par ^ 1].refA.y, sp_bx = g->spec[par ^ 1].refB.x, sp_by = g->spec[par ^ 1].refB.y;
    float sp_ra0 = g->spec[par ^ 1].ra.lo, sp_ra1 = g->spec[par ^ 1].ra.hi, sp_ra2 = g->spec[par ^ 1].ra.step, sp_ra3 = g->spec[par ^ 1].ra.lat;
    float sp_rb0 = g->spec[par ^ 1].rb.lo, sp_rb1 = g->spec[par ^ 1].rb.hi, sp_rb2 = g->spec[par ^ 1].rb.step, sp_rb3 = g->spec[par ^ 1].rb.lat;
    Ctx c = make_ctx_raw<SEEDED>(g, 2 * iter);
    uint32_t ord = 0;  // the chain's seeded tie order (SEEDED instantiations)
    if constexpr (SEEDED) ord = g->tie_order;
    DA_GLOBAL int *collen = (DA_GLOBAL int *)g->collen;
    DA_GLOBAL da_u2 *rowoff = (DA_GLOBAL da_u2 *)g->rowoff;
    DA_GLOBAL Entry *rl = (DA_GLOBAL Entry *)g->rlist;
    DA_GLOBAL Cell *mA = (DA_GLOBAL Cell *)g->mA, *mB = (DA_GLOBAL Cell *)g->mB;
    DA_GLOBAL int *mcol = (DA_GLOBAL int *)g->mcol;
    DA_GLOBAL unsigned long long *collist = (DA_GLOBAL unsigned long long *)g->collist;
    DA_GLOBAL uint16_t *cmap = (DA_GLOBAL uint16_t *)g->cmap;
    DA_GLOBAL uint32_t *colbits = (DA_GLOBAL uint32_t *)g->colbits;
    DA_GLOBAL uint32_t *pl_ids = (DA_GLOBAL uint32_t *)g->pl_ids;
    DA_GLOBAL unsigned long long *plist = (DA_GLOBAL unsigned long long *)g->plist;
    DA_GLOBAL da_i4 *picks = (DA_GLOBAL da_i4 *)g->picks;
    DA_GLOBAL uint32_t *sp_cnt = (DA_GLOBAL uint32_t *)g->sp_cnt;
    DA_GLOBAL int32_t *cs_slab = (DA_GLOBAL int32_t *)g->cs_slab, *cs_flags = (DA_GLOBAL int32_t *)g->cs_flags;  // (column-sharded chains only)
    pin_sgpr(was_done, had_error, lcap, claim_words, n_rows0, rcap, cbw, adder_size, carry_size, offN, rl_cap, n_live0, live_peak0, step_mant, step_tab, n_step_mant);
    pin_sgpr(sp_word, sp_tie, cn_prev, cl_prev, sp_ax, sp_ay, sp_bx, sp_by, sp_ra0, sp_ra1, sp_ra2, sp_ra3, sp_rb0, sp_rb1, sp_rb2, sp_rb3);
    pin_sgpr(c.n_out, c.n_bits, c.K, c.Kpad, c.rows);
    pin_sgpr(collen, rowoff, rl, mA, mB, mcol, collist, cmap, colbits, pl_ids, plist, picks, sp_cnt);
    if constexpr (SHARDED) pin_sgpr(cs_slab, cs_flags);
    if constexpr (SEEDED) pin_sgpr(c.seed, ord);
    const int n_out = c.n_out, Kpad = c.Kpad, nb = c.n_bits;
    // column-sharded chain (cmvm_shard.h): a rank whose chain stops (finished, or an error) still hands out the flag buffer of the step -- zero
    // flags and the status trailer {1, capacity error?, other error?} -- written here, on the device: the host does not read the descriptor
    // back between the steps
    auto shard_stop = [&](int err) {
        if constexpr (SHARDED) {
            const int fw = (n_rows0 + 3) / 4;  // rows before this step
            for (int w = threadIdx.x; w < fw; w += SEL2_THREADS) cs_flags[w] = 0;
            if (threadIdx.x == 0) {
                const bool cap = err == E_ROW_CAPACITY || err == E_TABLE_CAPACITY || err == E_LIST_CAPACITY;
                cs_flags[fw] = 1;
                cs_flags[fw + 1] = cap ? 1 : 0;
                cs_flags[fw + 2] = err != E_OK && !cap ? 1 : 0;
            }
        }
    };
    if (was_done) {
        shard_stop(had_error);
        return 1;
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // dynamic LDS carve: B's list | special-pair counters | per-matched-column scratch | column -> position in B
    using Idx = std::conditional_t<MANYCOL, uint16_t, int>;                          // a column, or 1 + a position among at most n_out (< 4096)
    Entry *s_bent = reinterpret_cast<Entry *>(smem);                                  // [n_out] entries of row B (updated in place)
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_bent + n_out);                  // [6][Kpad]
    int *s_len = reinterpret_cast<int *>(s_cnt + 6 * Kpad);                           // [n_out + 1] list lengths of the matched columns
    Idx *s_col = reinterpret_cast<Idx *>(s_len + n_out + 1);                          // [n_out] matched columns
    Idx *s_bpos = s_col + n_out;                                                      // [n_out] 1 + position of a column in B's list, 0 = absent
    int *s_clen = reinterpret_cast<int *>(s_bpos + n_out);                            // [n_out] list length of every column
    Idx *s_cm = reinterpret_cast<Idx *>(s_clen + n_out);                              // [n_out] 1 + index among the matched columns, 0 = not matched
    uint32_t *s_or = reinterpret_cast<uint32_t *>(s_cm + n_out);                      // [claim_words] OR of the substituted columns' row bitmaps (if it fits)
    if constexpr (MANYCOL) {  // special-pair counters | matched lengths | claim area | three 16-bit per-column arrays; no copy of B's list, no lengths of all columns
        s_bent = nullptr;
        s_clen = nullptr;
        s_cnt = reinterpret_cast<uint32_t *>(smem);
        s_len = reinterpret_cast<int *>(s_cnt + 6 * Kpad);
        s_or = reinterpret_cast<uint32_t *>(s_len + n_out + 1);
        s_col = reinterpret_cast<Idx *>(s_or + claim_words);
        s_bpos = s_col + n_out;
        s_cm = s_bpos + n_out;
    }
    constexpr int NW = SEL2_THREADS / WAVE;
    __shared__ int s_np, s_part[NW];
    __shared__ unsigned int s_matches;
    __shared__ RowInfo s_new;
    __shared__ unsigned long long s_am_tie[NW];  // table_argmax_block (a step whose pick was not known ahead)
    __shared__ uint32_t s_am_rank[NW];
    constexpr int IDS_LDS = DA_IDS_LDS;
    __shared__ uint32_t s_ids[IDS_LDS];  // the first partner row ids of the step (the rest, if any, goes through pl_ids in HBM)
    __shared__ Log2Table s_log2;  // copy of c_log2 (the latency model's look-up then stays off the memory path)

    const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();

    SEL_TIMER_DECL
    SEL_TIMER_MARK(0)
    if (had_error != E_OK) {  // a capacity error poisons the chain: stop it (the host retries with a larger arena)
        if (tid == 0) {
            g->done = 1;
            g->n_partners = 0;
            atomicAdd(n_done, 1u);
        }
        shard_stop(had_error);
        return 1;
    }
    // ---------------- (1) the pick: the best of what the previous step left (its untouched entry against the entries its update listed), or --
    // when it left nothing usable -- awaited from the search block of this launch
    unsigned long long best_tie;
    bool from_spec;
    const bool fast = resolve_pick(cl_prev, sp_word, sp_tie, cn_prev, best_tie, from_spec);
    uint32_t A, B;
    tie_rows<SEEDED>(best_tie, c.seed, ord, A, B);
    da_u2 refA = da_u2{sp_ax, sp_ay}, refB = da_u2{sp_bx, sp_by};
    RowInfo ra = RowInfo{sp_ra0, sp_ra1, sp_ra2, sp_ra3}, rb = RowInfo{sp_rb0, sp_rb1, sp_rb2, sp_rb3};
    if (fast && !from_spec) {  // (block-uniform) a listed entry won: its rows' list references and records (one round trip, broadcast loads)
        refA = rowoff[A];
        refB = rowoff[B];
        ra = load_row(c.rows, A);
        rb = load_row(c.rows, B);
    }
    {
        // the list lengths of all columns (needed for the matched columns only, after the substitution) and the latency model's table
        int clen0 = 0;
        if constexpr (!MANYCOL) clen0 = collen[tid < n_out ? tid : 0];
        const bool want_log2 = (adder_size >= 0 || carry_size >= 0) && tid < (int)(sizeof(Log2Table) / 4);
        const uint32_t l2w = want_log2 ? reinterpret_cast<const uint32_t *>(&c_log2)[tid] : 0u;
        if (tid == 0) {
            s_np = 0;
            s_matches = 0;
            g->c_n[par] = 0;  // this step's update appends to c_list[par] (last read by the selection of step - 1)
        }
        if (tid < n_out) {
            if constexpr (!MANYCOL) s_clen[tid] = clen0;
            s_cm[tid] = 0;
            s_bpos[tid] = 0;
        }
        if (want_log2) reinterpret_cast<uint32_t *>(&s_log2)[tid] = l2w;
        for (int w = tid; w < claim_words; w += SEL2_THREADS) s_or[w] = 0;
        for (int j = tid + SEL2_THREADS; j < n_out; j += SEL2_THREADS) {
            if constexpr (!MANYCOL) s_clen[j] = collen[j];
            s_cm[j] = 0;
            s_bpos[j] = 0;
        }
    }
    SEL_TIMER_MARK(1)
    unsigned long long pk_word = 1;
    if (!fast) {
        // (block-uniform, rare: the first step of a chain, an overflowed list) no pick known ahead: the arg-max of the table by this block itself, a
        // plain pass over the rank array -- nothing is written, no bound is read, and nothing is awaited from the search block of this launch, which
        // finds the same entry through the bounds for its own purpose (HIP promises nothing about the order in which workgroups are dispatched)
        uint32_t r0;
        table_argmax_block<SEEDED>(g, c.seed, ord, r0, best_tie, s_am_rank, s_am_tie);
        pk_word = r0 ? bound_word(r0, best_tie) : 0ull;
        tie_rows<SEEDED>(best_tie, c.seed, ord, A, B);
        if (pk_word) {
            refA = rowoff[A];
            refB = rowoff[B];
            ra = load_row(c.rows, A);
            rb = load_row(c.rows, B);
        }
    }
    __syncthreads();
    SEL_TIMER_MARK(2)
    const uint32_t Nw = (uint32_t)n_rows0;
    if (pk_word == 0 || (int)Nw >= rcap) {
        if (tid == 0) {
            if (pk_word != 0) g->error = E_ROW_CAPACITY;
            g->done = 1;
            g->n_partners = 0;
            atomicAdd(n_done, 1u);
        }
        shard_stop(pk_word != 0 ? E_ROW_CAPACITY : E_OK);
        return 1;
    }
    const int idx = (int)blk_pos<SEEDED>((uint32_t)(best_tie & 0x7F), c.seed);
    int shift, sub;
    key_decode(idx, nb, shift, sub);
    const bool same = A == B;

    // ---------------- (2) new row record + substitution (as select_body)
    const int lenA = (int)refA.y, lenB = (int)refB.y;
    if (offN + (uint32_t)lenA > rl_cap) {  // the new row has at most lenA entries (cannot happen with the exact bound; guarded)
        if (tid == 0) {
            g->error = E_LIST_CAPACITY;
            g->done = 1;
            g->n_partners = 0;
            atomicAdd(n_done, 1u);
        }
        shard_stop(E_LIST_CAPACITY);
        return 1;
    }
    DA_GLOBAL Entry *rlA = rl + refA.x, *rlB = rl + refB.x, *rlN = rl + offN;
    Entry eA0 = rl[tid < lenA ? refA.x + (uint32_t)tid : 0u], eB0 = rl[tid < lenB ? refB.x + (uint32_t)tid : 0u];
    load_fence();
    RowInfo rn = RowInfo{0.0f, 0.0f, 0.0f, 0.0f};
    int derr = 0;
    if (tid == 0) {  // arithmetic only, while the entries are in flight; the global stores follow once they have been consumed
        qint_add_pair(ra, rb, shift, sub, rn.lo, rn.hi, rn.step);
        float dlat = adder_dlat(ra, rb, shift, sub, adder_size, carry_size, s_log2, StepLog2{n_step_mant, step_mant, step_tab}, derr);
        rn.lat = (ra.lat < rb.lat ? rb.lat : ra.lat) + dlat;
        s_new = rn;
    }
    for (int k = tid; k < 6 * Kpad; k += SEL2_THREADS) s_cnt[k] = 0;
    if (tid >= lenA) eA0 = F::none();
    if (same || tid >= lenB) eB0 = F::none();
    pin_vgpr(eA0, eB0);  // both consumed (waited for) here, in front of thread 0's stores below
    if (!same) {  // B's list into LDS, addressable by column (s_bpos was zeroed in the prologue, a barrier ago)
        if (tid < lenB) {
            if constexpr (!MANYCOL) s_bent[tid] = eB0;
            s_bpos[F::col(eB0)] = (Idx)(tid + 1);
        }
        for (int t = tid + SEL2_THREADS; t < lenB; t += SEL2_THREADS) {
            const Entry e = rlB[t];
            if constexpr (!MANYCOL) s_bent[t] = e;
            s_bpos[F::col(e)] = (Idx)(t + 1);
        }
    }
    if (tid == 0) {  // (a wait for a loaded value also waits for every store issued before it: these come after the last one)
        if (derr) g->error = E_FLOAT_DOMAIN;
        store_row((DA_GLOBAL RowInfo *)c.rows, Nw, rn);
        picks[iter] = da_i4{(int)A, (int)B, sub, shift};
        if (n_live0 > live_peak0) g->live_peak = n_live0;
    }
    __syncthreads();
    SEL_TIMER_MARK(3)
    uint32_t *cAA = s_cnt, *cAB = s_cnt + Kpad, *cBB = s_cnt + 2 * Kpad, *cAN = s_cnt + 3 * Kpad, *cBN = s_cnt + 4 * Kpad,
             *cNN = s_cnt + 5 * Kpad;
    unsigned int my_matches = 0;
    int m = 0;  // matched columns so far (block-uniform)
    // pass 1: one thread per entry of A (ascending columns); the matched columns are compacted in column order, which
    // is the order of the new row's list
    for (int t0 = 0; t0 < lenA; t0 += SEL2_THREADS) {
        const int t = t0 + tid;
        Cell a = 0, b = 0, ma = 0, mb = 0, na = 0, nbv = 0;
        uint32_t colA = 0;
        int pos = 0;
        if (t < lenA) {
            const Entry e = t0 == 0 ? eA0 : rlA[t];
            colA = F::col(e);
            a = F::cell(e);
            if (same)
                b = a;
            else {
                pos = s_bpos[colA];
                if constexpr (MANYCOL)
                    b = pos ? F::cell(rlB[pos - 1]) : (Cell)0;
                else
                    b = pos ? F::cell(s_bent[pos - 1]) : (Cell)0;
            }
            if (a && b) substitute_column<Cell>(a, b, same, shift, sub, ma, mb);
            na = same ? (Cell)(a & ~ma & ~mb) : (Cell)(a & ~ma);
            nbv = b & ~mb;
        }
        const bool hit = ma != 0;
        const unsigned long long bal = __ballot(hit);
        if (lane == 0) s_part[wid] = __popcll(bal);
        __syncthreads();
        int wbase = 0, chunk = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int v = s_part[w];
            wbase += w < wid ? v : 0;
            chunk += v;
        }
        if (hit) {
            const int at = m + wbase + __popcll(bal & ((1ull << lane) - 1));
            rlA[t] = F::pack(colA, na);
            if constexpr (MANYCOL) {
                if (!same) rlB[pos - 1] = F::pack(colA, nbv);
            } else {
                if (!same) s_bent[pos - 1] = F::pack(colA, nbv);
            }
            rlN[at] = F::pack(colA, ma);
            mcol[at] = (int)colA;
            mA[at] = ma;
            mB[at] = mb;
            s_cm[colA] = (Idx)(at + 1);
            {  // row bitmaps of this column: the new row enters, a row whose cell just lost its last digit leaves
                DA_GLOBAL uint32_t *cb = colbits + (size_t)colA * cbw;
                atomicOr(gen(&cb[Nw >> 5]), 1u << (Nw & 31));
                if (na == 0) atomicAnd(gen(&cb[A >> 5]), ~(1u << (A & 31)));
                if (!same && nbv == 0) atomicAnd(gen(&cb[B >> 5]), ~(1u << (B & 31)));
            }
            if constexpr (MANYCOL)
                s_len[at] = collen[colA];
            else
                s_len[at] = s_clen[colA];  // the pre-append length: the new row itself is not a partner
            s_col[at] = (Idx)colA;
            my_matches += popc32(O::plus(ma) | O::minus(ma));
        }
        // ---------------- (3) exact recount of the pairs among {A, B, new} (their old blocks are replaced); the
        // self pairs of B are counted in pass 2 (B may have columns A does not have)
        if (na) for_pairs_self<Cell>(na, nb, [&](int k) { atomicAdd(&cAA[k], 1u); });
        if (!same) {
            if (na && nbv) for_pairs_cross<Cell>(na, nbv, nb, [&](int k) { atomicAdd(&cAB[k], 1u); });
            if (nbv && ma) for_pairs_cross<Cell>(nbv, ma, nb, [&](int k) { atomicAdd(&cBN[k], 1u); });
        }
        if (na && ma) for_pairs_cross<Cell>(na, ma, nb, [&](int k) { atomicAdd(&cAN[k], 1u); });
        if (ma) for_pairs_self<Cell>(ma, nb, [&](int k) { atomicAdd(&cNN[k], 1u); });
        m += chunk;
        __syncthreads();  // s_part is reused by the next chunk; s_bent updates visible to pass 2
    }
    if (my_matches) atomicAdd(&s_matches, my_matches);  // LDS; added to the chain's statistics by thread 0 at the end
    // pass 2: B's list back to memory, self pairs of what is left of B
    if (!same)
        for (int t = tid; t < lenB; t += SEL2_THREADS) {
            Entry e;
            if constexpr (MANYCOL)
                e = rlB[t];  // (rewritten where it lies by pass 1)
            else {
                e = s_bent[t];
                rlB[t] = e;
            }
            const Cell nbv = F::cell(e);
            if (nbv) for_pairs_self<Cell>(nbv, nb, [&](int k) { atomicAdd(&cBB[k], 1u); });
        }
    // the map column -> matched index for the update blocks (one coalesced copy; pass 1 has completed: its last barrier)
    for (int j = tid; j < n_out; j += SEL2_THREADS) cmap[j] = (uint16_t)s_cm[j];
    // the new row joins the lists of its columns
    {
        const unsigned long long refN = ref_pack(Nw, (uint32_t)m, offN);
        for (int k = tid; k < m; k += SEL2_THREADS) {
            const int j = s_col[k], len = s_len[k];
            if (len < lcap) {
                collist[(size_t)j * lcap + len] = refN;
                collen[j] = len + 1;
            } else
                g->error = E_LIST_CAPACITY;
        }
    }
    __syncthreads();
    SEL_TIMER_MARK(4)
    SEL_TIMER_MARK(5)
    // the exact counts of the six pairs among {A, B, new}: to the special-pair block of k_iter_update (all counters are final: the barrier above)
    if constexpr (SHARDED) {  // PARTIAL counts (this rank's columns): the head of the exchange slab, [6][K]; pairs with B do not exist when the pick is a row with itself
        for (int k = tid; k < 6 * c.K; k += SEL2_THREADS) {
            const int sp = k / c.K;
            cs_slab[k] = (same && (sp == 1 || sp == 2 || sp == 4)) ? 0 : (int32_t)s_cnt[sp * Kpad + (k - sp * c.K)];
        }
    } else
        for (int k = tid; k < 6 * Kpad; k += SEL2_THREADS) sp_cnt[k] = s_cnt[k];
    // ---------------- (4) partner rows -- the rows that have digits in a substituted column -- into the partner list:
    // OR of those columns' row bitmaps (A, B and the new row masked out: their bits are being changed by this very kernel).  Word w
    // of the OR covers rows 32 w ..; the set bits are counted (DPP prefix sum), one LDS atomic per wave reserves the places, the
    // row ids stay in LDS; then, one thread per partner, the list reference is attached (a parallel gather from rowoff).
    {
        const DA_GLOBAL uint32_t *cb = colbits;
        const int nwords = (int)((Nw + 31) >> 5), chunks = (nwords + WAVE - 1) / WAVE;
        DA_GLOBAL uint32_t *ids = pl_ids;
        // While the chain is young the bitmaps are a few 64-word chunks long and many columns are substituted (tens): one wave per chunk
        // would OR them one load after the other while the others idle (20 k of the 34 k cycles of an early step, measured).  The waves of
        // a chunk share its columns then and combine their parts in LDS.
        const bool split = chunks * 4 <= NW && m >= 8 && nwords <= claim_words;  // (at least four waves per chunk and two columns each: else the barrier costs more than it saves)
        if (split) {
            const int c = wid % chunks, part = wid / chunks, ways = (NW - c + chunks - 1) / chunks;  // waves c, c + chunks, ... serve chunk c
            const int w = c * WAVE + lane;
            if (w < nwords) {
                uint32_t bits = 0;
                for (int k = part; k < m; k += ways) bits |= cb[(size_t)s_col[k] * cbw + w];
                if (bits) atomicOr(&s_or[w], bits);
            }
            __syncthreads();
        }
        for (int wb = wid * WAVE; wb < nwords; wb += SEL2_THREADS) {  // wave-uniform trip count
            const int w = wb + lane;
            uint32_t bits = 0;
            if (w < nwords) {
                if (split)
                    bits = s_or[w];
                else
                    for (int k = 0; k < m; ++k) bits |= cb[(size_t)s_col[k] * cbw + w];
                if ((int)(A >> 5) == w) bits &= ~(1u << (A & 31));
                if ((int)(B >> 5) == w) bits &= ~(1u << (B & 31));
                if ((int)(Nw >> 5) == w) bits &= ~(1u << (Nw & 31));
            }
            if constexpr (SHARDED) {  // one 8-bit flag field per row (four rows per word: summed over the ranks without carry) instead of a partner list
                const int fw = (int)((Nw + 3) / 4);
                if (w < nwords) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const uint32_t b = (bits >> (4 * q)) & 0xFu;
                        if (8 * w + q < fw) cs_flags[8 * w + q] = (int32_t)((b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21));
                    }
                }
                continue;
            }
            const int cnt = popc32(bits), inc = (int)wave_scan_add_u32((uint32_t)cnt);  // inclusive prefix inside the wave (DPP)
            const int wave_total = __builtin_amdgcn_readlane(inc, WAVE - 1);
            if (wave_total == 0) continue;
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_np, wave_total);
            int at = __builtin_amdgcn_readfirstlane(base) + inc - cnt;
            while (bits) {
                const uint32_t id = (uint32_t)(w << 5) + (uint32_t)ctz32(bits);
                if (at < IDS_LDS)
                    s_ids[at] = id;
                else
                    ids[at] = id;
                ++at;
                bits &= bits - 1;
            }
        }
    }
    SEL_TIMER_MARK(6)
    __syncthreads();
    if constexpr (SHARDED) {
        if (tid < SHARD_TRAILER) cs_flags[(int)((Nw + 3) / 4) + tid] = 0;  // status trailer of a rank that took the step (cmvm_shard.h)
    }
    {  // partner ids -> partner list entries (row id, list length, list offset)
        const int np = s_np;
        const DA_GLOBAL uint32_t *ids = pl_ids;
        for (int t = tid; t < np; t += 2 * SEL2_THREADS) {  // two partners per thread and pass, their look-ups in flight together
            const int t2 = t + SEL2_THREADS;
            const bool has2 = t2 < np;
            const uint32_t r1 = t < IDS_LDS ? s_ids[t] : ids[t];
            const uint32_t r2 = !has2 ? r1 : t2 < IDS_LDS ? s_ids[t2] : ids[t2];
            const da_u2 ro1 = rowoff[r1], ro2 = rowoff[r2];
            load_fence();
            plist[t] = ref_pack(r1, ro1.y, ro1.x);
            if (has2) plist[t2] = ref_pack(r2, ro2.y, ro2.x);
        }
    }
    SEL_TIMER_MARK(7)
    if (tid == 0) {
        SEL_TIMER_FLUSH
        rowoff[Nw] = da_u2{offN, (uint32_t)m};
        g->rl_used = offN + (uint32_t)m;
        g->m = m;
        g->n_partners = s_np;
        // statistics: atomics without a return value (a plain += is load -> add -> store: one more round trip at the very end)
        atomicAdd(&g->st_matches, (unsigned long long)s_matches);
        atomicAdd(&g->st_partners, (unsigned long long)s_np);
        atomicAdd(&g->st_cells, (unsigned long long)s_np * (unsigned)m);
        if (fast) atomicAdd(&g->st_fast, 1ull);
        {
            // algorithmic bytes of this step's substitution block: the list lengths of all columns, the pick (64 B),
            // both row lists read and written back, the row bitmaps of the m substituted columns, per partner its id + list reference +
            // partner-list entry, the hand-off (matched columns, consumed digits, new row's list, column map, column-list and bitmap
            // updates), the six special-pair count vectors.  (The search block's bytes: st_rescans, and 17 B per group, priced by the host.)
            const unsigned long long eb = sizeof(Entry), cb = sizeof(Cell);
            const unsigned long long nwords = (Nw + 31) >> 5;
            atomicAdd(&g->st_sel_bytes, 4ull * (unsigned)n_out + 64ull + 2ull * eb * (unsigned)(lenA + (same ? 0 : lenB)) + 4ull * (unsigned)m * nwords + 20ull * (unsigned)s_np +
                                            (unsigned)m * (4ull + 2ull * cb + eb + 8ull + 12ull) + 2ull * (unsigned)n_out + 6ull * 4ull * (unsigned)Kpad);
        }
        g->A = A;
        g->B = B;
        g->Nw = Nw;
        g->pk_shift = shift;
        g->pk_sub = sub;
        g->n_rows = (int)Nw + 1;
        g->iter = iter + 1;
    }
    return 0;
}
// grid (chains padded to a multiple of 8, 2): the chain index is the fast grid dimension, so that the two blocks of a chain and its
// k_iter_update blocks run on the same XCD (update_body); y = 0 the search block, y = 1 the substitution block.  `step` = the
// number of the lockstep iteration = the `iter` of every chain of the launch that has not finished (kernel argument: the search
// block must not read a field the substitution block writes during the launch).
#ifndef DA_SEL2_WAVES
#define DA_SEL2_WAVES 4  // wavefronts per SIMD the register budget of k_iter_select2 is capped for (measured 4 .. 8: the spills of 5 and more cost more than the smaller footprint gains)
#endif
template <class Cell, bool SHARDED = false, bool MANYCOL = false, bool SEEDED = false> __global__ void __launch_bounds__(SEL2_THREADS) __attribute__((amdgpu_waves_per_eu(DA_SEL2_WAVES, DA_SEL2_WAVES))) k_iter_select2(ChainDev *chains, int n_chains, unsigned int *n_done, int step) {
    if ((int)blockIdx.x >= n_chains) return;
#ifdef DA_STEP_CLOCKS
    {
        ChainDev *g = &chains[blockIdx.x];
        if (threadIdx.x == 0 && !g->done) {
            CLK_MARK(g, step & 1, 0, true);
            if (blockIdx.y == 1 && step > 0) {  // the step before this one is complete: its four marks into the sums
                unsigned long long *k = g->clk[(step - 1) & 1];
                if (k[0] && k[1] && k[2] && k[3] && CLK_TIMED_STEP(step - 1)) {
                    g->st_qdiag[0] += k[1] - ~k[0];
                    g->st_qdiag[1] += ~k[2] - k[1];
                    g->st_qdiag[4] += k[3] - ~k[2];
                    g->st_qdiag[5] += CLK_NOW() - k[3];
                    g->st_qdiag[7] += 1;
                }
                k[0] = k[1] = k[2] = k[3] = 0;
            }
        }
    }
#endif
    if (blockIdx.y == 0)
        search_body<Cell, SEEDED>(&chains[blockIdx.x], step);
    else
        (void)pick_body<Cell, SHARDED, MANYCOL, SEEDED>(&chains[blockIdx.x], n_done, step);
#ifdef DA_STEP_CLOCKS
    __syncthreads();
    if (threadIdx.x == 0) CLK_MARK(&chains[blockIdx.x], step & 1, 1, false);
#endif
}

#ifndef DA_UPD_OCC
#define DA_UPD_OCC 5  // blocks of 256 threads per CU the register budget is capped for.  The cap no longer binds: the narrow instantiations take 63 - 67 VGPRs, the wide
                      // ones 67 - 71, none spills, at 5 and at 6 alike (80 = 512 / 6 at the granule of 8) -- up to seven waves per SIMD are resident
#endif
#if DA_UPD_OCC >= 8
#define DA_UPD_SGPRS 80  // 800 SGPRs per SIMD: more than 80 per wave would cap the residency below 8 waves per SIMD
#elif DA_UPD_OCC == 7
#define DA_UPD_SGPRS 96
#else
#define DA_UPD_SGPRS 102
#endif
constexpr int SLOT_NONE = -1, SLOT_SLOW = -2;  // no such block / to be searched beyond its first bucket

// ------------------------------------------------------------------------------------------------ k_iter_update (quad)
// The greedy loop is bound by VALU issue, not by memory: one wavefront per partner row executed ~260 vector and ~185
// scalar instructions per partner with a handful of lanes doing useful work (PMC: profiles/r02_*).  Here a partner row is
// handled by a 16-LANE GROUP -- one DPP row -- and a wavefront works on FOUR partners at once with one instruction
// stream: a key bucket is 16 slots = one load per lane, a typical row list has <= 16 entries, the K <= 32 counts of a
// block are 16 words = one word (two counts) per lane, and the reductions stay inside the DPP row.  Everything that was
// wave-uniform per partner (slots, keys, hashes) is now a per-lane value, identical across the lanes of a group.
// Rare cases (key not in its first bucket, block creation) fall back to the wave-wide table functions, one group at a time.
#ifndef DA_UPD_QG
#define DA_UPD_QG 16  // lanes per partner row (16: four partners per wavefront; 8: eight -- every wave instruction then serves twice as many partners, but a row list
                      // takes twice the chunks and a bucket two slots per lane: measured (MI355X, round 6, C3 batch / one chain) 32.5 / 24.2 us per step against 30.6 / 20.3)
#endif
constexpr int QG = DA_UPD_QG, QN = WAVE / QG;  // lanes per partner, partners per wavefront
constexpr int QG_LOG2 = QG == 16 ? 4 : 3, SPL = (int)BUCKET / QG, HL = QG / 2;  // key slots of a bucket per lane; lanes per block in the re-evaluation
constexpr uint32_t QMASK = (1u << QG) - 1u, HMASK = (1u << HL) - 1u;
static_assert(QG == 16 || QG == 8, "a partner row is handled by one DPP row or half a row");

__device__ __forceinline__ unsigned long long row_max_u64(unsigned long long v) {  // max over each 16-lane row, valid in lane 15 of the row
    v = dpp_max_u64<DPP_ROW_SHR1, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_SHR2, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_SHR4, 0xF>(v);
    v = dpp_max_u64<DPP_ROW_SHR8, 0xF>(v);
    return v;
}

constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141;  // quad_perm:[1,0,3,2], quad_perm:[2,3,0,1], lane i <-> 7 - i of its eight
template <int LANES> __device__ __forceinline__ unsigned long long part_row_max_u64(unsigned long long v) {  // max over each group of EIGHT / FOUR lanes, in all of them (butterfly steps)
    v = dpp_max_u64<DPP_QUAD_XOR1, 0xF>(v);
    v = dpp_max_u64<DPP_QUAD_XOR2, 0xF>(v);
    if constexpr (LANES == 8) v = dpp_max_u64<DPP_ROW_HALF_MIRROR, 0xF>(v);
    return v;
}

// ---- one update step of a chain, as the wave-uniform values its workers need (scalar registers)
template <class Cell> struct UpdStep {
    Ctx c;
    int done, n_partners, m, n_in;
    uint32_t A, B, Nw;
    int shift, sub;  // of the pick's key
    const DA_GLOBAL int *mcol;
    const DA_GLOBAL Cell *mA, *mB;
    const DA_GLOBAL uint16_t *cmap;
    const DA_GLOBAL typename RowFmt<Cell>::Entry *rl;
    const DA_GLOBAL unsigned long long *plist;
    uint32_t dcw;  // the bits of the chain's latency-penalty weight in the WEIGHTED instantiations, unused (0) in the others
    uint32_t ord;  // the chain's seeded tie order (TIE_ORDER_*) in the SEEDED instantiations, unused (0) in the others
    uint32_t slk;  // the chain's score slack in the SLACK instantiations, unused (0) in the others
};
// ONE round trip: every descriptor field an update worker needs, pinned before the first branch (pin_sgpr)
template <class Cell, bool SEEDED = false, bool WEIGHTED = false, bool SLACK = false> __device__ __forceinline__ UpdStep<Cell> load_upd_step(ChainDev *gq) {
    using Entry = typename RowFmt<Cell>::Entry;
    UpdStep<Cell> u;
    int iter = gq->iter;
    u.done = gq->done, u.n_partners = gq->n_partners, u.m = gq->m, u.n_in = gq->n_in;
    u.A = gq->A, u.B = gq->B, u.Nw = gq->Nw;
    u.shift = gq->pk_shift, u.sub = gq->pk_sub;
    u.c = make_ctx_raw<SEEDED>(gq, 2 * iter - 1);
    if constexpr (WEIGHTED)
        u.dcw = f2u(gq->dc_weight);
    else
        u.dcw = 0;
    if constexpr (SEEDED)
        u.ord = gq->tie_order;
    else
        u.ord = 0;
    if constexpr (SLACK)
        u.slk = gq->slack;
    else
        u.slk = 0;
    // the step being applied is iter - 1 (the selection has counted it): its search left the best entry the step does not touch in
    // spec[(iter - 1) & 1]; the best entry of every block this launch writes that reaches it goes to c_list[(iter - 1) & 1] (fold_entry)
    u.c.rword = gq->spec[(iter - 1) & 1].word;
    u.c.cn = &gq->c_n[(iter - 1) & 1];
    u.c.cl = &gq->c_list[(iter - 1) & 1][0];
    u.mcol = (const DA_GLOBAL int *)gq->mcol;
    u.mA = (const DA_GLOBAL Cell *)gq->mA, u.mB = (const DA_GLOBAL Cell *)gq->mB;
    u.cmap = (const DA_GLOBAL uint16_t *)gq->cmap;
    u.rl = (const DA_GLOBAL Entry *)gq->rlist;
    u.plist = (const DA_GLOBAL unsigned long long *)gq->plist;
    pin_sgpr(u.done, u.n_partners, iter, u.m, u.n_in, u.A, u.B, u.Nw, u.shift, u.sub, u.mcol, u.mA, u.cmap, u.rl, u.plist);
    pin_sgpr(u.c.n_out, u.c.n_bits, u.c.K, u.c.Kpad, u.c.method, u.c.gs_log2, u.c.pb_log2, u.c.cmask, u.c.windows, u.c.hkey, u.c.hrank, u.c.hblk, u.c.grec, u.c.rows);
    pin_sgpr(u.c.rword, u.c.cn, u.c.cl);
    if constexpr (SEEDED) pin_sgpr(u.c.seed, u.ord);
    if constexpr (WEIGHTED) pin_sgpr(u.dcw);
    if constexpr (SLACK) pin_sgpr(u.slk);
    u.c.tomb = KEY_TOMB - (unsigned long long)((2 * iter - 1) & 3);
    ctx_finish(u.c);
    return u;
}
// LDS of an update worker: the hand-off of the selection (consumed digits of A and B [n_out each], the substituted columns
// [n_out], column -> 1 + index of the substituted column [n_out]) -- shared by the waves that copied it together -- and ONE
// wave's per-partner counters [QN][Kpad] at the head of its region (the digit pairs gained with the new row; the losses of A's and B's blocks are read from them, upd_loss)
template <class Cell> struct UpdLds {
    Cell *mA, *mB;
    int *col;
    uint16_t *cmap;
    uint32_t *cnt;
    static __device__ __forceinline__ size_t table_bytes(int n_out) { return (size_t)n_out * (2 * sizeof(Cell) + 4 + 2); }
    // (a wave's region keeps the size it had with three vectors per partner and a spare one: the LDS budget check of the host and the size it reports are
    // unchanged; only the first QN vectors are used.  LDS does not bound the residency: seven blocks of the C3 line take 7 x 10 KB of the CU's 160 KB)
    static __device__ __forceinline__ size_t wave_bytes(int Kpad) { return (size_t)(QN * 3 + 1) * Kpad * 4; }
    __device__ __forceinline__ void carve(unsigned char *tables, unsigned char *counters, int n_out) {
        mA = reinterpret_cast<Cell *>(tables);
        mB = mA + n_out;
        col = reinterpret_cast<int *>(mB + n_out);
        cmap = reinterpret_cast<uint16_t *>(col + n_out);
        cnt = reinterpret_cast<uint32_t *>(counters);
    }
};
// the hand-off of the selection into LDS by `nthr` threads (t = this thread's index among them): one pass; the caller makes
// it visible (block barrier, or lds_fence() when one wave copies for itself)
template <class Cell> __device__ __forceinline__ void copy_handoff(const UpdStep<Cell> &u, const UpdLds<Cell> &s, int t, int nthr) {
    for (int j = t; j < u.c.n_out; j += nthr) s.cmap[j] = u.cmap[j];
    for (int j = t; j < u.m; j += nthr) {
        s.col[j] = u.mcol[j];
        s.mA[j] = u.mA[j];
    }
}

// The counts a block of a partner row loses are a RE-INDEXING of the counts the new row gains (cN, key (d, sg) at index sg W + d + nb - 1,
// W = 2 nb - 1): the walk of update_partners counts every digit pair once, under the new row's key, and the losses are read through the
// inverse map.  Key (d', s') of the block (X, partner) has lost cN[(s' ^ sub) W + sgn d' + cst]; a pre-image outside the W shifts reads 0.
//   * A-role digits (in A's block):  sgn = -1 when the partner lies above A (the key is mirrored), cst = nb - 1, sub = 0;
//   * B-role digits (in B's block, or A's when the pick is a row with itself): they sit `shift` further and their sign is flipped when
//     the pick subtracts -- sgn = -1 when the partner lies above B, cst = nb - 1 - shift, sub = pk_sub.
__device__ __forceinline__ uint32_t upd_loss(const uint32_t *cN, int k, int K, int W, int nbm1, int sgn, int cst, int sub) {
    const int sg = k >= W, t = __mul24(k - (sg ? W : 0) - nbm1, sgn) + cst;
    return (k < K && (unsigned)t < (unsigned)W) ? cN[((sg ^ sub) ? W : 0) + t] : 0u;
}
// What key k of the block (X, partner) loses with the partner's digit pairs counted in cN.  `role_b`: X is B -- the B-role pairs --, else X is A:
// the A-role pairs, and the B-role ones too when the pick is a row with itself (`same`; B has no block of its own then).  `above`: the partner
// lies above X (the key is mirrored).  nb, K: the chain's; shift, sub: the pick's key.
__device__ __forceinline__ uint32_t block_loss(const uint32_t *cN, int k, bool role_b, bool above, bool same, int K, int nb, int shift, int sub) {
    const int W = 2 * nb - 1, sgn = above ? -1 : 1;
    uint32_t v = upd_loss(cN, k, K, W, nb - 1, sgn, role_b ? nb - 1 - shift : nb - 1, role_b ? sub : 0);
    if (same) v += upd_loss(cN, k, K, W, nb - 1, sgn, nb - 1 - shift, sub);
    return v;
}

// update_partners: ONE WAVEFRONT works through the partner rows first + q, first + stride + q, ... < limit of the step (q = its
// four 16-lane groups); no block-level synchronisation inside.  `ref_next` = the (pre-fetched) reference of this group's first
// partner, `rnew` the record of the new row.
// STATS: tally the blocks found / created / deleted (benchmark instrumentation and the "peak pair blocks" statistic, DA4ML_HIP_STATS=1); the ballots, population
// counts and the scalar registers of the three counters are 1.8 % of the batch's step (measured: 27.9 -> 27.5 us, one chain 19.5 -> 19.0), so the product runs without them
template <class Cell, bool STATS, bool SEEDED = false, bool WEIGHTED = false, bool SLACK = false>
__device__ __forceinline__ void update_partners(ChainDev *g, const UpdStep<Cell> &u, const UpdLds<Cell> &s, int first, int stride, int limit, unsigned long long ref_next,
                                                const RowInfo &rnew, unsigned int &found, unsigned int &inserts, unsigned int &deletes) {
    using F = RowFmt<Cell>;
    using Entry = typename F::Entry;
    constexpr int HW = ((sizeof(Cell) == 4 ? 24 : 60) + HL - 1) / HL;  // count words per lane (a block's words over its HL lanes): narrow layout Kpad / 2 <= 24 words, wide <= 60
    const Ctx &c = u.c;
    const BlockEval<SEEDED, WEIGHTED, SLACK> ev{c, u.dcw, u.ord, u.slk};
    const uint32_t A = u.A, B = u.B, Nw = u.Nw;
    const int m = u.m, n_in = u.n_in, pk_shift = u.shift, pk_sub = u.sub;
    const DA_GLOBAL Entry *rl = u.rl;
    const DA_GLOBAL unsigned long long *plist = u.plist;
    Cell *s_mA = s.mA;
    int *s_col = s.col;
    uint16_t *s_cmap = s.cmap;
    uint32_t *s_cnt = s.cnt;
    const int nb = c.n_bits, Kpad = c.Kpad, K = c.K;
    const int lane = lane_id();
    // What a lane derives from its index -- group, place in the group, counter and count-word addresses, a dozen values -- is formed AGAIN in
    // every phase of a pass from a copy of the index the optimiser cannot see through: left alone it computes them once in front of the pass loop
    // and carries them through every pass in registers of their own, which is what kept the kernel above 80 VGPRs (six waves per SIMD).
    auto lane_now = [&]() {
        int v = lane;
        pin_vgpr(v);
        return v;
    };
    const bool same = A == B;
    const int W = 2 * nb - 1;  // key indices per sign
    const int KW = Kpad / 2;  // 32-bit words of counts per block (two u16 counts each)
    UPD_TIMER_DECL
    // partner p of the list: pass p / (QN total_waves), wave (p / QN) mod total_waves, group p mod QN -- all groups of all
    // waves are busy except in the last pass
#ifndef DA_UPD_CH
#define DA_UPD_CH 4  // measured on MI355X (C3 batch 64): 1 -> 52.7, 2 -> 53.8, 4 -> 54.5 solves/s
#endif
    constexpr int CH = DA_UPD_CH;  // list chunks (16 entries each) fetched together; longer lists continue in the loop below
    for (int base = first; base < limit; base += stride) {
        const int ln = lane_now(), q = ln >> QG_LOG2, l = ln & (QG - 1), qsh = q * QG;
        uint32_t *const cN = s_cnt + (size_t)q * Kpad;  // this group's counters
        const int idx = base + q;
        const bool valid = idx < limit;
        // ---- round trip 1: the group's partner reference (the next pass's one is fetched now: off the critical path there)
        const unsigned long long ref = ref_next;
        ref_next = idx + stride < limit ? plist[idx + stride] : 0ull;
        const uint32_t pr = ref_row(ref), off = ref_off(ref);
        const bool dense = valid && (int)pr < n_in;  // dense input row: entry j is column j -- fetch the substituted columns only
        const int cnt = !valid ? 0 : dense ? m : (int)ref_len(ref);
        // ---- round trip 2: the two key buckets (16 slots = one per lane) and the head of the row list
        const uint32_t lA = min(A, pr), hA = max(A, pr), lB = min(B, pr), hB = max(B, pr);
        const unsigned long long keyA = pack_pair(lA, hA), keyB = pack_pair(lB, hB);
        const uint32_t baseA = (hash_pair(lA, hA) & ~(BUCKET - 1)) & c.cmask, baseB = (hash_pair(lB, hB) & ~(BUCKET - 1)) & c.cmask;
        unsigned long long kA[SPL], kB[SPL];  // (16 slots of a bucket over the group's lanes: one or two -- adjacent -- per lane)
#pragma unroll
        for (int t = 0; t < SPL; ++t) {
            kA[t] = valid ? c.hkey[baseA + l * SPL + t] : KEY_TOMB;
            kB[t] = (valid && !same) ? c.hkey[baseB + l * SPL + t] : KEY_TOMB;
        }
        Entry e[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int j = l + u * QG;
            e[u] = j < cnt ? rl[(size_t)off + (dense ? s_col[j] : j)] : F::none();
        }
        for (int k = l; k < Kpad; k += QG) cN[k] = 0;  // while the loads are in flight
        // ---- resolve the probes (per group: 16 bits of the wave ballots)
        int sA = SLOT_NONE, sB = SLOT_NONE;
        {
            // which of a lane's slots holds the key (a key sits in one slot at most), and whether the bucket has an EMPTY slot
            bool emp_a = false, emp_b = false;
            int at_a = -1, at_b = -1;
#pragma unroll
            for (int t = 0; t < SPL; ++t) {
                at_a = kA[t] == keyA ? t : at_a;
                at_b = kB[t] == keyB ? t : at_b;
                emp_a |= kA[t] == KEY_EMPTY;
                emp_b |= kB[t] == KEY_EMPTY;
            }
            const uint32_t hitA = (uint32_t)(__ballot(at_a >= 0) >> qsh) & QMASK, empA = (uint32_t)(__ballot(emp_a) >> qsh) & QMASK;
            const uint32_t hitB = (uint32_t)(__ballot(at_b >= 0) >> qsh) & QMASK, empB = (uint32_t)(__ballot(emp_b) >> qsh) & QMASK;
            // (SPL == 2: the slot inside the hit lane's pair comes from that lane; all lanes take part in the exchange)
            int ta = 0, tb = 0;
            if constexpr (SPL > 1) {
                ta = __shfl(at_a, hitA ? qsh + ctz32(hitA) : lane);
                tb = __shfl(at_b, hitB ? qsh + ctz32(hitB) : lane);
            }
            if (valid) {
                sA = hitA ? (int)(baseA + (uint32_t)(ctz32(hitA) * SPL + ta)) : (empA ? SLOT_NONE : SLOT_SLOW);
                if (!same) sB = hitB ? (int)(baseB + (uint32_t)(ctz32(hitB) * SPL + tb)) : (empB ? SLOT_NONE : SLOT_SLOW);
            }
        }
        UPD_TIMER_MARK(1)  // reference + list + table probes
        // ---- round trip 3: the payload lines of the blocks that exist.  The two blocks of a partner -- (A, r) and (B, r) -- are handled SIDE BY SIDE:
        // the lower half of the group's lanes takes A's block, the upper half B's, so that one pass of the instruction stream below re-evaluates both
        // (round 6: one pass per block was twice the instructions; batch 31.1 -> 30.7 us per step); a lane holds the header of its block (16 bytes)
        // and every HL-th count word
        const int half = l / HL, hl = l % HL;
        const int sX = half ? sB : sA;
        const da_i4 z4 = da_i4{0, 0, 0, 0};
        const da_i4 hdX = sX >= 0 ? *reinterpret_cast<const DA_GLOBAL da_i4 *>(blk_ptr(c, sX)) : z4;
        uint32_t wX[HW];
#pragma unroll
        for (int u = 0; u < HW; ++u) {
            const int j = hl + u * HL;
            wX[u] = (sX >= 0 && j < KW) ? reinterpret_cast<const DA_GLOBAL uint32_t *>(blk_ptr(c, sX) + 16)[j] : 0u;
        }
        lds_fence();  // counters are zero
        // ---- digit pairs lost with A's / B's consumed digits and gained with the new row: a lane per list entry.
        // The digit pairs (partner digit, consumed A-role digit) are walked ONCE and counted ONCE, under the key they gain with the new row,
        // whose cell in this column IS ma (the partner is the row with the smaller id): key (q - p, signs).  What A's and B's blocks lose with
        // the same pairs is that vector re-indexed (upd_loss):
        //   * lost with A: the same key when the partner is also below A, the mirrored one (shift negated) otherwise;
        //   * lost with the B-role digit that went with the A-role one: it sits `shift` positions further, its sign flipped when the pick
        //     subtracts (substitute_column, cmvm_core.h: mb = ma moved by shift, also when A and B are one row) -- in B's block, or in A's
        //     when the pick is a row with itself.
        // The body of the walk is straight-line, the consumed digits (one per column, hardly ever more) are the OUTER loop.
        const int Wk4 = 4 * W;  // (byte offsets into the counters)
        unsigned char *const pN = reinterpret_cast<unsigned char *>(cN + (nb - 1));
        auto bump = [](unsigned char *at) { atomicAdd(reinterpret_cast<uint32_t *>(at), 1u); };
        auto pairs_of = [&](const Entry en) {
            using O = CellOps<Cell>;
            const Cell x = F::cell(en);
            const int at = x ? (int)s_cmap[F::col(en)] : 0;
            if (!at) return;  // empty cell, or a column that was not substituted
            const Cell ma = s_mA[at - 1];
            const uint32_t xm = O::minus(x), hm = O::minus(ma), la0 = O::plus(x) | xm;
            uint32_t h = O::plus(ma) | hm;
            while (h) {
                const int q_ = ctz32(h);
                h &= h - 1;
                const uint32_t xq = (hm >> q_) & 1u ? ~xm : xm;  // bit p: the signs of the two digits differ
                uint32_t la = la0;
                while (la) {
                    const int p_ = ctz32(la);
                    la &= la - 1;
                    int sgm = -(int)((xq >> p_) & 1u);
                    pin_vgpr(sgm);  // (kept as a mask: the compiler otherwise turns the AND below into compare + move + select)
                    const int d = q_ - p_, off = sgm & Wk4;  // key (d, sg) -> index sg (2 nb - 1) + d + nb - 1
                    bump(pN + off + 4 * d);
                }
            }
        };
#pragma unroll
        for (int u = 0; u < CH; ++u)
            if (__any(u * QG < cnt)) pairs_of(e[u]);  // e[u] is empty beyond the list
        for (int j = l + CH * QG; __any(j < cnt); j += QG)
            if (j < cnt) pairs_of(rl[(size_t)off + (dense ? s_col[j] : j)]);
        lds_fence();
        int fnew = 0;  // a block (partner, new row) is created when one of its counts reached 2
        for (int k = l; k < K; k += QG) fnew |= cN[k] >= 2u;
        const bool gnew = valid && (((uint32_t)(__ballot(fnew != 0) >> qsh) & QMASK) != 0);
        UPD_TIMER_MARK(2)  // pair enumeration
        // ---- re-evaluate both blocks at once: two counts per lane and word, reduction inside the eight lanes of a block, their last lane publishes
        {
            const int ln = lane_now(), q = ln >> QG_LOG2, l = ln & (QG - 1), qsh = q * QG, half = l / HL, hl = l % HL;
            const uint32_t *const cN = s_cnt + (size_t)q * Kpad;
            const bool has = sX >= 0;
            const int ov = hdX.x;
            const float dl = __int_as_float(hdX.y);
            // this lane's block loses the A-role pairs (lower half: A's block) or the B-role ones (upper half: B's block) -- and both when
            // the pick is a row with itself (A's block; the upper half then has no block)
            const uint32_t rowX = half ? B : A;
            auto lost = [&](int k) { return block_loss(cN, k, half != 0, rowX < pr, same, K, nb, pk_shift, pk_sub); };
            unsigned long long best = 0;
            int alive = 0;
            const uint32_t pw = ev.pair_word(min(rowX, pr), max(rowX, pr));
#pragma unroll
            for (int u = 0; u < HW; ++u) {
                const int j = hl + u * HL;
                if (has && j < KW) {
                    const uint32_t o0 = wX[u] & 0xFFFFu, o1 = wX[u] >> 16;
                    const uint32_t n0 = o0 - lost(2 * j), n1 = o1 - lost(2 * j + 1);
                    if (n0 != o0 || n1 != o1) reinterpret_cast<DA_GLOBAL uint32_t *>(blk_ptr(c, sX) + 16)[j] = (n0 & 0xFFFFu) | (n1 << 16);
                    alive |= (n0 >= 2u) | (n1 >= 2u);
                    const unsigned long long c0 = ev.candidate(n0, (uint32_t)(2 * j), ov, dl, pw), c1 = ev.candidate(n1, (uint32_t)(2 * j + 1), ov, dl, pw);
                    ev.fold(best, c0);
                    ev.fold(best, c1);
                }
            }
            best = part_row_max_u64<HL>(best);  // all lanes take part (the DPP source lanes must be active); every lane of a block's HL holds its result
            const bool any_alive = (((uint32_t)(__ballot(alive != 0) >> (qsh + HL * half)) & HMASK) != 0);
            if (has && hl == HL - 1) block_commit(ev, sX, pack_pair(min(rowX, pr), max(rowX, pr)), BlkHdr{ov, dl, (uint32_t)hdX.z, (uint32_t)hdX.w}, best, any_alive, false);
            if constexpr (STATS) deletes += (unsigned)__popcll(__ballot(has && hl == HL - 1 && !any_alive));  // (wave-uniform: the blocks this pass deleted, tallied once per workgroup)
        }
        UPD_TIMER_MARK(3)  // block updates
        // ---- block creation, ALL creating groups of the wavefront at once (a group = one new block (partner, new row)): the first bucket of the key
        // is probed by the group's lanes, its first free slot claimed by compare-and-swap (lost to another claimant: the next free one), the counts
        // come from the group's LDS counters two per lane, the best key by a reduction inside the DPP row.  One instruction stream for up to QN
        // creations instead of one wave-wide table_insert after the other: the launch lasts as long as its slowest wave, and in the first thousands
        // of steps that is a wave with four creations in a pass (round 6: batch 30.4 -> 29.5 us per step; steps 0 - 2000: update 35.1 -> 28.7 us).
        // A group whose first bucket has no free slot takes the wave-wide path below.
        bool gslow = false;  // this group's creation is left to table_insert
        if (__ballot(gnew)) {
            const int ln = lane_now(), q = ln >> QG_LOG2, l = ln & (QG - 1), qsh = q * QG;
            const uint32_t *const cN = s_cnt + (size_t)q * Kpad;
            const unsigned long long keyN = pack_pair(pr, Nw);  // (the partner is older than the new row)
            const uint32_t baseN = (hash_pair(pr, Nw) & ~(BUCKET - 1)) & c.cmask;
            unsigned long long kN[SPL];
#pragma unroll
            for (int t = 0; t < SPL; ++t) kN[t] = gnew ? c.hkey[baseN + l * SPL + t] : 0ull;
            const RowInfo rp = load_row(c.rows, gnew ? pr : 0u);
            int pick_t = -1;  // a free slot of this lane: EMPTY, or a tombstone of an earlier launch
#pragma unroll
            for (int t = SPL - 1; t >= 0; --t)
                if (gnew && (kN[t] == KEY_EMPTY || (kN[t] >= KEY_TOMB_LO && kN[t] != c.tomb))) pick_t = t;
            uint32_t av = (uint32_t)(__ballot(pick_t >= 0) >> qsh) & QMASK;
            int nslot = -1;
            bool trying = gnew;
            while (__ballot(trying)) {
                const int cand = av ? ctz32(av) : -1;
                int ok = 0;
                if (trying && l == cand) {
                    const unsigned long long was = pick_t == 0 ? kN[0] : kN[SPL - 1];
                    ok = atomicCAS(gen(&c.hkey[baseN + l * SPL + pick_t]), was, keyN) == was;
                }
                const bool won = (((uint32_t)(__ballot(ok != 0) >> qsh)) & QMASK) != 0;
                int tsel = 0;
                if constexpr (SPL > 1) tsel = __shfl(pick_t, cand >= 0 ? qsh + cand : lane);
                if (trying) {
                    if (cand < 0) {
                        trying = false;
                        gslow = true;
                    } else if (won) {
                        nslot = (int)(baseN + (uint32_t)(cand * SPL + tsel));
                        trying = false;
                    } else
                        av &= av - 1;
                }
            }
            const bool made = nslot >= 0;
            const int ovn = n_overlap(rp, rnew);
            const float dln = fabsf(rp.lat - rnew.lat);
            unsigned long long bestn = 0;
            const uint32_t pwn = ev.pair_word(pr, Nw);  // (the partner is older than the new row)
            constexpr int CWN = ((sizeof(Cell) == 4 ? 24 : 60) + QG - 1) / QG;  // count words per lane
#pragma unroll
            for (int u = 0; u < CWN; ++u) {
                const int j = l + u * QG;
                if (made && j < KW) {
                    const uint32_t n0 = cN[2 * j], n1 = cN[2 * j + 1];  // (zero beyond K: nothing ever counts there)
                    if ((n0 | n1) > 65535u) c.g->error = E_COUNT_OVERFLOW;
                    reinterpret_cast<DA_GLOBAL uint32_t *>(blk_ptr(c, nslot) + 16)[j] = (n0 & 0xFFFFu) | (n1 << 16);
                    const unsigned long long c0 = ev.candidate(n0, (uint32_t)(2 * j), ovn, dln, pwn), c1 = ev.candidate(n1, (uint32_t)(2 * j + 1), ovn, dln, pwn);
                    ev.fold(bestn, c0);
                    ev.fold(bestn, c1);
                }
            }
            bestn = part_row_max_u64<8>(bestn);  // (eight lanes, then the two halves of the group)
            if constexpr (QG == 16) bestn = dpp_max_u64<0x140, 0xF>(bestn);  // row_mirror: lane i <-> 15 - i
            if (made && l == QG - 1) publish_new_block(ev, nslot, pr, Nw, ovn, dln, bestn);
            if constexpr (STATS) inserts += (unsigned)__popcll(__ballot(made && l == 0));
        }
        // ---- rare: blocks beyond their first bucket (look-up, or creation in a full bucket) -- the whole wave, one group at a time
        const unsigned long long rare = __ballot(valid && (sA == SLOT_SLOW || sB == SLOT_SLOW || gslow));
        if constexpr (STATS) found += (unsigned)__popcll(__ballot(l == 0 && sA >= 0)) + (unsigned)__popcll(__ballot(l == 0 && sB >= 0));
        if (rare) {
#pragma unroll 1
            for (int qq = 0; qq < QN; ++qq) {  // a plain loop: the wave-wide table functions are emitted once
                if (!((rare >> (qq * QG)) & 1ull)) continue;
                const uint32_t rpr = (uint32_t)__builtin_amdgcn_readlane((int)pr, qq * QG);
                const int rsA = __builtin_amdgcn_readlane(sA, qq * QG), rsB = __builtin_amdgcn_readlane(sB, qq * QG);
                const int rnewb = __builtin_amdgcn_readlane((int)gslow, qq * QG);
                const uint32_t *rcN = s_cnt + (size_t)qq * Kpad;
                auto rdA = [&](int k) { return block_loss(rcN, k, false, A < rpr, same, K, nb, pk_shift, pk_sub); };
                auto rdB = [&](int k) { return block_loss(rcN, k, true, B < rpr, same, K, nb, pk_shift, pk_sub); };
                if (rsA == SLOT_SLOW) {
                    const uint32_t lo = min(A, rpr), hi = max(A, rpr);
                    const int slot = table_find_from(c, pack_pair(lo, hi), hash_pair(lo, hi), 1);
                    if (slot >= 0) {
                        const bool gone = table_update(ev, slot, pack_pair(lo, hi), [&](int k, uint32_t old) { return old - rdA(k); }, false);
                        if constexpr (STATS) deletes += (unsigned)gone, ++found;
                    }
                }
                if (rsB == SLOT_SLOW) {
                    const uint32_t lo = min(B, rpr), hi = max(B, rpr);
                    const int slot = table_find_from(c, pack_pair(lo, hi), hash_pair(lo, hi), 1);
                    if (slot >= 0) {
                        const bool gone = table_update(ev, slot, pack_pair(lo, hi), [&](int k, uint32_t old) { return old - rdB(k); }, false);
                        if constexpr (STATS) deletes += (unsigned)gone, ++found;
                    }
                }
                if (rnewb) {
                    table_insert(ev, rpr, Nw, load_row(c.rows, rpr), rnew, [&](int k) { return rcN[k]; }, false);
                    if constexpr (STATS) ++inserts;
                }
            }
        }
        UPD_TIMER_PASS_END  // slow path + block creation
        lds_fence();  // the next pass overwrites the counters
    }
    UPD_TIMER_FLUSH
}

// special_pairs: the pairs among the rows a step modified -- (A,A), (A,B), (B,B): their blocks are re-counted from scratch; (A,N), (B,N),
// (N,N): new -- from the exact counts the substitution block left in sp_cnt (select_body used to write them itself: the table is now
// written by this kernel only).  One wavefront per pair.  Like every block this kernel re-evaluates they pass their best entry to fold_entry,
// changed or not.
// Two workgroups per chain share the work, one pair per wavefront and ONE turn each (find -> re-count / create: the longest dependent chain
// of this kernel; with all six in one workgroup of four waves it took two turns): part 0 the four pairs with A, part 1 (B,N), (N,N) and the
// listed entries.
template <class Cell, bool SEEDED = false, bool WEIGHTED = false, bool SLACK = false> __device__ __forceinline__ void special_pairs(ChainDev *gq, const UpdStep<Cell> &u, int part) {
    const Ctx &c = u.c;
    const uint32_t A = u.A, B = u.B, Nw = u.Nw;
    const BlockEval<SEEDED, WEIGHTED, SLACK> ev{c, u.dcw, u.ord, u.slk};
    const DA_GLOBAL uint32_t *spc = (const DA_GLOBAL uint32_t *)gq->sp_cnt;
    const RowInfo ra = load_row(c.rows, A), rb = load_row(c.rows, B), rn = load_row(c.rows, Nw);
    const int lane = lane_id();
    for (int sp = part * UPD_WAVES + wave_id(); sp < min(6, (part + 1) * UPD_WAVES); sp += UPD_WAVES) {
        // this kernel's wave order 0 1 3 2 4 5 of the rows of special_pair: the four pairs with A, then (B,N), (N,N).  (Spelled as selects: an order array
        // indexed by the wave becomes a load from constant memory in front of the longest dependent chain of the kernel)
        const int row = sp == 2 ? 3 : sp == 3 ? 2 : sp;
        const SpecialPair p = special_pair(row, A, B, Nw);
        if (!p.active) continue;
        const RowInfo xa = pick_row(p.lo == Nw, rn, pick_row(p.lo == A, ra, rb)), xb = pick_row(p.hi == Nw, rn, pick_row(p.hi == A, ra, rb));
        replace_block(ev, p, xa, xb, spc + (size_t)row * c.Kpad);
    }
    // the entries the search listed (they touch exactly one of A / B and reach the untouched entry): a block whose other row is a partner
    // row is re-evaluated by the partner waves of this launch, which pass its best entry on themselves; the others are unchanged -- passed on here.
    // Partner row = a row with digits in a substituted column: bit r of the row bitmaps of those columns (A, B, N are never the other row)
    if (c.rword && part == 1) {
        const int nl = (int)gq->l_n[(gq->iter - 1) & 1];
        const CandEntry *ll = &gq->l_list[(gq->iter - 1) & 1][0];
        const uint32_t *colbits = gq->colbits;
        const int cbw = gq->cb_words;
        for (int e = (wave_id() + 2) % UPD_WAVES; e < nl; e += UPD_WAVES) {  // (waves 2 and 3 first: 0 and 1 had a pair)
            const unsigned long long tw = ll[e].tie;
            uint32_t i0, i1;
            tie_rows<SEEDED>(tw, c.seed, ev.ord, i0, i1);
            const uint32_t r = (i0 == A || i0 == B) ? i1 : i0;
            int hit = 0;
            for (int k = lane; k < u.m; k += WAVE) hit |= (int)((colbits[(size_t)u.mcol[k] * cbw + (r >> 5)] >> (r & 31)) & 1u);
            if (!__any(hit) && lane == 0) fold_entry(c, (uint32_t)ll[e].rank, tw);
        }
    }
}

// update_body: the partner rows [block_y * NWV * QN + ..., stride grid_y * NWV * QN) of chain `gq`'s current step, by a
// workgroup of NWV wavefronts (k_iter_update: 256-thread blocks, grid = chains x blocks per chain).
template <class Cell, int NWV, bool STATS, bool SEEDED = false, bool WEIGHTED = false, bool SLACK = false>
__device__ __forceinline__ void update_body(ChainDev *gq, bool in_range, int block_y, int grid_y) {
    constexpr int NTHR = NWV * WAVE;
    // Grid (chains padded to a multiple of 8, blocks per chain): the chain index is the FAST grid dimension.  Workgroups go to
    // the XCDs round-robin by their linear id, so all blocks of chain c -- and block c of k_iter_select, which has the same
    // linear id modulo 8 -- run on XCD c mod 8: the table lines, bounds and lists of a chain stay in ONE of the eight
    // non-coherent L2s instead of being spread over all of them.
    const UpdStep<Cell> u = load_upd_step<Cell, SEEDED, WEIGHTED, SLACK>(gq);
    if (!in_range || u.done) return;
    if (block_y >= grid_y - 2) {  // the last two blocks of a chain: the six blocks of the pairs among {A, B, new row}
        special_pairs<Cell, SEEDED, WEIGHTED, SLACK>(gq, u, block_y - (grid_y - 2));
        return;
    }
    grid_y -= 2;
    // the grid is sized for the partner counts of the first steps of a chain (thousands); later most blocks have nothing
    // to do and leave before the hand-off is copied
    if (block_y * (NWV * QN) >= u.n_partners) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
    UpdLds<Cell> s;
    s.carve(smem, smem + align16(UpdLds<Cell>::table_bytes(u.c.n_out)) + (size_t)wid * UpdLds<Cell>::wave_bytes(u.c.Kpad), u.c.n_out);
    const int total_waves = grid_y * NWV, gw = block_y * NWV + wid;
    // ---- ONE vector round trip: the group's first partner reference and the new row's record leave together with the
    // hand-off of k_iter_select (they used to wait behind the hand-off barrier: two more dependent round trips)
    const unsigned long long ref0 = gw * QN + (lane >> QG_LOG2) < u.n_partners ? u.plist[gw * QN + (lane >> QG_LOG2)] : 0ull;
    const RowInfo rnew = load_row(u.c.rows, u.Nw);
    __shared__ unsigned int s_stat[3];
    if constexpr (STATS)
        if (tid < 3) s_stat[tid] = 0;
    copy_handoff<Cell>(u, s, tid, NTHR);  // one pass, one barrier (the column map arrives ready-made)
    __syncthreads();
    unsigned int found = 0, inserts = 0, deletes = 0;
    update_partners<Cell, STATS, SEEDED, WEIGHTED, SLACK>(gq, u, s, gw * QN, total_waves * QN, u.n_partners, ref0, rnew, found, inserts, deletes);
    if constexpr (!STATS) return;
    // statistics: summed per block in LDS, then ONE pair of device atomics per block.  (Four atomics per wave on one line
    // of the chain descriptor -- 640 per chain and launch, from all XCDs -- serialise at ~12 ns each and every launch had
    // to wait for them; the partner / cell counts are added by k_iter_select, which knows them without counting.)
    if (lane == 0 && (found | inserts | deletes)) {
        if (found) atomicAdd(&s_stat[0], found);
        if (inserts) atomicAdd(&s_stat[1], inserts);
        if (deletes) atomicAdd(&s_stat[2], deletes);
    }
    __syncthreads();
    if (tid == 0) {
        if (s_stat[0]) atomicAdd(&gq->st_found, (unsigned long long)s_stat[0]);
        if (s_stat[1]) atomicAdd(&gq->st_inserts, (unsigned long long)s_stat[1]);
        if (s_stat[1] != s_stat[2]) atomicAdd(&gq->n_live, s_stat[1] - s_stat[2]);  // blocks created less blocks deleted by this workgroup (modulo 2^32)
    }
}
template <class Cell, bool STATS, bool SEEDED = false, bool WEIGHTED = false, bool SLACK = false>
__global__ void __launch_bounds__(UPD_THREADS, DA_UPD_OCC) __attribute__((amdgpu_num_sgpr(DA_UPD_SGPRS))) k_iter_update(ChainDev *chains, int n_chains) {
    // Grid (chains padded to a multiple of 8, blocks per chain): the chain index is the FAST grid dimension (see update_body)
#ifdef DA_STEP_CLOCKS
    ChainDev *gk = &chains[(int)blockIdx.x < n_chains ? blockIdx.x : 0];
    const bool clk_on = (int)blockIdx.x < n_chains && !gk->done;
    const int clk_par = (gk->iter - 1) & 1;
    if (clk_on && threadIdx.x == 0) CLK_MARK(gk, clk_par, 2, true);
#endif
    update_body<Cell, UPD_WAVES, STATS, SEEDED, WEIGHTED, SLACK>(&chains[(int)blockIdx.x < n_chains ? blockIdx.x : 0], (int)blockIdx.x < n_chains, (int)blockIdx.y, (int)gridDim.y);  // clamped: the descriptor read is unconditional
#ifdef DA_STEP_CLOCKS
    __syncthreads();
    if (clk_on && threadIdx.x == 0) CLK_MARK(gk, clk_par, 3, false);
#endif
}

// ================================================================================= column-sharded chains (cmvm_shard.h)
// The chain holds the digits of a slice of the columns and a replica of the pair table; counts are sums over columns,
// exchanged between the ranks as int32 slabs (all-reduce(sum) between the kernels below, driven by cmvm_shard.cc).

// grid (ceil(n_pairs / 4)): one wave per pair of input rows: partial counts over the own columns -> cs_init [n_pairs][K]
template <class Cell> __global__ void __launch_bounds__(256) k_cs_init_counts(ChainDev *g) {
    const Ctx c = make_ctx(g, 0);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t *cnt = reinterpret_cast<uint32_t *>(smem) + (size_t)wave_id() * c.Kpad;
    const long long n_in = g->n_in, n_pairs = n_in * (n_in + 1) / 2;
    const long long p = (long long)blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (p >= n_pairs) return;
    uint32_t lo, hi;
    pair_of_index(p, lo, hi);
    count_row_pair<Cell>(c, reinterpret_cast<const typename RowFmt<Cell>::Entry *>(g->rlist), lo, hi, cnt);
    for (int k = lane_id(); k < c.K; k += WAVE) g->cs_init[(size_t)p * c.K + k] = (int32_t)cnt[k];
}
// same grid: the summed counts into the (replicated) table
template <class Cell> __global__ void __launch_bounds__(256) k_cs_init_table(ChainDev *g) {
    const Ctx c = make_ctx(g, 0);
    const long long n_in = g->n_in, n_pairs = n_in * (n_in + 1) / 2;
    const long long p = (long long)blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (p >= n_pairs) return;
    uint32_t lo, hi;
    pair_of_index(p, lo, hi);
    const int32_t *cnt = g->cs_init + (size_t)p * c.K;
    if (!wave_any_ge2(cnt, c.K)) return;
    if (c.method < 0) {  // unknown method string with a non-empty table: the reference throws here
        if (lane_id() == 0) g->unknown_hit = 1;
        return;
    }
    table_insert(BlockEval<false, false>{c, 0u, 0u}, lo, hi, load_row(c.rows, lo), load_row(c.rows, hi), [&](int k) { return (uint32_t)cnt[k]; });
}

// one block: union of the partner rows of all ranks (summed flag fields != 0), ascending row ids -> cs_uni, cs_nuni
// `report` (pinned host memory, mapped): {sequence number of the step, size of the union, the three summed status words} -- what the host needs
// between the two exchanges of a step, written by the device itself: no device-to-host copies and no stream synchronisation per step
// (each of the two small copies was a DMA operation of ~10 us; round 6).  The sequence number is stored last, behind a system-scope fence.
__global__ void __launch_bounds__(1024) k_cs_union(ChainDev *g, volatile int *report, int seq, int flag_words) {
    __shared__ int s_part[16], s_base[17];
    const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
    const int n_rows = (int)g->Nw;  // rows that existed before this step's new row
    const int per = (n_rows + 1023) / 1024;
    const int r0 = min(tid * per, n_rows), r1 = min(r0 + per, n_rows);
    int mine = 0;
    for (int r = r0; r < r1; ++r) mine += ((g->cs_flags[r >> 2] >> (8 * (r & 3))) & 0xFF) != 0;
    int inc = mine;
    for (int o = 1; o < WAVE; o <<= 1) {
        int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == WAVE - 1) s_part[wid] = inc;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int w = 0; w < 16; ++w) {
            s_base[w] = run;
            run += s_part[w];
        }
        s_base[16] = run;
        g->cs_nuni = run;
        if (report) {
            report[1] = run;
            report[2] = g->cs_flags[flag_words];
            report[3] = g->cs_flags[flag_words + 1];
            report[4] = g->cs_flags[flag_words + 2];
            __threadfence_system();
            report[0] = seq;
        }
    }
    __syncthreads();
    int at = s_base[wid] + inc - mine;
    for (int r = r0; r < r1; ++r)
        if (((g->cs_flags[r >> 2] >> (8 * (r & 3))) & 0xFF) != 0) g->cs_uni[at++] = (uint32_t)r;
}

// grid (ceil(n_union / 4)): one wave per row of the union: this rank's partial count changes over its own substituted
// columns -> slab [6 + 3 u .. 6 + 3 u + 2][K] = {lost with A, lost with B, gained with the new row}
template <class Cell> __global__ void __launch_bounds__(256) k_cs_partial(ChainDev *g) {
    using F = RowFmt<Cell>;
    using Entry = typename F::Entry;
    const Ctx c = make_ctx(g, 0);
    const int m = g->m, nb = c.n_bits, n_out = c.n_out, K = c.K, Kpad = c.Kpad;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    Cell *s_mA = reinterpret_cast<Cell *>(smem);
    Cell *s_mB = s_mA + n_out;
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_mB + n_out);  // [4][3][Kpad]
    uint16_t *s_cmap = reinterpret_cast<uint16_t *>(s_cnt + 4 * 3 * Kpad);
    const int tid = threadIdx.x, lane = lane_id(), wid = wave_id();
    for (int j = tid; j < n_out; j += 256) s_cmap[j] = 0;
    __syncthreads();
    for (int j = tid; j < m; j += 256) {
        s_cmap[g->mcol[j]] = (uint16_t)(j + 1);
        s_mA[j] = reinterpret_cast<const Cell *>(g->mA)[j];
        s_mB[j] = reinterpret_cast<const Cell *>(g->mB)[j];
    }
    __syncthreads();
    const int u = (int)blockIdx.x * 4 + wid;
    if (u >= g->cs_nuni) return;
    const uint32_t A = g->A, B = g->B, r = g->cs_uni[u];
    const bool same = A == B;
    uint32_t *dA = s_cnt + (size_t)wid * 3 * Kpad, *dB = dA + Kpad, *cN = dB + Kpad;
    for (int k = lane; k < 3 * Kpad; k += WAVE) dA[k] = 0;
    lds_fence();
    const da_u2 ref = g->rowoff[r];
    const Entry *row = reinterpret_cast<const Entry *>(g->rlist) + ref.x;
    for (int j = lane; j < (int)ref.y; j += WAVE) {
        const Entry en = row[j];
        const Cell x = F::cell(en);
        if (!x) continue;
        const int at = (int)s_cmap[F::col(en)];
        if (!at) continue;
        const Cell ma = s_mA[at - 1], mb = s_mB[at - 1];
        for_pairs_part<Cell>(ma, x, A < r, nb, [&](int k) { atomicAdd(&dA[k], 1u); });
        if (same)
            for_pairs_part<Cell>(mb, x, A < r, nb, [&](int k) { atomicAdd(&dA[k], 1u); });
        else
            for_pairs_part<Cell>(mb, x, B < r, nb, [&](int k) { atomicAdd(&dB[k], 1u); });
        for_pairs_cross<Cell>(x, ma, nb, [&](int k) { atomicAdd(&cN[k], 1u); });
    }
    lds_fence();
    int32_t *out = g->cs_slab + (size_t)(6 + 3 * u) * K;
    for (int k = lane; k < K; k += WAVE) {
        out[k] = (int32_t)dA[k];
        out[K + k] = (int32_t)dB[k];
        out[2 * K + k] = (int32_t)cN[k];
    }
}

// grid (ceil((n_union + 6) / 4)): the summed slab into the table.  Waves 0-5: the six pairs among {A, B, new} (their
// blocks are replaced); wave 6 + u: row u of the union (blocks with A and B reduced, block with the new row created).
template <class Cell> __global__ void __launch_bounds__(256) k_cs_apply(ChainDev *g) {
    Ctx c = make_ctx(g, 2 * g->iter - 1);
    // as k_iter_update (load_upd_step): the step being applied is iter - 1; the best entry of every block this launch writes or re-evaluates that
    // reaches the entry the step leaves untouched (spec) is listed for the next pick (fold_entry)
    c.rword = g->spec[(g->iter - 1) & 1].word;
    c.cn = &g->c_n[(g->iter - 1) & 1];
    c.cl = &g->c_list[(g->iter - 1) & 1][0];
    const BlockEval<false, false> ev{c, 0u, 0u};  // (the sharded kernels have no SEEDED / WEIGHTED instantiations)
    const int K = c.K;
    const int w = (int)blockIdx.x * 4 + wave_id();
    const uint32_t A = g->A, B = g->B, Nw = g->Nw;
    const bool same = A == B;
    if (w == 5 && c.rword) {
        // the entries the search listed (they touch exactly one of A / B and reach the untouched entry): a block whose other row is in the union of
        // partner rows is re-evaluated by that row's wave, which passes its best entry on itself; the others are unchanged -- passed on here
        // (special_pairs does the same for ordinary chains).  In the union <=> the row's summed flag field is not zero.
        const int nl = (int)g->l_n[(g->iter - 1) & 1];
        const CandEntry *ll = &g->l_list[(g->iter - 1) & 1][0];
        if (lane_id() == 0)
            for (int e = 0; e < nl; ++e) {
                const unsigned long long tw = ll[e].tie;
                uint32_t i0, i1;
                tie_rows<false>(tw, c.seed, 0u, i0, i1);
                const uint32_t r = (i0 == A || i0 == B) ? i1 : i0;
                if (((g->cs_flags[r >> 2] >> (8 * (r & 3))) & 0xFF) == 0) fold_entry(c, (uint32_t)ll[e].rank, tw);
            }
    }
    if (w < 6) {  // slab row w = count vector w of special_pair
        const SpecialPair p = special_pair(w, A, B, Nw);
        if (p.active) replace_block(ev, p, load_row(c.rows, p.lo), load_row(c.rows, p.hi), g->cs_slab + (size_t)w * K);
        return;
    }
    const int u = w - 6;
    if (u >= g->cs_nuni) return;
    const uint32_t r = g->cs_uni[u];
    const int32_t *dA = g->cs_slab + (size_t)(6 + 3 * u) * K, *dB = dA + K, *cN = dB + K;
    {
        const uint32_t lo = min(A, r), hi = max(A, r);
        const int slot = table_find(c, pack_pair(lo, hi), hash_pair(lo, hi));
        if (slot >= 0) table_update(ev, slot, pack_pair(lo, hi), [&](int k, uint32_t old) { return old - (uint32_t)dA[k]; });
    }
    if (!same) {
        const uint32_t lo = min(B, r), hi = max(B, r);
        const int slot = table_find(c, pack_pair(lo, hi), hash_pair(lo, hi));
        if (slot >= 0) table_update(ev, slot, pack_pair(lo, hi), [&](int k, uint32_t old) { return old - (uint32_t)dB[k]; });
    }
    if (wave_any_ge2(cN, K)) table_insert(ev, r, Nw, load_row(c.rows, r), load_row(c.rows, Nw), [&](int k) { return (uint32_t)cN[k]; });
    if (lane_id() == 0) atomicAdd(&g->st_partners, 1ull);
}

// ------------------------------------------------------------------------------------------------ k_extract
// grid (ceil(n_out / 4), n_chains): one wave per column compacts the surviving (row, cell) entries in row order.
template <class Cell> __global__ void __launch_bounds__(256) k_extract(ChainDev *chains) {
    using O = CellOps<Cell>;
    using F = RowFmt<Cell>;
    ChainDev &ch = chains[blockIdx.y];
    int j = blockIdx.x * (blockDim.x / WAVE) + wave_id();
    if (j >= ch.n_out) return;
    const auto *rl = reinterpret_cast<const typename F::Entry *>(ch.rlist);
    int lane = lane_id(), len = ch.collen[j], out = 0;
    for (int base = 0; base < len; base += WAVE) {
        int e = base + lane;
        Cell c = 0;
        uint32_t r = 0;
        if (e < len) {
            const unsigned long long ref = ch.collist[(size_t)j * ch.lcap + e];
            r = ref_row(ref);
            const auto *row = rl + ref_off(ref);
            if ((int)r < ch.n_in)
                c = F::cell(row[j]);  // dense input row
            else {  // sparse row, sorted by column: binary search for column j (listed here, so it is present)
                int lo = 0, hi = (int)ref_len(ref) - 1;
                while (lo < hi) {
                    int mid = (lo + hi) >> 1;
                    if (F::col(row[mid]) < (uint32_t)j)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                const auto en = row[lo];
                c = F::col(en) == (uint32_t)j ? F::cell(en) : (Cell)0;
            }
        }
        unsigned long long nz = __ballot(c != 0);
        if (c != 0) {
            size_t at = (size_t)j * ch.lcap + out + __popcll(nz & ((1ull << lane) - 1));
            ch.fin_row[at] = r;
            ch.fin_cell[at] = (unsigned long long)O::plus(c) | ((unsigned long long)O::minus(c) << 32);
        }
        out += __popcll(nz);
    }
    if (lane == 0) ch.fin_count[j] = (uint32_t)out;
}

// ------------------------------------------------------------------------------------------------ k_pack
// grid (n_chains): prefix sum of the per-column counts and a dense copy of the surviving digits and of the row
// latencies, so that the download is proportional to the result instead of to the list capacities.
__global__ void __launch_bounds__(256) k_pack(ChainDev *chains) {
    ChainDev &ch = chains[blockIdx.x];
    __shared__ uint32_t s_total;
    const int n_out = ch.n_out, tid = threadIdx.x, lane = lane_id(), nw = blockDim.x / WAVE;
    if (tid < WAVE) {  // exclusive prefix by the first wave, 64 columns per step
        uint32_t run = 0;
        for (int base = 0; base < n_out; base += WAVE) {
            int j = base + lane;
            uint32_t v = j < n_out ? ch.fin_count[j] : 0u, inc = v;
            for (int o = 1; o < WAVE; o <<= 1) {
                uint32_t t = (uint32_t)__shfl_up((int)inc, o);
                if (lane >= o) inc += t;
            }
            if (j < n_out) ch.fin_start[j] = run + inc - v;
            run += (uint32_t)__shfl((int)inc, WAVE - 1);
        }
        if (lane == 0) {
            ch.fin_start[n_out] = run;
            ch.pk_total = run;
            s_total = run;
        }
    }
    __syncthreads();
    if (s_total > (uint32_t)ch.pk_cap) {
        if (tid == 0) ch.error = E_LIST_CAPACITY;
        return;
    }
    for (int j = wave_id(); j < n_out; j += nw) {
        const uint32_t cnt = ch.fin_count[j], dst = ch.fin_start[j];
        const size_t src = (size_t)j * ch.lcap;
        for (uint32_t e = lane; e < cnt; e += WAVE) {
            ch.pk_row[dst + e] = ch.fin_row[src + e];
            ch.pk_cell[dst + e] = ch.fin_cell[src + e];
        }
    }
    for (int r = tid; r < ch.n_rows; r += blockDim.x) ch.pk_lat[r] = ch.rows[r].lat;
}

// ------------------------------------------------------------------------------------------------ k_gather
// grid (blocks, pieces): the result arrays of all chains of a batch (seven per chain, scattered over the arena) copied into ONE
// contiguous buffer, which then leaves in a single device-to-host copy (448 small copies per 64-chain batch before: each a DMA
// operation of its own, ~10 us apiece on one stream).  Sources start on 256-byte boundaries, destinations on 64-byte ones.
struct GatherPiece {
    const void *src;
    unsigned long long dst_off, bytes;
};
__global__ void __launch_bounds__(256) k_gather(const GatherPiece *pieces, unsigned char *dst) {
    const GatherPiece pc = pieces[blockIdx.y];
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t n16 = (size_t)pc.bytes / 16;
    const da_i4 *s16 = reinterpret_cast<const da_i4 *>(pc.src);
    da_i4 *d16 = reinterpret_cast<da_i4 *>(dst + pc.dst_off);
    for (size_t i = t0; i < n16; i += stride) d16[i] = s16[i];
    const unsigned char *s1 = reinterpret_cast<const unsigned char *>(pc.src);
    unsigned char *d1 = dst + pc.dst_off;
    for (size_t i = n16 * 16 + t0; i < (size_t)pc.bytes; i += stride) d1[i] = s1[i];
}

// ------------------------------------------------------------------------------------------------ k_col_dist
// Stage-1 distance matrix: d0[a][b] = sum_i nnzNAF(M[i,a] - M[i,b]), d1 with '+'.  grid (ceil(W/16), ceil(W/16)),
// block 16x16: a 16x16 tile of (a,b); the two 16-column strips of M are staged through LDS 64 rows at a time.
__global__ void __launch_bounds__(256) k_col_dist(const int32_t *aug, int n_in, int W, long long *d0, long long *d1) {
    __shared__ int32_t sa[64][17], sb[64][17];
    int ta = threadIdx.y, tb = threadIdx.x;
    int a = blockIdx.y * 16 + ta, b = blockIdx.x * 16 + tb;
    int tid = ta * 16 + tb;
    long long acc0 = 0, acc1 = 0;
    for (int base = 0; base < n_in; base += 64) {
        for (int q = tid; q < 64 * 16; q += 256) {
            int i = base + q / 16, c = q % 16;
            int ca = blockIdx.y * 16 + c, cb = blockIdx.x * 16 + c;
            sa[q / 16][c] = (i < n_in && ca < W) ? aug[(size_t)i * W + ca] : 0;
            sb[q / 16][c] = (i < n_in && cb < W) ? aug[(size_t)i * W + cb] : 0;
        }
        __syncthreads();
        int rows = min(64, n_in - base);
        for (int i = 0; i < rows; ++i) {
            int32_t x = sa[i][ta], y = sb[i][tb];
            acc0 += naf_weight(x - y);
            acc1 += naf_weight(x + y);
        }
        __syncthreads();
    }
    if (a < W && b < W) {
        d0[(size_t)a * W + b] = acc0;
        d1[(size_t)a * W + b] = acc1;
    }
}

// NAF digits of a flat int32 array (int_arr_to_csd, bit_decompose.cc:22-42): out[i][b] in {-1,0,1}
__global__ void __launch_bounds__(256) k_naf_digits(const int32_t *x, long long n, int N, int8_t *out) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t p, m;
    naf_masks(x[i], p, m);
    for (int b = 0; b < N; ++b) out[i * N + b] = (int8_t)(((p >> b) & 1) - ((m >> b) & 1));
}
__global__ void __launch_bounds__(256) k_absmax(const int32_t *x, long long n, unsigned int *out) {
    unsigned int mx = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int32_t v = x[i];
        mx = max(mx, (unsigned int)(v < 0 ? -v : v));
    }
    mx = wave_max_u32(mx);
    if (lane_id() == 0) atomicMax(out, mx);
}

// =================================================================================================== host side
// in headers by concern, in dependency order; DA_ENGINE_TU lets them compile here and nowhere else
#define DA_ENGINE_TU
#include "hip_host_util.h"
#include "hip_chain_setup.h"
#include "hip_batch.h"
#include "hip_shard_engine.h"
#include "hip_stage01.h"

}  // namespace gpu
}  // namespace da
