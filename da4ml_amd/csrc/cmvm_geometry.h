// cmvm_geometry.h -- size of a greedy chain's row arena and pair-count table.  Plain C++, shared by
// HipBackend::run_chains and the column-sharded chain (derive_geometry, hip_chain_setup.h) and by the CPU tests (tests/geometry).
#pragma once

#include <algorithm>
#include <cstdint>

#include "cmvm_core.h"
#include "cmvm_host.h"

namespace da {

// Tables the heuristic sizes at up to 2^25 slots keep the heuristic's size; larger ones are capped by what the chain can hold.
constexpr int TABLE_HEURISTIC_LOG2 = 25;
// The largest table: 2^30 slots.  Slot indices stay below 2^31 (the kernels keep them in int), C stays a uint32_t.
constexpr int TABLE_MAX_LOG2 = 30;
// Inverse load factor of a capped table: slots per block the chain can hold.
constexpr int TABLE_SLOTS_PER_PAIR = 2;

struct TableGeometry {
    uint32_t C;      // slots, a power of two
    int gs_log2;     // slots per group of the selection's bounds
    int n_groups;    // C >> gs_log2, at most max_groups
    long long rcap;  // rows of the chain's arena
};

inline uint64_t pow2_ceil_u64(uint64_t v) {
    uint64_t p = 1;
    while (p < v && p < (1ull << 62)) p <<= 1;
    return p;
}

// Rows and pair table of a chain.
//   * rows: the inputs, one per greedy step, one spare.  Steps: every step removes at least one digit, typical chains need ~D0/8 of
//     them, the arena is sized for max(16, D0 row_scale / 4) (at most D0);
//   * slots, heuristic: blocks peak well above the initial pair count when rows are dense -- 0.8 x initial pairs x max(4, n_in / 5);
//   * a chain the heuristic gives more than 2^25 slots (none of them ran before) is sized by what it can hold instead.  Rows: n_in + D0 + 1,
//     the hard bound (no row-capacity retry).  Blocks: one per row pair that shares a column, and the digits of a column never grow, so at
//     most sum_j C(D_j, 2) + D0 (prep_pairs + prep_digits; a row paired with itself included) and at most rcap (rcap + 1) / 2; at
//     TABLE_SLOTS_PER_PAIR slots per block, plus the slots that the tombstones of one launch keep from re-use (the blocks of the step's two
//     rows: 2 rcap).  table_scale scales this cap too, so the capacity retry (x4) and DA4ML_HIP_TABLE_SCALE still grow the table; the
//     heuristic's size stays the upper end;
//   * at most 2^30 slots, at least 256; groups of 2^8 slots and up, at most max_groups of them.
inline TableGeometry table_geometry(const ChainJob &job, long long prep_pairs, long long prep_digits, double table_scale, double row_scale,
                                    int max_groups) {
    const long long D0 = prep_digits;
    long long steps = 0;
    if (job.method != M_DUMMY && job.method >= 0) {
        steps = std::max<long long>(16, (long long)(D0 * row_scale / 4));
        if (steps > D0) steps = std::max<long long>(D0, 1);
    }
    TableGeometry g;
    g.rcap = (long long)job.n_in + steps + 1;
    const long long pairs0 = std::min<long long>((long long)job.n_in * (job.n_in + 1) / 2, std::max<long long>(prep_pairs, 1));
    const double growth = std::max(4.0, job.n_in / 5.0);
    double want = std::max(1024.0, 0.8 * pairs0 * growth * table_scale);
    if (job.method == M_DUMMY) want = 64;
    uint64_t C = pow2_ceil_u64((uint64_t)std::min(want, 0x1p62));
    if (C > (1ull << TABLE_HEURISTIC_LOG2)) {
        if (steps) g.rcap = (long long)job.n_in + std::max<long long>(D0, 1) + 1;
        const double rcap = (double)g.rcap;
        const double blocks = std::min(rcap * (rcap + 1) / 2, (double)std::max<long long>(prep_pairs, 0) + (double)D0);
        const double cap = (TABLE_SLOTS_PER_PAIR * blocks + 2 * rcap) * table_scale;
        C = std::min<uint64_t>(C, pow2_ceil_u64((uint64_t)std::min(cap, 0x1p62)));
        C = std::min<uint64_t>(C, 1ull << TABLE_MAX_LOG2);
    }
    g.gs_log2 = 8;
    while ((C >> g.gs_log2) > (uint64_t)max_groups) ++g.gs_log2;
    if (C < 256) C = 256;
    g.C = (uint32_t)C;
    g.n_groups = (int)(C >> g.gs_log2);
    return g;
}

}  // namespace da
