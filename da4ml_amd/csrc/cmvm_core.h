// cmvm_core.h -- scalar building blocks of the CMVM greedy engine, shared verbatim by the HIP kernels
// (cmvm_engine.hip) and by the sequential reformulation model used in tests (tests/model/engine_model.cc).
//
// Everything here is integer / bit manipulation plus a handful of IEEE-exact float operations, written so
// that host (g++) and device (hipcc --offload-arch=gfx950 -ffp-contract=off) produce identical bits.
//
// Data model (differs from the reference's sparse int8 digit lists, types.hh:104-141):
//   * a CELL holds all CSD digits of one (row, output column): two position bitmasks, `plus` in the low
//     half and `minus` in the high half of a 32-bit (n_bits <= 16) or 64-bit (n_bits <= 32) word;
//   * a pair KEY index enumerates (sub, shift): idx = sub * (2N-1) + shift + (N-1), so that a larger idx
//     is exactly a larger (sub, shift) in the reference's Pair ordering (types.hh:28-36);
//   * a BLOCK holds the occurrence counts of all K = 2(2N-1) keys of one row pair (id0 <= id1).
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DA_HD __host__ __device__ __forceinline__
#else
#define DA_HD inline
#endif

namespace da {

enum Method : int { M_MC = 0, M_MC_DC = 1, M_MC_PDC = 2, M_WMC = 3, M_WMC_DC = 4, M_WMC_PDC = 5, M_DUMMY = 6 };

enum ChainError : int {
    E_OK = 0,
    E_ROW_CAPACITY = 1,    // more greedy iterations than the row arena holds
    E_TABLE_CAPACITY = 2,  // pair-block table arena too small
    E_LIST_CAPACITY = 3,   // a column row-list overflowed (cannot happen with the exact bound; guarded anyway)
    E_FLOAT_DOMAIN = 4,    // the latency model met a step it has no logarithm for (subnormal / non-positive)
    E_COUNT_OVERFLOW = 5,  // a pair count exceeded 16 bits
    E_REMOTE_ERROR = 6,    // column-sharded chain: another rank failed with something other than a capacity error, or the ranks fell out of step -- not worth a retry
};

struct RowInfo {  // quantised interval + latency of one row (reference Op.qint / Op.latency)
    float lo, hi, step, lat;
};

// ----------------------------------------------------------------------------------------------- bits
DA_HD uint32_t f2u(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
DA_HD float u2f(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
DA_HD int popc32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}
DA_HD int ctz32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)x) - 1;
#else
    return __builtin_ctz(x);
#endif
}

template <class Cell> struct CellOps;
template <> struct CellOps<uint32_t> {
    static constexpr int HALF = 16;
    static DA_HD uint32_t plus(uint32_t c) { return c & 0xFFFFu; }
    static DA_HD uint32_t minus(uint32_t c) { return c >> 16; }
    static DA_HD uint32_t make(uint32_t p, uint32_t m) { return p | (m << 16); }
};
template <> struct CellOps<uint64_t> {
    static constexpr int HALF = 32;
    static DA_HD uint32_t plus(uint64_t c) { return (uint32_t)c; }
    static DA_HD uint32_t minus(uint64_t c) { return (uint32_t)(c >> 32); }
    static DA_HD uint64_t make(uint32_t p, uint32_t m) { return (uint64_t)p | ((uint64_t)m << 32); }
};

DA_HD int key_count(int n_bits) { return 2 * (2 * n_bits - 1); }
DA_HD int key_index(int shift, int sub, int n_bits) { return sub * (2 * n_bits - 1) + shift + (n_bits - 1); }
DA_HD void key_decode(int idx, int n_bits, int &shift, int &sub) {
    int w = 2 * n_bits - 1;
    sub = idx >= w;
    shift = idx - sub * w - (n_bits - 1);
}

// bit p of the result = bit (p + s) of x   (s may be negative)
DA_HD uint32_t take_from(uint32_t x, int s) { return s >= 0 ? (s >= 32 ? 0u : x >> s) : (-s >= 32 ? 0u : x << (-s)); }
// bit (p + s) of the result = bit p of x
DA_HD uint32_t move_by(uint32_t x, int s) { return take_from(x, -s); }

// ------------------------------------------------------------------------------------ CSD (NAF) digits
// Non-adjacent form of x: identical digits to the reference's threshold recoding (bit_decompose.cc:22-42);
// checked exhaustively against the oracle in tests/test_oracle.py.
DA_HD void naf_masks(int32_t x, uint32_t &plus, uint32_t &minus) {
    uint32_t a = x < 0 ? (uint32_t)(-(int64_t)x) : (uint32_t)x;
    uint64_t x3 = (uint64_t)a * 3u;
    uint32_t pos = (uint32_t)((x3 & ~(uint64_t)a) >> 1);
    uint32_t neg = (uint32_t)((~x3 & (uint64_t)a) >> 1);
    plus = x < 0 ? neg : pos;
    minus = x < 0 ? pos : neg;
}
DA_HD int naf_weight(int32_t x) {
    uint32_t a = x < 0 ? (uint32_t)(-(int64_t)x) : (uint32_t)x;
    uint64_t x3 = (uint64_t)a * 3u;
    uint64_t d = (x3 ^ (uint64_t)a) >> 1;
    return popc32((uint32_t)d) + popc32((uint32_t)(d >> 32));
}
// ------------------------------------------------------------------------------------ digit recoding
// The digits a greedy chain STARTS from (no reference counterpart: the reference always starts from the NAF).  The NAF is one of several
// minimal signed-digit forms of a number (3 = 4 - 1 = 2 + 1); which one the search starts from changes which digit pairs repeat.
//   RECODE_CSD      naf_masks, bit for bit.
//   RECODE_COMPACT  from the NAF digits d, for p from (top position - 2) down to 0: a site d[p+2] = s != 0, d[p+1] = 0, d[p] = -s is
//                   rewritten to d[p+2] = 0, d[p+1] = s, d[p] = s  (4s - s = 2s + s).  The scan runs top down, so a site that a rewrite
//                   creates below it is seen: 11 = 16 - 4 - 1 -> 8 + 4 - 1 -> 8 + 2 + 1.
//   RECODE_SEEDED   the same scan; a site at p is rewritten only when its coin is 1:
//                       coin(seed, |x|, p) = splitmix64(splitmix64(seed) ^ ((uint64_t)|x| << 5 | p)) >> 63
//                   with splitmix64 as da4ml_amd.cmvm.splitmix64 has it.  The coin is keyed by the coefficient's VALUE, not by where it
//                   stands: equal values get equal digits wherever they stand (a coin per matrix entry loses the sharing between them).
// The scan works on the digits of |x| and mirrors them for x < 0: x and -x get mirrored digits.  A rewrite preserves the value and the
// digit count and touches nothing above p + 2: the top position is never raised, so csd_width, naf_weight and everything sized by them
// hold for every mode.
constexpr uint32_t RECODE_CSD = 0, RECODE_COMPACT = 1, RECODE_SEEDED = 2, RECODE_COUNT = 3;
DA_HD uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
DA_HD void digit_masks(int32_t x, uint32_t mode, uint64_t seed, uint32_t &plus, uint32_t &minus) {
    naf_masks(x, plus, minus);
    if (mode == RECODE_CSD) return;
    uint32_t same = x < 0 ? minus : plus, opp = x < 0 ? plus : minus;  // the digits of |x|: +1 | -1
    if (!(same | opp)) return;
    const uint32_t a = x < 0 ? (uint32_t)(-(int64_t)x) : (uint32_t)x;
    const uint64_t key = mode == RECODE_SEEDED ? splitmix64(seed) : 0;
    int top = 31;
    while (!(((same | opp) >> top) & 1u)) --top;
    for (int p = top - 2; p >= 0; --p) {
        const uint32_t hi = 4u << p, mid = 2u << p, lo = 1u << p;
        if ((same | opp) & mid) continue;
        const bool up = (same & hi) && (opp & lo), down = (opp & hi) && (same & lo);  // s = +1 | s = -1
        if (!up && !down) continue;
        if (mode == RECODE_SEEDED && !(splitmix64(key ^ (((uint64_t)a << 5) | (uint64_t)p)) >> 63)) continue;
        if (up)
            same = (same & ~hi) | mid | lo, opp &= ~lo;
        else
            opp = (opp & ~hi) | mid | lo, same &= ~lo;
    }
    plus = x < 0 ? opp : same;
    minus = x < 0 ? same : opp;
}

// digit width N = max(1, ceil(log2(max(maxabs,1) * 1.5)))  (bit_decompose.cc:24-27), in exact integers:
// the smallest N >= 1 with 2^(N+1) >= 3 * maxabs (3*maxabs is never a power of two, so no rounding case).
DA_HD int csd_width(uint32_t max_abs) {
    uint64_t t = 3ull * (max_abs ? max_abs : 1u);
    int n = 1;
    while ((1ull << (n + 1)) < t) ++n;
    return n;
}
// lowest set bit position of a float (bit_decompose.cc:10-20); 127 for zero
DA_HD int lsb_loc(float x) {
    if (x == 0.0f) return 127;
    uint32_t b = f2u(x);
    int e = (int)((b >> 23) & 0xFF);
    uint32_t m = (b & 0x7FFFFFu) + (1u << 23);
    return (int)(int8_t)(e + ctz32(m) - 150);
}
// ceil(log2 x) from the float bit pattern (indexers.hh:12-18), including its int8 wrap
DA_HD int iceil_log2(float x) {
    uint32_t b = f2u(x);
    int e = (int)((b >> 23) & 0xFF);
    return (int)(int8_t)(e - 127 + ((b & 0x7FFFFFu) != 0));
}
// exact 2^s as float for |s| <= 126
DA_HD float pow2f(int s) { return u2f((uint32_t)(s + 127) << 23); }

// ------------------------------------------------------------------------------------ pair occurrences
// Visit every digit pair between cell `lo` (row with the smaller id) and cell `hi` of one column and call
// f(key_index, +1).  Cross-row rule: shift = pos(hi digit) - pos(lo digit), sub = signs differ
// (state_opr.cc:69-77,133-137).
template <class Cell, class F> DA_HD void for_pairs_cross(Cell lo, Cell hi, int n_bits, F &&f) {
    using O = CellOps<Cell>;
    uint32_t lp = O::plus(lo), lm = O::minus(lo), hp = O::plus(hi), hm = O::minus(hi);
    uint32_t la = lp | lm, ha = hp | hm;
    while (la) {
        int p = ctz32(la);
        la &= la - 1;
        int sl = (lm >> p) & 1;
        uint32_t h = ha;
        while (h) {
            int q = ctz32(h);
            h &= h - 1;
            int sh = (hm >> q) & 1;
            f(key_index(q - p, sl ^ sh, n_bits));
        }
    }
}
// Same-row rule: ordered (higher digit, lower digit) => shift = pos(lower) - pos(higher) < 0
// (state_opr.cc:124-131).
template <class Cell, class F> DA_HD void for_pairs_self(Cell c, int n_bits, F &&f) {
    using O = CellOps<Cell>;
    uint32_t cp = O::plus(c), cm = O::minus(c);
    uint32_t all = cp | cm;
    uint32_t hi = all;
    while (hi) {
        int a = ctz32(hi);
        hi &= hi - 1;
        int sa = (cm >> a) & 1;
        uint32_t lo = all & ((1u << a) - 1u);
        while (lo) {
            int b = ctz32(lo);
            lo &= lo - 1;
            int sb = (cm >> b) & 1;
            f(key_index(b - a, sa ^ sb, n_bits));
        }
    }
}
// pairs between a SUBSET of digits `part` of the row `x` and all digits of the other row cell `y`;
// x_is_lo tells which of the two rows has the smaller id.
template <class Cell, class F> DA_HD void for_pairs_part(Cell part, Cell y, bool x_is_lo, int n_bits, F &&f) {
    if (x_is_lo)
        for_pairs_cross<Cell>(part, y, n_bits, f);
    else
        for_pairs_cross<Cell>(y, part, n_bits, f);
}

// ------------------------------------------------------------------------------------ substitution
// Apply the chosen pair (id0=A, id1=B, shift, sub) to one column (state_opr.cc:249-280).
// a, b: cells of rows A and B (b ignored when same_row).  Outputs the digits consumed from A (ma), from B
// (mb) and the cell of the new row (= the consumed A-role digits, position and sign preserved).
template <class Cell> DA_HD void substitute_column(Cell a, Cell b, bool same_row, int shift, int sub, Cell &ma, Cell &mb) {
    using O = CellOps<Cell>;
    uint32_t ap = O::plus(a), am = O::minus(a);
    if (!same_row) {
        uint32_t bp = O::plus(b), bm = O::minus(b);
        uint32_t map = ap & take_from(sub ? bm : bp, shift);
        uint32_t mam = am & take_from(sub ? bp : bm, shift);
        uint32_t tp = move_by(map, shift), tm = move_by(mam, shift);
        ma = O::make(map, mam);
        mb = sub ? O::make(tm, tp) : O::make(tp, tm);
        return;
    }
    // same row: shift < 0; walk the lower digit position upward, each digit used at most once
    int rel = -shift;
    uint32_t avp = ap, avm = am, map = 0, mam = 0, mbp = 0, mbm = 0;
    for (int p = 0; p + rel < O::HALF; ++p) {
        uint32_t bit_lo = 1u << p, bit_hi = 1u << (p + rel);
        uint32_t all = avp | avm;
        if (!(all & bit_lo) || !(all & bit_hi)) continue;
        int s_lo = (avm & bit_lo) != 0, s_hi = (avm & bit_hi) != 0;
        if ((s_lo ^ s_hi) != sub) continue;
        avp &= ~(bit_lo | bit_hi);
        avm &= ~(bit_lo | bit_hi);
        if (s_hi)
            mam |= bit_hi;
        else
            map |= bit_hi;
        if (s_lo)
            mbm |= bit_lo;
        else
            mbp |= bit_lo;
    }
    ma = O::make(map, mam);  // A-role digits (higher position) -> new row
    mb = O::make(mbp, mbm);  // B-role digits (lower position)
}

// ------------------------------------------------------------------------------------ scoring
// n_overlap of overlap_and_accum (indexers.cc:36-56), int8 arithmetic as in the reference
DA_HD int n_overlap(const RowInfo &a, const RowInfo &b) {
    float hi0 = a.hi + a.step, hi1 = b.hi + b.step;
    float st = a.step > b.step ? a.step : b.step;  // std::max(step0, step1)
    int8_t f = (int8_t)(-iceil_log2(st));
    float m0 = __builtin_fabsf(a.lo) < __builtin_fabsf(hi0) ? __builtin_fabsf(hi0) : __builtin_fabsf(a.lo);
    float m1 = __builtin_fabsf(b.lo) < __builtin_fabsf(hi1) ? __builtin_fabsf(hi1) : __builtin_fabsf(b.lo);
    int8_t i_low = (int8_t)iceil_log2(m1 < m0 ? m1 : m0);
    int8_t k = (a.lo < 0 || b.lo < 0) ? 1 : 0;
    return (int)(int8_t)(k + i_low + f);
}

// order-preserving map float -> u32 rank >= 1 (0 is reserved for "not selectable"); -0 == +0; NaN -> 0
DA_HD uint32_t float_rank(float s) {
    if (s != s) return 0;
    if (s == 0.0f) s = 0.0f;
    uint32_t u = f2u(s == 0.0f ? 0.0f : s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rank of one table entry; 0 = cannot be selected.  Larger rank == larger reference score; equal rank ==
// equal score (indexers.cc:6-90).  `ov` = n_overlap, `dl` = |lat0 - lat1|.
// The -dc / -pdc methods subtract a latency penalty: score = float(count) - w * dl (mc-*), float(u32 count * ov) - w * dl (wmc-*), the multiply
// and the subtract each rounded once (never fused: the host is built with -ffp-contract=off).  The reference's w is DC_WEIGHT_MC resp.
// DC_WEIGHT_WMC; mc, wmc and dummy read none.
constexpr float DC_WEIGHT_MC = 1e9f, DC_WEIGHT_WMC = 256.0f;
DA_HD float dc_weight_default(int method) { return method == M_MC_DC || method == M_MC_PDC ? DC_WEIGHT_MC : DC_WEIGHT_WMC; }
namespace detail {
// The one body behind both forms of entry_rank.  Two weights, one per family, because the method is a run-time value: the four-argument form
// hands in both constants, so that each stays a literal of its own instruction, the five-argument form the chain's weight twice.
DA_HD uint32_t entry_rank_weights(uint32_t count, int ov, float dl, int method, float w_mc, float w_wmc) {
    if (count < 2) return 0;
    switch (method) {
    case M_MC: return count + 1;
    case M_WMC: {
#if defined(__HIP_DEVICE_COMPILE__)
        // counts are stored as u16 and |ov| < 2^7: the product fits 32 bits (the 64-bit multiply was four vector
        // instructions, eight times per partner pass)
        if (count <= 0xFFFFu) {
            const int32_t s32 = (int32_t)count * ov;
            return s32 >= 0 ? (uint32_t)s32 + 1 : 0;
        }
#endif
        int64_t s = (int64_t)count * ov;
        return s >= 0 ? (uint32_t)s + 1 : 0;
    }
    case M_MC_DC:
    case M_MC_PDC: {
#if defined(__HIP_DEVICE_COMPILE__)
        float s = __fsub_rn((float)count, __fmul_rn(w_mc, dl));
#else
        float pen = w_mc * dl;
        float s = (float)count - pen;
#endif
        if (method == M_MC_DC && !(s >= 0.0f)) return 0;
        return float_rank(s);
    }
    case M_WMC_DC:
    case M_WMC_PDC: {
        uint32_t prod = count * (uint32_t)ov;  // unsigned wrap for negative overlap, as in the reference
#if defined(__HIP_DEVICE_COMPILE__)
        float s = __fsub_rn((float)prod, __fmul_rn(w_wmc, dl));
#else
        float pen = w_wmc * dl;
        float s = (float)prod - pen;
#endif
        if (method == M_WMC_DC && !(s >= 0.0f)) return 0;
        return float_rank(s);
    }
    default: return 0;
    }
}
}  // namespace detail
// rank with the weight `w` in place of the method's constant
DA_HD uint32_t entry_rank(uint32_t count, int ov, float dl, int method, float w) { return detail::entry_rank_weights(count, ov, dl, method, w, w); }
// the reference's scores: every method with its own constant
DA_HD uint32_t entry_rank(uint32_t count, int ov, float dl, int method) { return detail::entry_rank_weights(count, ov, dl, method, DC_WEIGHT_MC, DC_WEIGHT_WMC); }

// ------------------------------------------------------------------------------------ score slack
// A chain with a slack != 0 (and a tie seed != 0: the slack is keyed by it) draws its pick from the pairs whose score lies within a small fraction
// of the best one -- the restricted candidate list of a randomised greedy search.  No reference counterpart: a restart dimension, never a default.
// Every entry gets a discount of its OWN, a pure function of (count, rows, key, the chain's constants): the table stays exact and incremental.
//   slack_byte(id0, id1, idx, seed) in 0 .. 255: a keyed hash of the row pair and the key index, 32-bit arithmetic only.
//       word = slack_pair_word(id0, id1, seed): the two ids and the two halves of the seed combined by four odd multipliers, then the "lowbias32"
//              finaliser (h ^= h >> 16, h *= 0x7FEB352D, h ^= h >> 15, h *= 0x846CA68B, h ^= h >> 16); once per block (row pair);
//       byte = ((word ^ idx * 0x9E3779) * 0x9E3779B1) >> 24: a 24-bit multiply, an xor, a multiply and a shift per key.  (The xor is what
//              unties the keys of a block: with word * (2 idx + 1), or any form linear in the word, the byte of key 1 is a fixed function of
//              the byte of key 0 in every block -- a correlation of 0.34 between the two over a grid of pairs.)
//   entry_rank_slack(count, ov, dl, method, w, slack, byte), slack in 0 .. 255:
//       base = count (mc family) | the integer product count * ov (wmc family: signed for wmc, the reference's unsigned wrap for wmc-dc / wmc-pdc);
//       0 < base < 2^24:  base -= (base * ((byte * slack) >> 8)) >> 8      -- at most slack / 256 of the score; base * 254 < 2^32: no 64-bit multiply
//       otherwise base is left alone (zero, negative, the unsigned wrap of a negative overlap, products the float would round anyway);
//       then entry_rank's: mc / wmc rank = base + 1; the -dc / -pdc methods float(base) - w * dl with its two single roundings, the `absolute`
//       cut, float_rank.  count < 2 is 0, as there.
// Properties (tests/test_slack_rank.py): slack == 0 is entry_rank(count, ov, dl, method, w) bit for bit; the rank is non-decreasing in count
// (b -> b - floor(b d / 256), d <= 254, never steps down, and 2^24 - 1 maps below 2^24); a discounted base >= 1 stays >= 1 (b d / 256 < b).
// Entries of equal rank are ordered by the chain's tie word, unchanged.
DA_HD uint32_t slack_pair_word(uint32_t id0, uint32_t id1, uint64_t seed) {
    uint32_t h = id0 * 0x9E3779B1u + id1 * 0x85EBCA77u + (uint32_t)seed * 0xC2B2AE3Du + (uint32_t)(seed >> 32) * 0x27D4EB2Fu;
    h ^= h >> 16;
    h *= 0x7FEB352Du;
    h ^= h >> 15;
    h *= 0x846CA68Bu;
    h ^= h >> 16;
    return h;
}
DA_HD uint32_t slack_word_byte(uint32_t word, uint32_t idx) { return ((word ^ (idx * 0x9E3779u)) * 0x9E3779B1u) >> 24; }
DA_HD uint32_t slack_byte(uint32_t id0, uint32_t id1, int idx, uint64_t seed) { return slack_word_byte(slack_pair_word(id0, id1, seed), (uint32_t)idx); }
DA_HD uint32_t slack_discount(uint32_t base, uint32_t slack, uint32_t byte) {
    return base - 1u < 0xFFFFFFu ? base - ((base * ((byte * slack) >> 8)) >> 8) : base;
}
DA_HD uint32_t entry_rank_slack(uint32_t count, int ov, float dl, int method, float w, uint32_t slack, uint32_t byte) {
    if (count < 2) return 0;
    switch (method) {
    case M_MC: return slack_discount(count, slack, byte) + 1;
    case M_WMC: {
#if defined(__HIP_DEVICE_COMPILE__)
        if (count <= 0xFFFFu) {  // (as entry_rank: the product fits 32 bits)
            const int32_t s32 = (int32_t)count * ov;
            return s32 >= 0 ? slack_discount((uint32_t)s32, slack, byte) + 1 : 0;
        }
#endif
        int64_t s = (int64_t)count * ov;
        return s >= 0 ? slack_discount((uint32_t)s, slack, byte) + 1 : 0;
    }
    case M_MC_DC:
    case M_MC_PDC:
    case M_WMC_DC:
    case M_WMC_PDC: {
        const bool mc = method == M_MC_DC || method == M_MC_PDC;
        const uint32_t base = slack_discount(mc ? count : count * (uint32_t)ov, slack, byte);
#if defined(__HIP_DEVICE_COMPILE__)
        float s = __fsub_rn((float)base, __fmul_rn(w, dl));
#else
        float pen = w * dl;
        float s = (float)base - pen;
#endif
        if ((method == M_MC_DC || method == M_WMC_DC) && !(s >= 0.0f)) return 0;
        return float_rank(s);
    }
    default: return 0;
    }
}

// tie-break word: larger == later in the reference's sorted table (id1, id0, sub, shift)
DA_HD uint64_t tie_word(uint32_t id0, uint32_t id1, int idx) {
    return ((uint64_t)id1 << 31) | ((uint64_t)id0 << 7) | (uint64_t)idx;
}

// ------------------------------------------------------------------------------------ seeded tie order
// A chain with a tie seed != 0 settles equal ranks by another strict total order: a random restart of the greedy search.  Only ties
// move: ranks (scores) are what they were, so every such run is a greedy run of the reference's method.  The word keeps the shape
// of the reference's -- 48 bits of the row pair above 7 bits of the key index, below 2^55 -- so that bound words (rank << 32 | tie
// >> 23) order coarser than (rank, tie) as before:
//   * high part: a keyed bijection of the 48 bits (id1 << 24 | id0), invertible steps only -- xor with the seed's low 48 bits,
//     multiply by an odd constant mod 2^48, xor-shift by 24 (its own inverse on 48 bits), xor with the seed's high 48 bits.  The
//     rows of an entry are read back from its word (tie_word_rows);
//   * low part: idx ^ k7, k7 = the seed's top seven bits.  Inside a block (one row pair) the order of the keys is therefore the
//     order of (idx ^ k7): the best entry of a block is the maximum of (rank << 8 | (idx ^ k7)), see tie_block_pos.
// Injective in (id0, id1, idx) for ids < 2^24 and idx < 128.  tie_word_seeded wants seed != 0; the four-argument tie_word takes any.
constexpr uint64_t TIE_PAIR_MASK = (1ull << 48) - 1;
constexpr uint64_t TIE_MUL = 0x9E3779B97F4Bull;  // odd
constexpr uint64_t tie_mul_inverse(uint64_t m) {  // Newton's iteration: correct bits double, from the three of m * m == 1 (mod 8)
    uint64_t x = m;
    for (int i = 0; i < 5; ++i) x *= 2 - m * x;
    return x & TIE_PAIR_MASK;
}
constexpr uint64_t TIE_MUL_INV = tie_mul_inverse(TIE_MUL);
static_assert(((TIE_MUL * TIE_MUL_INV) & TIE_PAIR_MASK) == 1, "inverse of the tie multiplier mod 2^48");
DA_HD uint32_t tie_k7(uint64_t seed) { return (uint32_t)(seed >> 57); }
// position of key `idx` in the within-block order of a seeded chain, and back (an involution); values stay below 128
DA_HD uint32_t tie_block_pos(uint32_t idx, uint64_t seed) { return idx ^ tie_k7(seed); }
DA_HD uint64_t tie_pair_mix(uint64_t pair, uint64_t seed) {  // the bijection of (id1 << 24 | id0)
    uint64_t h = pair ^ (seed & TIE_PAIR_MASK);
    h = (h * TIE_MUL) & TIE_PAIR_MASK;
    h ^= h >> 24;
    return h ^ (seed >> 16);
}
DA_HD uint64_t tie_pair_unmix(uint64_t h, uint64_t seed) {  // and its inverse
    h ^= seed >> 16;
    h ^= h >> 24;
    h = (h * TIE_MUL_INV) & TIE_PAIR_MASK;
    return h ^ (seed & TIE_PAIR_MASK);
}
DA_HD uint64_t tie_word_seeded(uint32_t id0, uint32_t id1, int idx, uint64_t seed) {
    return (tie_pair_mix(((uint64_t)id1 << 24) | (uint64_t)id0, seed) << 7) | (uint64_t)tie_block_pos((uint32_t)idx, seed);
}
DA_HD uint64_t tie_word(uint32_t id0, uint32_t id1, int idx, uint64_t seed) {
    return seed ? tie_word_seeded(id0, id1, idx, seed) : tie_word(id0, id1, idx);
}
// the rows of an entry from its tie word (seed 0: the reference's word), and its key index
DA_HD void tie_word_rows(uint64_t tie, uint64_t seed, uint32_t &id0, uint32_t &id1) {
    const uint64_t h = seed ? tie_pair_unmix(tie >> 7, seed) : tie >> 7;
    id0 = (uint32_t)(h & 0xFFFFFFu);
    id1 = (uint32_t)(h >> 24);
}
DA_HD int tie_word_idx(uint64_t tie, uint64_t seed) { return (int)(((uint32_t)tie & 0x7Fu) ^ tie_k7(seed)); }

// ------------------------------------------------------------------------------------ the second seeded order: newest row first
// The reference lets the larger (id1, id0) win a tie: the pair that re-uses the newest row.  The random order above throws that away; this
// one keeps it and moves only what lies below: among equal ranks the larger id1 still wins, pairs of one id1 are ordered by a keyed
// 24-bit bijection of id0, keys of one pair by idx ^ k7 as above (so the within-block order, tie_block_pos, is shared by both orders):
//   word = id1 << 31 | mix24(id0) << 7 | (idx ^ k7)                                         below 2^55, injective as the others
//   mix24: xor with the seed's low 24 bits, multiply by TIE_MUL mod 2^24, xor-shift by 12 (its own inverse on 24 bits), xor with the
//          seed's bits 24 .. 47.
// A bound word (rank << 32 | word >> 23) holds id1 and the top eight bits of the mixed id0: coarser than (rank, word), as before.
// No reference counterpart: with seed 0 the order is the reference's, whatever TIE_ORDER_* says.
constexpr uint32_t TIE_ORDER_RANDOM = 0, TIE_ORDER_NEWEST = 1, TIE_ORDER_COUNT = 2;
constexpr uint32_t TIE_ID_MASK = 0xFFFFFFu;
static_assert((((TIE_MUL & TIE_ID_MASK) * (TIE_MUL_INV & TIE_ID_MASK)) & TIE_ID_MASK) == 1, "inverse of the tie multiplier mod 2^24");
constexpr uint32_t tie_xs12(uint32_t h) { return h ^ (h >> 12); }
static_assert(tie_xs12(tie_xs12(0xABCDEFu)) == 0xABCDEFu && tie_xs12(tie_xs12(0xFFFFFFu)) == 0xFFFFFFu && tie_xs12(tie_xs12(0x800001u)) == 0x800001u,
              "the 12-bit xor-shift is its own inverse on 24 bits");
DA_HD uint32_t tie_mix24(uint32_t id0, uint64_t seed) {
    uint32_t h = id0 ^ ((uint32_t)seed & TIE_ID_MASK);
    h = (h * (uint32_t)(TIE_MUL & TIE_ID_MASK)) & TIE_ID_MASK;
    h ^= h >> 12;
    return h ^ ((uint32_t)(seed >> 24) & TIE_ID_MASK);
}
DA_HD uint32_t tie_unmix24(uint32_t h, uint64_t seed) {
    h ^= (uint32_t)(seed >> 24) & TIE_ID_MASK;
    h ^= h >> 12;
    h = (h * (uint32_t)(TIE_MUL_INV & TIE_ID_MASK)) & TIE_ID_MASK;
    return h ^ ((uint32_t)seed & TIE_ID_MASK);
}
DA_HD uint64_t tie_word_newest(uint32_t id0, uint32_t id1, int idx, uint64_t seed) {
    return ((uint64_t)id1 << 31) | ((uint64_t)tie_mix24(id0, seed) << 7) | (uint64_t)tie_block_pos((uint32_t)idx, seed);
}
// Both seeded orders as ONE expression of the 48 bits (id1 << 24 | id0), for code that learns the order at run time (the SEEDED kernels of the
// engine): the random order mixes all 48 bits (mask 2^48 - 1, xor-shift 24, the seed's bits 16 .. 63 on top), the newest-first order the low 24
// (mask 2^24 - 1, xor-shift 12, the seed's bits 24 .. 47) and passes id1 through.
DA_HD uint64_t tie_pair_mix(uint64_t pair, uint64_t seed, uint32_t order) {
    const uint64_t m = order == TIE_ORDER_NEWEST ? (uint64_t)TIE_ID_MASK : TIE_PAIR_MASK;
    const int s = order == TIE_ORDER_NEWEST ? 12 : 24;
    uint64_t h = ((pair ^ seed) * TIE_MUL) & m;
    h ^= h >> s;
    h ^= (order == TIE_ORDER_NEWEST ? seed >> 24 : seed >> 16) & m;
    return (pair & ~m) | h;
}
DA_HD uint64_t tie_pair_unmix(uint64_t w, uint64_t seed, uint32_t order) {
    const uint64_t m = order == TIE_ORDER_NEWEST ? (uint64_t)TIE_ID_MASK : TIE_PAIR_MASK;
    const int s = order == TIE_ORDER_NEWEST ? 12 : 24;
    uint64_t h = (w ^ (order == TIE_ORDER_NEWEST ? seed >> 24 : seed >> 16)) & m;
    h ^= h >> s;
    h = ((h * TIE_MUL_INV) ^ seed) & m;
    return (w & ~m) | h;
}
// seed != 0 wanted, as tie_word_seeded
DA_HD uint64_t tie_word_seeded(uint32_t id0, uint32_t id1, int idx, uint64_t seed, uint32_t order) {
    return (tie_pair_mix(((uint64_t)id1 << 24) | (uint64_t)id0, seed, order) << 7) | (uint64_t)tie_block_pos((uint32_t)idx, seed);
}
// any seed, either order (seed 0: the reference's word under both)
DA_HD uint64_t tie_word(uint32_t id0, uint32_t id1, int idx, uint64_t seed, uint32_t order) {
    return seed ? tie_word_seeded(id0, id1, idx, seed, order) : tie_word(id0, id1, idx);
}
DA_HD void tie_word_rows(uint64_t tie, uint64_t seed, uint32_t order, uint32_t &id0, uint32_t &id1) {
    const uint64_t h = seed ? tie_pair_unmix(tie >> 7, seed, order) : tie >> 7;
    id0 = (uint32_t)(h & TIE_ID_MASK);
    id1 = (uint32_t)(h >> 24);
}

// ------------------------------------------------------------------------------------ qint / latency
// qint_add(q0, q1, shift, false, sub) (state_opr.cc:8-29); all operations exact or single-rounded IEEE
DA_HD void qint_add_pair(const RowInfo &a, const RowInfo &b, int shift, int sub, float &lo, float &hi, float &step) {
    float lo1 = b.lo, hi1 = b.hi, st1 = b.step;
    if (sub) {
        float t = lo1;
        lo1 = -hi1;
        hi1 = -t;
    }
    float s = pow2f(shift);
#if defined(__HIP_DEVICE_COMPILE__)
    lo1 = __fmul_rn(lo1, s);
    hi1 = __fmul_rn(hi1, s);
    st1 = __fmul_rn(st1, s);
    lo = __fadd_rn(a.lo, lo1);
    hi = __fadd_rn(a.hi, hi1);
#else
    lo1 = lo1 * s;
    hi1 = hi1 * s;
    st1 = st1 * s;
    lo = a.lo + lo1;
    hi = a.hi + hi1;
#endif
    step = a.step < st1 ? a.step : st1;  // std::min(step0, step1)
}

// Host-measured description of glibc's log2f near powers of two: ceil(log2f(x)) for x = 2^e * (1 + t*2^-23)
// equals e (not e+1) iff t <= tie[e + 150].  Filled by the host at library start-up from the local libm, so the
// device latency model reproduces std::ceil(std::log2(float)) of this very machine bit for bit.
struct Log2Table {
    uint8_t tie[280];
};

// std::ceil(std::log2(x)) for float x >= 0 (cost_add, state_opr.cc:58-62)
DA_HD float ceil_log2f_emul(float x, const Log2Table &tab, int &domain_err) {
    uint32_t b = f2u(x);
    int e = (int)((b >> 23) & 0xFF);
    uint32_t m = b & 0x7FFFFFu;
    if (x != x) return x;
    if (x == 0.0f) return -__builtin_inff();
    if (e == 255) return __builtin_inff();
    if (e == 0) {  // subnormal bounds never occur for fixed-point intervals
        domain_err = 1;
        return 0.0f;
    }
    int ee = e - 127;
    if (m == 0 || m <= tab.tie[ee + 150]) return (float)ee;
    return (float)(ee + 1);
}
// -std::log2(step) (state_opr.cc:57).  A power of two is read off the exponent.  Any other step gets the HOST libm's value from a
// table: every row's step is an input step times a power of two (qint_add keeps min(step0, step1 * 2^shift)), so only the
// mantissas of the input steps ever occur; for each of them the host tabulates -log2f(mantissa * 2^(e - 127)) for all 254
// normal exponents with its own std::log2 -- exact by construction, no libm re-implementation on the device.  (One table row per
// distinct mantissa, as many as the inputs have: the look-up is a linear search, and matrices with more than a handful of
// different odd step mantissas do not come out of the tracer.)
struct StepLog2 {
    int n;                 // distinct non-power-of-two step mantissas of the chain's inputs
    const uint32_t *mant;  // [n] their 23 mantissa bits
    const float *tab;      // [n][256] -log2f of (mantissa, biased exponent)
};
DA_HD float neg_log2f_step(float st, const StepLog2 &sl, int &domain_err) {
    uint32_t b = f2u(st);
    int e = (int)((b >> 23) & 0xFF);
    if (st != st) return st;
    if (st == 0.0f) return __builtin_inff();
    if (e == 255 && (b & 0x7FFFFFu) == 0) return (b >> 31) ? st : -__builtin_inff();
    if ((b >> 31) || e == 0 || e == 255) {
        domain_err = 1;
        return 0.0f;
    }
    const uint32_t m = b & 0x7FFFFFu;
    if (m == 0) return -(float)(e - 127);
    for (int i = 0; i < sl.n; ++i)
        if (sl.mant[i] == m) return sl.tab[i * 256 + e];
    domain_err = 1;
    return 0.0f;
}
// latency increment of cost_add (state_opr.cc:31-67); the cost itself is recomputed on the host
DA_HD float adder_dlat(const RowInfo &a, const RowInfo &b, int shift, int sub, int adder_size, int carry_size,
                       const Log2Table &tab, const StepLog2 &sl, int &domain_err) {
    if (adder_size < 0 && carry_size < 0) return 1.0f;
    if (carry_size < 0) carry_size = 65535;
    float lo0 = a.lo, hi0 = a.hi, st0 = a.step, lo1 = b.lo, hi1 = b.hi, st1 = b.step;
    if (sub) {
        float t = lo1;
        lo1 = hi1;
        hi1 = t;
    }
    float sf = pow2f(shift);
#if defined(__HIP_DEVICE_COMPILE__)
    lo1 = __fmul_rn(lo1, sf);
    hi1 = __fmul_rn(hi1, sf);
    st1 = __fmul_rn(st1, sf);
    hi0 = __fadd_rn(hi0, st0);
    hi1 = __fadd_rn(hi1, st1);
#else
    lo1 = lo1 * sf;
    hi1 = hi1 * sf;
    st1 = st1 * sf;
    hi0 = hi0 + st0;
    hi1 = hi1 + st1;
#endif
    float f = neg_log2f_step(st0 > st1 ? st0 : (st1 > st0 ? st1 : st0), sl, domain_err);
    float m = __builtin_fabsf(lo0);
    float t1 = __builtin_fabsf(lo1), t2 = __builtin_fabsf(hi0), t3 = __builtin_fabsf(hi1);
    m = m < t1 ? t1 : m;
    m = m < t2 ? t2 : m;
    m = m < t3 ? t3 : m;
    float i = ceil_log2f_emul(m, tab, domain_err);
    int k = (a.lo < 0 || b.lo < 0) ? 1 : 0;
#if defined(__HIP_DEVICE_COMPILE__)
    float n_accum = __fadd_rn(__fadd_rn((float)k, i), f);
    return ceilf(__fdiv_rn(n_accum, (float)carry_size));
#else
    float n_accum = (float)k + i;
    n_accum = n_accum + f;
    float q = n_accum / (float)carry_size;
    return __builtin_ceilf(q);
#endif
}

}  // namespace da
