// C entry points around the tie words of da4ml_amd/csrc/cmvm_core.h that take a tie order, for tests/test_tie_newest.py (and, as a second
// translation unit, for the patched restatement of tests/golden/make_newest_golden.py).  TEST INFRASTRUCTURE.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "cmvm_core.h"

extern "C" {
// the five-argument word (any seed, either order) of n entries
void tn_words(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, long long n, uint64_t seed, uint32_t order, uint64_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::tie_word(id0[i], id1[i], idx[i], seed, order);
}
// the word as the specification spells it, from the named pieces: id1 << 31 | mix24(id0) << 7 | tie_block_pos(idx)
void tn_words_newest(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, long long n, uint64_t seed, uint64_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::tie_word_newest(id0[i], id1[i], idx[i], seed);
}
// the four-argument word as it was before there was an order (any seed)
void tn_words4(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, long long n, uint64_t seed, uint64_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::tie_word(id0[i], id1[i], idx[i], seed);
}
void tn_decode(const uint64_t *w, long long n, uint64_t seed, uint32_t order, uint32_t *id0, uint32_t *id1, int32_t *idx) {
    for (long long i = 0; i < n; ++i) {
        da::tie_word_rows(w[i], seed, order, id0[i], id1[i]);
        idx[i] = da::tie_word_idx(w[i], seed);
    }
}
void tn_mix24(const uint32_t *id0, long long n, uint64_t seed, uint32_t *mixed, uint32_t *back) {
    for (long long i = 0; i < n; ++i) {
        mixed[i] = da::tie_mix24(id0[i], seed);
        back[i] = da::tie_unmix24(mixed[i], seed);
    }
}
// all words of id0, id1 < n_ids and idx < n_idx: out[0] = how many, out[1] = how many distinct, out[2] = the largest,
// out[3] = entries whose rows / index do not come back from the word, out[4] = entries whose word is not the specification's
void tn_exhaustive(uint32_t n_ids, int n_idx, uint64_t seed, uint32_t order, uint64_t *out) {
    std::vector<uint64_t> w;
    w.reserve((size_t)n_ids * n_ids * n_idx);
    uint64_t bad = 0, off = 0;
    for (uint32_t a = 0; a < n_ids; ++a)
        for (uint32_t b = 0; b < n_ids; ++b)
            for (int k = 0; k < n_idx; ++k) {
                const uint64_t t = da::tie_word(a, b, k, seed, order);
                uint32_t ra, rb;
                da::tie_word_rows(t, seed, order, ra, rb);
                bad += ra != a || rb != b || da::tie_word_idx(t, seed) != k;
                const uint64_t spec = !seed ? da::tie_word(a, b, k) : order == da::TIE_ORDER_NEWEST ? da::tie_word_newest(a, b, k, seed) : da::tie_word_seeded(a, b, k, seed);
                off += t != spec;
                w.push_back(t);
            }
    out[0] = w.size();
    std::sort(w.begin(), w.end());
    out[2] = w.empty() ? 0 : w.back();
    out[1] = (uint64_t)(std::unique(w.begin(), w.end()) - w.begin());
    out[3] = bad;
    out[4] = off;
}
}
