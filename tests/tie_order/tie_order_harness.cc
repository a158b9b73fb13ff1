// C entry points around the tie words of da4ml_amd/csrc/cmvm_core.h for tests/test_tie_order.py.  TEST INFRASTRUCTURE.
#include <algorithm>
#include <cstddef>
#include <vector>

#include "cmvm_core.h"

extern "C" {
// the three-argument (reference) and the four-argument (seeded) word of n entries
void tie_words3(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, long long n, uint64_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::tie_word(id0[i], id1[i], idx[i]);
}
void tie_words4(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, long long n, uint64_t seed, uint64_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::tie_word(id0[i], id1[i], idx[i], seed);
}
// the rows and key index read back from a word
void tie_decode(const uint64_t *w, long long n, uint64_t seed, uint32_t *id0, uint32_t *id1, int32_t *idx) {
    for (long long i = 0; i < n; ++i) {
        da::tie_word_rows(w[i], seed, id0[i], id1[i]);
        idx[i] = da::tie_word_idx(w[i], seed);
    }
}
// all words of id0, id1 < n_ids and idx < n_idx: out[0] = how many, out[1] = how many distinct, out[2] = the largest,
// out[3] = entries whose rows / index do not come back from the word
void tie_exhaustive(uint32_t n_ids, int n_idx, uint64_t seed, uint64_t *out) {
    std::vector<uint64_t> w;
    w.reserve((size_t)n_ids * n_ids * n_idx);
    uint64_t bad = 0;
    for (uint32_t a = 0; a < n_ids; ++a)
        for (uint32_t b = 0; b < n_ids; ++b)
            for (int k = 0; k < n_idx; ++k) {
                const uint64_t t = da::tie_word(a, b, k, seed);
                uint32_t ra, rb;
                da::tie_word_rows(t, seed, ra, rb);
                bad += ra != a || rb != b || da::tie_word_idx(t, seed) != k;
                w.push_back(t);
            }
    out[0] = w.size();
    std::sort(w.begin(), w.end());
    out[2] = w.empty() ? 0 : w.back();
    out[1] = (uint64_t)(std::unique(w.begin(), w.end()) - w.begin());
    out[3] = bad;
}
uint32_t tie_block_position(uint32_t idx, uint64_t seed) { return da::tie_block_pos(idx, seed); }
uint32_t tie_seed_k7(uint64_t seed) { return da::tie_k7(seed); }
}
