// C entry points around entry_rank_slack and slack_byte of da4ml_amd/csrc/cmvm_core.h for tests/test_slack_rank.py.  TEST INFRASTRUCTURE.
#include <cstdint>

#include "cmvm_core.h"

extern "C" {
// the enum value of a method by its name's position in (mc, mc-dc, mc-pdc, wmc, wmc-dc, wmc-pdc, dummy)
int slk_method_id(int i) {
    static const int ids[7] = {da::M_MC, da::M_MC_DC, da::M_MC_PDC, da::M_WMC, da::M_WMC_DC, da::M_WMC_PDC, da::M_DUMMY};
    return ids[i];
}
// entry_rank with a weight, and entry_rank_slack, of n entries
void slk_ranks_plain(const uint32_t *count, const int32_t *ov, const float *dl, const int32_t *method, const float *w, long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::entry_rank(count[i], ov[i], dl[i], method[i], w[i]);
}
void slk_ranks(const uint32_t *count, const int32_t *ov, const float *dl, const int32_t *method, const float *w, const uint32_t *slack, const uint32_t *byte,
               long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::entry_rank_slack(count[i], ov[i], dl[i], method[i], w[i], slack[i], byte[i]);
}
void slk_discount(const uint32_t *base, const uint32_t *slack, const uint32_t *byte, long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::slack_discount(base[i], slack[i], byte[i]);
}
// slack_byte of n (id0, id1, idx) under one seed; and the same through the per-block word, as the kernels form it
void slk_bytes(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, uint64_t seed, long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::slack_byte(id0[i], id1[i], idx[i], seed);
}
void slk_bytes_by_word(const uint32_t *id0, const uint32_t *id1, const int32_t *idx, uint64_t seed, long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::slack_word_byte(da::slack_pair_word(id0[i], id1[i], seed), (uint32_t)idx[i]);
}
}
