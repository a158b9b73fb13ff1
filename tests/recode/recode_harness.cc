// C entry points around the digit recoding of da4ml_amd/csrc/cmvm_core.h, for tests/test_recode_digits.py.  TEST INFRASTRUCTURE.
#include "cmvm_core.h"

extern "C" {
// digit_masks of n values under one (mode, seed)
void rc_digit_masks(const int32_t *x, long long n, uint32_t mode, uint64_t seed, uint32_t *plus, uint32_t *minus) {
    for (long long i = 0; i < n; ++i) da::digit_masks(x[i], mode, seed, plus[i], minus[i]);
}
void rc_naf_masks(const int32_t *x, long long n, uint32_t *plus, uint32_t *minus) {
    for (long long i = 0; i < n; ++i) da::naf_masks(x[i], plus[i], minus[i]);
}
uint64_t rc_splitmix64(uint64_t x) { return da::splitmix64(x); }
void rc_widths(const int32_t *x, long long n, int32_t *naf_weight, int32_t *csd_width) {
    for (long long i = 0; i < n; ++i) {
        naf_weight[i] = da::naf_weight(x[i]);
        csd_width[i] = da::csd_width(x[i] < 0 ? (uint32_t)(-(int64_t)x[i]) : (uint32_t)x[i]);
    }
}
}
