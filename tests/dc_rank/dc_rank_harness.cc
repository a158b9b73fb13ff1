// C entry points around entry_rank of da4ml_amd/csrc/cmvm_core.h for tests/test_dc_rank.py.  TEST INFRASTRUCTURE.
#include <cstdint>

#include "cmvm_core.h"

extern "C" {
// the enum value of a method by its name's position in (mc, mc-dc, mc-pdc, wmc, wmc-dc, wmc-pdc, dummy)
int dc_method_id(int i) {
    static const int ids[7] = {da::M_MC, da::M_MC_DC, da::M_MC_PDC, da::M_WMC, da::M_WMC_DC, da::M_WMC_PDC, da::M_DUMMY};
    return ids[i];
}
float dc_weight_mc() { return da::DC_WEIGHT_MC; }
float dc_weight_wmc() { return da::DC_WEIGHT_WMC; }
float dc_weight_of(int method) { return da::dc_weight_default(method); }
// the four-argument rank (every method with its own constant) and the five-argument one of n entries
void dc_ranks4(const uint32_t *count, const int32_t *ov, const float *dl, const int32_t *method, long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::entry_rank(count[i], ov[i], dl[i], method[i]);
}
void dc_ranks5(const uint32_t *count, const int32_t *ov, const float *dl, const int32_t *method, const float *w, long long n, uint32_t *out) {
    for (long long i = 0; i < n; ++i) out[i] = da::entry_rank(count[i], ov[i], dl[i], method[i], w[i]);
}
}
