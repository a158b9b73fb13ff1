// C entry point around da::table_geometry (da4ml_amd/csrc/cmvm_geometry.h) for tests/test_table_geometry.py.  TEST INFRASTRUCTURE.
#include "cmvm_geometry.h"

extern "C" {
// out[0..3]: C, gs_log2, n_groups, rcap
void geo_table(int n_in, int n_out, int method, long long prep_pairs, long long prep_digits, double table_scale, double row_scale, int max_groups,
               long long *out) {
    da::ChainJob job;
    job.n_in = n_in;
    job.n_out = n_out;
    job.method = method;
    const da::TableGeometry g = da::table_geometry(job, prep_pairs, prep_digits, table_scale, row_scale, max_groups);
    out[0] = g.C;
    out[1] = g.gs_log2;
    out[2] = g.n_groups;
    out[3] = g.rcap;
}
}
