// dais_exec.h -- a chain of DAIS programs compiled once into one statement list over one slot-compacted register file: the data
// behind da_dais_compile (include/da4ml_hip.h).  Built on the host (dais_gpu.hip: build_chain), run by the device kernel
// k_dais_exec and, sample by sample, by the host-scalar mode of da_dais_exec_run (dais_interp.cc), which is how the CPU tests pin
// the chain's slot logic.
#pragma once
#include <cstdint>
#include <vector>

#include "dais_core.h"

namespace dais {

// where a K_INPUT statement takes its raw value from
constexpr int32_t SRC_EXTERNAL = -1;  // input s.a of the chain's first program
constexpr int32_t SRC_ABSENT = -2;    // an absent output (index -1) of the producing stage: 0.0

struct ChainStep {
    Step s;                    // operand fields a/b/c hold SLOTS (K_INPUT with SRC_EXTERNAL: a = input number)
    int32_t dst;               // slot written
    int32_t tab_off, tab_len;  // K_LUT: the table inside the concatenated table array
    int32_t src;               // K_INPUT: SRC_EXTERNAL, SRC_ABSENT or the slot of the producing stage's output value
    int32_t src_neg;           // ... its negation flag
    int32_t pad;
    double src_scale;          // ... its output scale
};

struct ChainOut {
    int32_t slot;  // -1: absent output
    int32_t neg;
    double scale;
};

struct Chain {
    int n_stages = 0;
    int64_t n_in = 0, n_out = 0, n_slots = 1;
    bool has_tables = false;
    std::vector<ChainStep> steps;  // the statements of all stages, in order
    std::vector<ChainOut> outs;    // of the last stage
    std::vector<int32_t> tables;   // all tables of all stages, concatenated
};

// One slot assignment over the whole chain.  An input statement of stage s+1 is a read of the value behind output a of stage s,
// so that value keeps its slot until its last such reader -- and, like every output, at least to the end of its own stage.
// Throws "stage s has n outputs, stage s+1 expects m inputs".
Chain build_chain(const std::vector<Program> &stages);

}  // namespace dais

// ---- device side of a compiled chain (dais_gpu.hip) ----------------------------------------------------------------------------
struct DaisDevExec;
// uploads steps, outputs and tables to the current device; nullptr without a device
DaisDevExec *dais_dev_create(const dais::Chain &c);
void dais_dev_free(DaisDevExec *d);
// scratch3 = {address of the register-file scratch, its bytes, device allocations made by runs so far}
void dais_dev_scratch(const DaisDevExec *d, int64_t *scratch3);
// in / out: host pointers staged tile by tile (resident == false, synchronous) or device pointers used in place (resident == true:
// queued on `stream`, or on the handle's stream and synchronised when stream is null)
void dais_dev_run(DaisDevExec *d, const dais::Chain &c, const void *in, int in_type, int64_t in_stride, int64_t n_samples, void *out, int out_type,
                  int64_t out_stride, bool resident, void *stream);
