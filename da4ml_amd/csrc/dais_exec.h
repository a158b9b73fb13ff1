// dais_exec.h -- a chain of DAIS programs compiled once into one statement list over one slot-compacted register file: the data
// behind da_dais_compile (include/da4ml_hip.h).  Built on the host (dais_gpu.hip: build_chain), run by the device kernel
// k_dais_exec and, sample by sample, by the host-scalar mode of da_dais_exec_run (dais_interp.cc), which is how the CPU tests pin
// the chain's slot logic.  The same statements a second time in dependency-level order with a slot assignment of their own
// (LevelSchedule): kernel k_dais_exec_level runs the statements of a level side by side.
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

// The statements of a chain by dependency level.  Level of a statement: 0 when it reads no value (K_CONST, K_INPUT from outside or of
// an absent output), otherwise 1 + the largest level among the values it reads; an inner stage's K_INPUT reads the value behind the
// producing stage's output like any operand.  The statements of a level run concurrently and in no particular order, so the slot of
// a value whose last reader is in level L is handed out again in level L + 1 at the earliest: slots are released only when a level
// is complete, and a level takes only slots that earlier levels released.  The outputs of the last stage keep theirs to the end.
struct LevelSchedule {
    int64_t n_slots = 1, widest = 0;
    std::vector<ChainStep> steps;    // by (level, kind, program order); operand fields, dst and src hold the slots of THIS schedule
    std::vector<int32_t> level_off;  // [levels + 1] into steps
    std::vector<ChainOut> outs;      // of the last stage, over this schedule's slots
    std::vector<int32_t> value;      // program-order number (index into Chain::steps) of every statement of `steps`
    int64_t n_levels() const { return (int64_t)level_off.size() - 1; }
};

struct Chain {
    int n_stages = 0;
    int64_t n_in = 0, n_out = 0, n_slots = 1;
    bool has_tables = false;
    std::vector<ChainStep> steps;  // the statements of all stages, in order
    std::vector<ChainOut> outs;    // of the last stage
    std::vector<int32_t> tables;   // all tables of all stages, concatenated
    LevelSchedule lv;              // the same statements by level (tables shared)
};

// One slot assignment over the whole chain.  An input statement of stage s+1 is a read of the value behind output a of stage s,
// so that value keeps its slot until its last such reader -- and, like every output, at least to the end of its own stage.
// Throws "stage s has n outputs, stage s+1 expects m inputs".  Builds both orders: the program-order list with its slots, and Chain::lv.
Chain build_chain(const std::vector<Program> &stages);

// execution modes of a compiled chain (DA_DAIS_MODE_* of include/da4ml_hip.h)
constexpr int MODE_AUTO = 0, MODE_SAMPLE = 1, MODE_LEVEL = 2;
// What AUTO runs on the device for `n_samples` rows of a chain of `n_steps` statements in `n_levels` levels (the rule and its
// measurement: DESIGN.md section 10a)
int auto_mode(int64_t n_steps, int64_t n_levels, int64_t n_samples);

}  // namespace dais

// ---- device side of a compiled chain (dais_gpu.hip) ----------------------------------------------------------------------------
struct DaisDevExec;
// uploads steps, outputs and tables to the current device; nullptr without a device
DaisDevExec *dais_dev_create(const dais::Chain &c);
void dais_dev_free(DaisDevExec *d);
// scratch3 = {address of the register-file scratch, its bytes, device allocations made by runs so far}
void dais_dev_scratch(const DaisDevExec *d, int64_t *scratch3);
// last2 = {what the last device run was: -1 none yet, 0 sample, 1 level with the value file in LDS, 2 level with it in global memory;
// samples per tile of the last level run (0: none yet)}
void dais_dev_last(const DaisDevExec *d, int64_t *last2);
// in / out: host pointers staged tile by tile (resident == false, synchronous) or device pointers used in place (resident == true:
// queued on `stream`, or on the handle's stream and synchronised when stream is null); mode: MODE_SAMPLE or MODE_LEVEL
void dais_dev_run(DaisDevExec *d, const dais::Chain &c, const void *in, int in_type, int64_t in_stride, int64_t n_samples, void *out, int out_type,
                  int64_t out_stride, bool resident, void *stream, int mode);
