// dais_gpu.hip -- device executor of DAIS programs for gfx950: the samples of CombLogic.predict are independent, so one
// thread runs one sample through the whole (sequential) program.
//
// Layout: the int64 register file is [slot][sample] in HBM, so the 64 lanes of a wavefront touch 512 consecutive bytes
// per register access (fully coalesced) and every step costs 8 B written + 8 B per operand read per sample -- the
// algorithmic traffic; the kernel is HBM/L2-bandwidth bound.  Registers are *slots*: a linear
// liveness scan on the host lets a step reuse the slot of a value whose last reader has passed, so the live working set
// per sample is the maximum number of simultaneously live values (hundreds for an adder graph of 10^4-10^5 steps), not
// n_ops -- small enough for a tile of 10^5-10^6 samples to stay L2/MALL resident between producer and consumer steps.
// The decoded steps are uniform across the grid: the compiler reads them with scalar loads, the switch is a uniform
// branch.  Per-value arithmetic is dais::eval of dais_core.h, the same code the host executor is tested with.
//
// A compiled executable (second half of the file) has a second kernel for small batches, k_dais_exec_level: a workgroup runs the
// statements of a dependency level side by side, so that a call lasts as long as the graph is deep, not as long as its list.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/da4ml_hip.h"

#include "dais_core.h"
#include "dais_exec.h"

namespace {

#define DAIS_HIP(expr)                                                                                                 \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess)                                                                                          \
            throw std::runtime_error(std::string("HIP error in DAIS executor: ") + hipGetErrorString(e_) + " (" #expr ")"); \
    } while (0)

struct DevStep {
    dais::Step s;              // operand fields a/b/c hold SLOTS here (K_INPUT: a = input number)
    int32_t dst;               // slot written
    int32_t tab_off, tab_len;  // K_LUT: the table inside the concatenated table array
    int32_t pad;
};

struct DevOut {
    int32_t slot;  // -1: absent output
    int32_t neg;
    double scale;
};

constexpr int TPB = 256;

// regs: [n_slots][tile]; x: [n][n_in]; y: [n][n_out] for the samples of this tile
__global__ __launch_bounds__(TPB) void k_dais_run(const DevStep *__restrict__ steps, int64_t n_ops, const DevOut *__restrict__ outs, int64_t n_in,
                                                  int64_t n_out, const int32_t *__restrict__ tables, const double *__restrict__ x,
                                                  double *__restrict__ y, int64_t *__restrict__ regs, int64_t tile, int64_t n,
                                                  unsigned long long *__restrict__ lut_fault) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    int64_t *R = regs + t;
    const double *xs = x + t * n_in;
    for (int64_t i = 0; i < n_ops; ++i) {
        const DevStep &d = steps[i];  // uniform address: scalar loads
        const dais::Step &s = d.s;
        const int rd = dais::reads(s.kind);
        const int64_t a = (rd & 1) ? R[(int64_t)s.a * tile] : 0;
        const int64_t b = (rd & 2) ? R[(int64_t)s.b * tile] : 0;
        const int64_t c = (rd & 4) ? R[(int64_t)s.c * tile] : 0;
        int64_t v;
        if (s.kind == dais::K_LUT) {
            const int64_t idx = dais::lut_index(s, a);
            if (idx < 0 || idx >= d.tab_len) {
                // record the first offending index and keep going with 0; the host turns it into the reference's error
                atomicCAS(lut_fault, 0ull, (1ull << 63) | ((unsigned long long)(uint32_t)d.tab_len << 32) | (unsigned long long)(uint32_t)idx);
                v = 0;
            } else
                v = tables[d.tab_off + idx];
        } else
            v = dais::eval(s, a, b, c, s.kind == dais::K_INPUT ? xs[s.a] : 0.0);
        R[(int64_t)d.dst * tile] = v;
    }
    double *ys = y + t * n_out;
    for (int64_t j = 0; j < n_out; ++j) {
        const DevOut o = outs[j];
        if (o.slot < 0) {
            ys[j] = 0.0;
            continue;
        }
        const int64_t v = R[(int64_t)o.slot * tile];
        ys[j] = (double)(o.neg ? -v : v) * o.scale;
    }
}

template <class T> struct DevBuf {
    T *p = nullptr;
    explicit DevBuf(size_t n) { DAIS_HIP(hipMalloc((void **)&p, std::max<size_t>(n, 1) * sizeof(T))); }
    ~DevBuf() { (void)hipFree(p); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

}  // namespace

// Slot assignment: value i gets a slot when it is produced and gives it back after its last reader; a step may write
// the slot of an operand that dies in it (a thread reads its operands before it writes).  Outputs stay live to the end.
// Returns the number of slots; rewrites the operand fields of `steps` from value numbers to slots, fills slot_of.
// Also used by the host-side run of the device code path (da_dais_run_on with DA_DAIS_HOST_SCALAR, dais_interp.cc), which is
// how the CPU tests check the slot logic against the golden vectors.
int64_t dais_assign_slots(const dais::Program &g, std::vector<dais::Step> &steps, std::vector<int32_t> &dst, std::vector<int32_t> &slot_of) {
    const int64_t n = g.n_ops;
    std::vector<int64_t> last(n, -1);
    for (int64_t i = 0; i < n; ++i) {
        const dais::Step &s = g.steps[i];
        const int rd = dais::reads(s.kind);
        if (rd & 1) last[s.a] = i;
        if (rd & 2) last[s.b] = i;
        if (rd & 4) last[s.c] = i;
    }
    for (int32_t o : g.out_idx)
        if (o >= 0) last[o] = n;  // read by the output stage
    slot_of.assign(n, -1);
    dst.assign(n, -1);
    std::vector<int32_t> free_slots;
    int64_t n_slots = 0;
    steps = g.steps;
    for (int64_t i = 0; i < n; ++i) {
        dais::Step &s = steps[i];
        const int rd = dais::reads(s.kind);
        const int32_t ops[3] = {(rd & 1) ? s.a : -1, (rd & 2) ? s.b : -1, (rd & 4) ? s.c : -1};
        if (rd & 1) s.a = slot_of[ops[0]];
        if (rd & 2) s.b = slot_of[ops[1]];
        if (rd & 4) s.c = slot_of[ops[2]];
        for (int k = 0; k < 3; ++k) {  // operands whose last reader is this step release their slot (once per value)
            const int32_t v = ops[k];
            if (v < 0 || last[v] != i) continue;
            bool dup = false;
            for (int m = 0; m < k; ++m) dup |= ops[m] == v;
            if (!dup) free_slots.push_back(slot_of[v]);
        }
        int32_t slot;
        if (!free_slots.empty()) {
            slot = free_slots.back();
            free_slots.pop_back();
        } else
            slot = (int32_t)n_slots++;
        slot_of[i] = dst[i] = slot;
        if (last[i] < 0) free_slots.push_back(slot);  // never read: the slot is free again right away
    }
    return std::max<int64_t>(n_slots, 1);
}

void dais_run_gpu(const dais::Program &g, const double *inputs, int64_t n_samples, double *outputs) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)
        throw std::runtime_error("no HIP device: the DAIS device executor needs a GPU (the host executor does not)");
    std::vector<dais::Step> slot_steps;
    std::vector<int32_t> dst, slot_of;
    const int64_t n_slots = dais_assign_slots(g, slot_steps, dst, slot_of);
    std::vector<DevStep> steps((size_t)g.n_ops);
    std::vector<int32_t> tables, off;
    for (const auto &t : g.tables) {
        off.push_back((int32_t)tables.size());
        tables.insert(tables.end(), t.begin(), t.end());
    }
    for (int64_t i = 0; i < g.n_ops; ++i) {
        DevStep d{};
        d.s = slot_steps[i], d.dst = dst[i];
        if (d.s.kind == dais::K_LUT) d.tab_off = off[d.s.aux], d.tab_len = (int32_t)g.tables[d.s.aux].size();
        steps[i] = d;
    }
    std::vector<DevOut> outs((size_t)g.n_out);
    for (int64_t j = 0; j < g.n_out; ++j) outs[j] = DevOut{g.out_idx[j] < 0 ? -1 : slot_of[g.out_idx[j]], g.out_neg[j], g.out_scale[j]};

    // tile: as many samples as fit a register-file budget (1/4 of free memory, at most 2^22 samples), whole blocks
    size_t free_b = 0, total_b = 0;
    DAIS_HIP(hipMemGetInfo(&free_b, &total_b));
    const int64_t per_sample = n_slots * 8 + (g.n_in + g.n_out) * 8;
    int64_t tile = std::min<int64_t>({n_samples, (int64_t)1 << 22, std::max<int64_t>((int64_t)(free_b / 4) / per_sample, TPB)});
    if (const char *e = std::getenv("DA4ML_DAIS_TILE"))  // experiment knob: samples per launch (cache residency vs occupancy)
        tile = std::max<int64_t>(1, std::min<int64_t>(tile, std::atoll(e)));
    tile = (tile + TPB - 1) / TPB * TPB;

    DevBuf<DevStep> d_steps(steps.size());
    DevBuf<DevOut> d_outs(outs.size());
    DevBuf<int32_t> d_tab(tables.size());
    DevBuf<int64_t> d_regs((size_t)(n_slots * tile));
    DevBuf<double> d_x((size_t)(tile * g.n_in)), d_y((size_t)(tile * g.n_out));
    DevBuf<unsigned long long> d_fault(1);
    hipStream_t st;
    DAIS_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    struct StreamGuard {
        hipStream_t s;
        ~StreamGuard() { (void)hipStreamDestroy(s); }
    } guard{st};
    DAIS_HIP(hipMemcpyAsync(d_steps.p, steps.data(), steps.size() * sizeof(DevStep), hipMemcpyHostToDevice, st));
    DAIS_HIP(hipMemcpyAsync(d_outs.p, outs.data(), outs.size() * sizeof(DevOut), hipMemcpyHostToDevice, st));
    if (!tables.empty()) DAIS_HIP(hipMemcpyAsync(d_tab.p, tables.data(), tables.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    DAIS_HIP(hipMemsetAsync(d_fault.p, 0, sizeof(unsigned long long), st));
    for (int64_t s0 = 0; s0 < n_samples; s0 += tile) {
        const int64_t n = std::min(tile, n_samples - s0);
        DAIS_HIP(hipMemcpyAsync(d_x.p, inputs + s0 * g.n_in, (size_t)(n * g.n_in) * sizeof(double), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_dais_run, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, d_steps.p, g.n_ops, d_outs.p, g.n_in, g.n_out, d_tab.p,
                           d_x.p, d_y.p, d_regs.p, tile, n, d_fault.p);
        DAIS_HIP(hipGetLastError());
        if (g.n_out > 0)
            DAIS_HIP(hipMemcpyAsync(outputs + s0 * g.n_out, d_y.p, (size_t)(n * g.n_out) * sizeof(double), hipMemcpyDeviceToHost, st));
    }
    unsigned long long fault = 0;
    DAIS_HIP(hipMemcpyAsync(&fault, d_fault.p, sizeof fault, hipMemcpyDeviceToHost, st));
    DAIS_HIP(hipStreamSynchronize(st));
    if (fault) {
        const int64_t idx = (int64_t)(int32_t)(uint32_t)(fault & 0xFFFFFFFFull);
        throw std::runtime_error("Logic lookup index out of bounds: index=" + std::to_string(idx) +
                                 ", table_size=" + std::to_string((fault >> 32) & 0x7FFFFFFFull));
    }
}

// ================================================================================================================================
// Compiled executables (da_dais_compile, include/da4ml_hip.h): a chain of programs as ONE statement list over one register file,
// uploaded once; k_dais_exec runs all stages of a sample in one thread and one launch.
// ================================================================================================================================

namespace {

// Chain::lv (dais_exec.h) from the chain's statements (c.steps: everything but the slots), the values every statement reads and the
// values behind the outputs of the last stage (-1: absent)
void build_levels(dais::Chain &c, const std::vector<std::array<int64_t, 3>> &opnd, const std::vector<int64_t> &out_value) {
    using namespace dais;
    const int64_t total = (int64_t)c.steps.size();
    LevelSchedule &lv = c.lv;
    std::vector<int32_t> level((size_t)total, 0), dies((size_t)total, -1);  // dies: the level of a value's last reader
    int32_t n_levels = 0;
    for (int64_t v = 0; v < total; ++v) {  // (a statement's operands precede it: causality inside a stage, the stage order across)
        for (int64_t r : opnd[v])
            if (r >= 0) level[v] = std::max(level[v], level[r] + 1);
        for (int64_t r : opnd[v])
            if (r >= 0) dies[r] = std::max(dies[r], level[v]);
        n_levels = std::max(n_levels, level[v] + 1);
    }
    for (int64_t v = 0; v < total; ++v)
        if (dies[v] < 0) dies[v] = level[v];  // never read: gone with its own level
    for (int64_t o : out_value)
        if (o >= 0) dies[o] = n_levels;  // read by the output stage: never released
    lv.value.resize((size_t)total);
    for (int64_t v = 0; v < total; ++v) lv.value[v] = (int32_t)v;
    std::stable_sort(lv.value.begin(), lv.value.end(), [&](int32_t p, int32_t q) {
        return level[p] != level[q] ? level[p] < level[q] : c.steps[p].s.kind < c.steps[q].s.kind;  // by kind: fewer divergent lanes in dais::eval
    });
    lv.level_off.assign((size_t)n_levels + 1, 0);
    for (int64_t v = 0; v < total; ++v) ++lv.level_off[level[v] + 1];
    for (int32_t l = 0; l < n_levels; ++l) {
        lv.widest = std::max<int64_t>(lv.widest, lv.level_off[l + 1]);
        lv.level_off[l + 1] += lv.level_off[l];
    }
    std::vector<std::vector<int32_t>> dying((size_t)n_levels + 1);
    for (int64_t v = 0; v < total; ++v) dying[dies[v]].push_back((int32_t)v);
    std::vector<int32_t> slot_of((size_t)total, -1), free_slots;
    int64_t n_slots = 0;
    lv.steps.resize((size_t)total);
    for (int32_t l = 0; l < n_levels; ++l) {
        // free_slots holds what levels < l released; what dies in l comes back only when all of l has its slots
        for (int64_t i = lv.level_off[l]; i < lv.level_off[l + 1]; ++i) {
            const int32_t v = lv.value[i];
            ChainStep d = c.steps[v];
            const std::array<int64_t, 3> &r = opnd[v];
            if (r[0] >= 0) (d.s.kind == K_INPUT ? d.src : d.s.a) = slot_of[r[0]];
            if (r[1] >= 0) d.s.b = slot_of[r[1]];
            if (r[2] >= 0) d.s.c = slot_of[r[2]];
            if (!free_slots.empty()) {
                d.dst = free_slots.back();
                free_slots.pop_back();
            } else
                d.dst = (int32_t)n_slots++;
            slot_of[v] = d.dst;
            lv.steps[i] = d;
        }
        for (int32_t v : dying[l]) free_slots.push_back(slot_of[v]);
    }
    lv.n_slots = std::max<int64_t>(n_slots, 1);
    lv.outs = c.outs;
    for (size_t j = 0; j < lv.outs.size(); ++j) lv.outs[j].slot = out_value[j] < 0 ? -1 : slot_of[out_value[j]];
}

}  // namespace

dais::Chain dais::build_chain(const std::vector<Program> &stages) {
    const int S = (int)stages.size();
    if (S < 1) throw std::runtime_error("a DAIS executable needs at least one program");
    for (int s = 0; s + 1 < S; ++s)
        if (stages[s].n_out != stages[s + 1].n_in)
            throw std::runtime_error("stage " + std::to_string(s) + " has " + std::to_string(stages[s].n_out) + " outputs, stage " + std::to_string(s + 1) +
                                     " expects " + std::to_string(stages[s + 1].n_in) + " inputs");
    Chain c;
    c.n_stages = S, c.n_in = stages[0].n_in, c.n_out = stages[S - 1].n_out;
    std::vector<int64_t> base((size_t)S + 1, 0);  // value numbers of the chain: base[s] + statement index in stage s
    for (int s = 0; s < S; ++s) base[s + 1] = base[s] + stages[s].n_ops;
    const int64_t total = base[S];
    c.steps.resize((size_t)total);
    std::vector<std::array<int64_t, 3>> opnd((size_t)total);  // the values a statement reads (a boundary input: the producer's value in [0])
    std::vector<int64_t> last((size_t)total, -1);             // last reader of a value
    for (int s = 0; s < S; ++s) {
        const Program &g = stages[s];
        std::vector<int32_t> off;
        for (const auto &t : g.tables) {
            off.push_back((int32_t)c.tables.size());
            c.tables.insert(c.tables.end(), t.begin(), t.end());
        }
        c.has_tables |= !g.tables.empty();
        for (int64_t i = 0; i < g.n_ops; ++i) {
            const int64_t v = base[s] + i;
            ChainStep d{};
            d.s = g.steps[i], d.src = SRC_EXTERNAL;
            const int rd = reads(d.s.kind);
            opnd[v] = {(rd & 1) ? base[s] + d.s.a : -1, (rd & 2) ? base[s] + d.s.b : -1, (rd & 4) ? base[s] + d.s.c : -1};
            if (d.s.kind == K_INPUT && s > 0) {
                const Program &p = stages[s - 1];
                const int32_t o = p.out_idx[d.s.a];
                if (o < 0)
                    d.src = SRC_ABSENT;
                else
                    opnd[v][0] = base[s - 1] + o, d.src = 0, d.src_neg = p.out_neg[d.s.a], d.src_scale = p.out_scale[d.s.a];
            }
            if (d.s.kind == K_LUT) d.tab_off = off[d.s.aux], d.tab_len = (int32_t)g.tables[d.s.aux].size();
            for (int64_t r : opnd[v])
                if (r >= 0) last[r] = v;
            c.steps[v] = d;
        }
    }
    for (int32_t o : stages[S - 1].out_idx)
        if (o >= 0) last[base[S - 1] + o] = total;  // read by the output stage
    // an inner stage's output that the next stage never reads keeps its slot to the end of its own stage all the same
    std::vector<char> pinned((size_t)total, 0);
    for (int s = 0; s + 1 < S; ++s)
        for (int32_t o : stages[s].out_idx)
            if (o >= 0 && last[base[s] + o] < base[s + 1]) pinned[base[s] + o] = 1;

    std::vector<int32_t> slot_of((size_t)total, -1), free_slots;
    int64_t n_slots = 0;
    for (int s = 0; s < S; ++s) {
        if (s > 0)
            for (int32_t o : stages[s - 1].out_idx)
                if (o >= 0 && pinned[base[s - 1] + o]) free_slots.push_back(slot_of[base[s - 1] + o]), pinned[base[s - 1] + o] = 0;
        for (int64_t v = base[s]; v < base[s + 1]; ++v) {
            ChainStep &d = c.steps[v];
            const std::array<int64_t, 3> &r = opnd[v];
            if (r[0] >= 0) (d.s.kind == K_INPUT ? d.src : d.s.a) = slot_of[r[0]];
            if (r[1] >= 0) d.s.b = slot_of[r[1]];
            if (r[2] >= 0) d.s.c = slot_of[r[2]];
            for (int k = 0; k < 3; ++k) {  // operands whose last reader is this statement release their slot (once per value)
                if (r[k] < 0 || last[r[k]] != v || pinned[r[k]]) continue;
                bool dup = false;
                for (int m = 0; m < k; ++m) dup |= r[m] == r[k];
                if (!dup) free_slots.push_back(slot_of[r[k]]);
            }
            int32_t slot;
            if (!free_slots.empty()) {
                slot = free_slots.back();
                free_slots.pop_back();
            } else
                slot = (int32_t)n_slots++;
            slot_of[v] = d.dst = slot;
            if (last[v] < 0 && !pinned[v]) free_slots.push_back(slot);  // never read: the slot is free again right away
        }
    }
    c.n_slots = std::max<int64_t>(n_slots, 1);
    const Program &e = stages[S - 1];
    c.outs.resize((size_t)e.n_out);
    for (int64_t j = 0; j < e.n_out; ++j) c.outs[j] = ChainOut{e.out_idx[j] < 0 ? -1 : slot_of[base[S - 1] + e.out_idx[j]], e.out_neg[j], e.out_scale[j]};
    std::vector<int64_t> out_value((size_t)e.n_out);
    for (int64_t j = 0; j < e.n_out; ++j) out_value[j] = e.out_idx[j] < 0 ? -1 : base[S - 1] + e.out_idx[j];
    build_levels(c, opnd, out_value);
    return c;
}

namespace {

// One thread per sample, all stages of the chain.  x: [n][x_stride] of In, y: [n][y_stride] of Out (strides in elements).
// Register file [slot][sample] in HBM at regs, `pitch` samples per slot (the tile): the 64 lanes of a wavefront touch 512 consecutive
// bytes per access.  (A register file in the block's LDS was built and left out: DESIGN.md section 9.)
template <class In, class Out>
__global__ __launch_bounds__(TPB) void k_dais_exec(const dais::ChainStep *__restrict__ steps, int64_t n_steps, const dais::ChainOut *__restrict__ outs,
                                                   int64_t n_out, const int32_t *__restrict__ tables, const In *__restrict__ x, int64_t x_stride,
                                                   Out *__restrict__ y, int64_t y_stride, int64_t *__restrict__ regs, int64_t pitch, int64_t n,
                                                   unsigned long long *__restrict__ lut_fault) {
    const int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (t >= n) return;
    int64_t *R = regs + t;
    const int64_t P = pitch;
    const In *xs = x + t * x_stride;
    for (int64_t i = 0; i < n_steps; ++i) {
        const dais::ChainStep &d = steps[i];  // uniform address: scalar loads
        const dais::Step &s = d.s;
        const int rd = dais::reads(s.kind);
        const int64_t a = (rd & 1) ? R[(int64_t)s.a * P] : 0;
        const int64_t b = (rd & 2) ? R[(int64_t)s.b * P] : 0;
        const int64_t c = (rd & 4) ? R[(int64_t)s.c * P] : 0;
        int64_t v;
        if (s.kind == dais::K_LUT) {
            const int64_t idx = dais::lut_index(s, a);
            if (idx < 0 || idx >= d.tab_len) {
                // record the first offending index and keep going with 0; the host turns it into the reference's error
                atomicCAS(lut_fault, 0ull, (1ull << 63) | ((unsigned long long)(uint32_t)d.tab_len << 32) | (unsigned long long)(uint32_t)idx);
                v = 0;
            } else
                v = tables[d.tab_off + idx];
        } else {
            double xin = 0.0;  // K_INPUT: an input of the chain, or the producing stage's output straight from the register file
            if (s.kind == dais::K_INPUT) {
                if (d.src == dais::SRC_EXTERNAL)
                    xin = (double)xs[s.a];
                else if (d.src >= 0)
                    xin = dais::out_value(R[(int64_t)d.src * P], d.src_neg, d.src_scale);
            }
            v = dais::eval(s, a, b, c, xin);
        }
        R[(int64_t)d.dst * P] = v;
    }
    Out *ys = y + t * y_stride;
    for (int64_t j = 0; j < n_out; ++j) {
        const dais::ChainOut o = outs[j];
        ys[j] = o.slot < 0 ? (Out)0.0 : (Out)dais::out_value(R[(int64_t)o.slot * P], o.neg, o.scale);
    }
}

// The level-parallel executor: a workgroup runs a TILE of S = 1 << log2s samples through the statements of the level schedule
// (dais_exec.h: LevelSchedule), the lanes of the block over (statement of the current level, sample of the tile), one block barrier
// between levels.  The duration of a call no longer grows with the length of the statement list but with its depth -- the graphs
// of a solve are some ten levels deep and thousands of statements wide.  Value file [slot][S] of int64: FILE_IN_LDS in the block's
// dynamic LDS, otherwise in the block's part of a scratch in global memory, `file` = [block][slot][S], which only the wavefronts
// of this one workgroup exchange: __syncthreads() is a workgroup-scope release/acquire for global memory too, and the waves of a
// workgroup share one CU and its vector L1 (the property the many-column carve of k_iter_select2 rests on).
// The grid is persistent: a block loops over tiles.  Every value is computed by the code of k_dais_exec above.
constexpr int LV_TPB = 1024;    // largest (and default) block
constexpr int LV_S_MAX = 16;    // samples per tile, at most
constexpr int LV_WAVES_CU = 32; // wavefronts a CU keeps resident
template <class In, class Out, bool FILE_IN_LDS>
__global__ __launch_bounds__(LV_TPB) void k_dais_exec_level(const dais::ChainStep *__restrict__ steps, const int32_t *__restrict__ level_off, int n_levels,
                                                            const dais::ChainOut *__restrict__ outs, int n_out, const int32_t *__restrict__ tables,
                                                            const In *__restrict__ x, int64_t x_stride, Out *__restrict__ y, int64_t y_stride, int64_t *file,
                                                            int64_t n_slots, int log2s, int64_t n, int64_t n_tiles, unsigned long long *__restrict__ lut_fault) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int S = 1 << log2s;
    int64_t *R = FILE_IN_LDS ? reinterpret_cast<int64_t *>(smem) : file + ((int64_t)blockIdx.x * n_slots << log2s);
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t s0 = tile << log2s;
        const int live = n - s0 < S ? (int)(n - s0) : S;  // samples of this tile
        for (int l = 0; l < n_levels; ++l) {
            const int lo = level_off[l], work = (level_off[l + 1] - lo) << log2s;
            for (int w = (int)threadIdx.x; w < work; w += (int)blockDim.x) {
                const int k = w & (S - 1);
                if (k >= live) continue;
                const dais::ChainStep &d = steps[lo + (w >> log2s)];
                const dais::Step &s = d.s;
                const int rd = dais::reads(s.kind);
                const int64_t a = (rd & 1) ? R[(s.a << log2s) + k] : 0;
                const int64_t b = (rd & 2) ? R[(s.b << log2s) + k] : 0;
                const int64_t c = (rd & 4) ? R[(s.c << log2s) + k] : 0;
                int64_t v;
                if (s.kind == dais::K_LUT) {
                    const int64_t idx = dais::lut_index(s, a);
                    if (idx < 0 || idx >= d.tab_len) {
                        // as k_dais_exec: record the first offending index and keep going with 0
                        atomicCAS(lut_fault, 0ull, (1ull << 63) | ((unsigned long long)(uint32_t)d.tab_len << 32) | (unsigned long long)(uint32_t)idx);
                        v = 0;
                    } else
                        v = tables[d.tab_off + idx];
                } else {
                    double xin = 0.0;
                    if (s.kind == dais::K_INPUT) {
                        if (d.src == dais::SRC_EXTERNAL)
                            xin = (double)x[(s0 + k) * x_stride + s.a];
                        else if (d.src >= 0)
                            xin = dais::out_value(R[(d.src << log2s) + k], d.src_neg, d.src_scale);
                    }
                    v = dais::eval(s, a, b, c, xin);
                }
                R[(d.dst << log2s) + k] = v;
            }
            __syncthreads();  // the values of level l are there for level l + 1 (and for the outputs)
        }
        const int n_y = n_out * live;
        for (int w = (int)threadIdx.x; w < n_y; w += (int)blockDim.x) {  // consecutive lanes, consecutive elements of a row
            const int k = w / n_out, j = w - k * n_out;
            const dais::ChainOut o = outs[j];
            y[(s0 + k) * y_stride + j] = o.slot < 0 ? (Out)0.0 : (Out)dais::out_value(R[(o.slot << log2s) + k], o.neg, o.scale);
        }
        __syncthreads();  // the next tile's first level writes slots the outputs were read from
    }
}

// grow-only device allocation owned by a handle
struct Scratch {
    void *p = nullptr;
    size_t bytes = 0;
    // true when it had to allocate
    bool need(size_t want) {
        if (want <= bytes) return false;
        if (p) DAIS_HIP(hipFree(p));
        p = nullptr, bytes = 0;
        DAIS_HIP(hipMalloc(&p, want));
        bytes = want;
        return true;
    }
    ~Scratch() { (void)hipFree(p); }
};

size_t elem_size(int type) { return type == DA_DAIS_F32 ? sizeof(float) : sizeof(double); }

}  // namespace

struct DaisDevExec {
    dais::ChainStep *steps = nullptr;
    dais::ChainOut *outs = nullptr;
    int32_t *tables = nullptr;
    unsigned long long *fault = nullptr;
    hipStream_t stream = nullptr;
    int64_t tile_cap = 0;  // samples per launch the memory of the device allows (fixed at creation)
    Scratch regs, x, y;
    int64_t allocations = 0;
    // the level schedule: its statements, level offsets and outputs; the global value file [block][slot][S] of runs that need one
    dais::ChainStep *lv_steps = nullptr;
    int32_t *lv_off = nullptr;
    dais::ChainOut *lv_outs = nullptr;
    Scratch lv_file;
    int cus = 1;            // compute units of the device
    size_t lds_budget = 0;  // dynamic LDS a block of k_dais_exec_level may ask for
    int64_t free_bytes = 0; // free device memory at creation
    int last_run = -1, last_s = 0;  // dais_dev_last
};

void dais_dev_free(DaisDevExec *d) {
    if (!d) return;
    (void)hipFree(d->steps), (void)hipFree(d->outs), (void)hipFree(d->tables), (void)hipFree(d->fault);
    (void)hipFree(d->lv_steps), (void)hipFree(d->lv_off), (void)hipFree(d->lv_outs);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
}

namespace {

template <class In, class Out> void launch_exec(DaisDevExec *d, const dais::Chain &c, hipStream_t st, const void *x, int64_t x_stride, void *y, int64_t y_stride,
                                                int64_t pitch, int64_t n) {
    hipLaunchKernelGGL((k_dais_exec<In, Out>), dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, st, d->steps, (int64_t)c.steps.size(), d->outs, c.n_out,
                       d->tables, (const In *)x, x_stride, (Out *)y, y_stride, (int64_t *)d->regs.p, pitch, n, d->fault);
    DAIS_HIP(hipGetLastError());
}

void launch_typed(DaisDevExec *d, const dais::Chain &c, hipStream_t st, const void *x, int in_type, int64_t x_stride, void *y, int out_type, int64_t y_stride,
                  int64_t pitch, int64_t n) {
    if (in_type == DA_DAIS_F32)
        out_type == DA_DAIS_F32 ? launch_exec<float, float>(d, c, st, x, x_stride, y, y_stride, pitch, n)
                                : launch_exec<float, double>(d, c, st, x, x_stride, y, y_stride, pitch, n);
    else
        out_type == DA_DAIS_F32 ? launch_exec<double, float>(d, c, st, x, x_stride, y, y_stride, pitch, n)
                                : launch_exec<double, double>(d, c, st, x, x_stride, y, y_stride, pitch, n);
}

// geometry of a level-mode run of n samples
struct LevelGeom {
    bool lds = false;
    int log2s = 0, tpb = LV_TPB, grid = 1;
    size_t lds_bytes = 0;
};

int env_int(const char *name, int fallback) {
    const char *e = std::getenv(name);
    return e && *e ? std::atoi(e) : fallback;
}

// S: the largest power of two <= LV_S_MAX that still leaves every CU a tile (small batches spread over the device, large ones share
// a statement's record among S lanes), halved until the value file fits: the LDS budget, or 1 GB of global scratch and a quarter of
// the device's free memory.  DA4ML_DAIS_LEVEL_LDS=0 forces the global file, DA4ML_DAIS_LEVEL_S the tile (a power of two, where the file
// allows it), DA4ML_DAIS_LEVEL_TPB the block size: experiment and test knobs, read at every run; no result depends on them.
LevelGeom level_geometry(const DaisDevExec *d, const dais::Chain &c, int64_t n) {
    LevelGeom g;
    const int64_t slots = c.lv.n_slots;
    g.tpb = std::min(LV_TPB, std::max(64, env_int("DA4ML_DAIS_LEVEL_TPB", LV_TPB) / 64 * 64));
    int s = 1;
    if (const int forced = env_int("DA4ML_DAIS_LEVEL_S", 0); forced > 0)
        while (s * 2 <= std::min(forced, 64)) s *= 2;
    else
        while (s * 2 <= LV_S_MAX && n / (s * 2) >= d->cus) s *= 2;
    g.lds = env_int("DA4ML_DAIS_LEVEL_LDS", 1) != 0 && (size_t)slots * 8 <= d->lds_budget;
    const int per_cu_max = std::max(1, LV_WAVES_CU * 64 / g.tpb);
    auto grid_for = [&](int s_, int per_cu) { return (int)std::min<int64_t>((n + s_ - 1) / s_, (int64_t)d->cus * per_cu); };
    if (g.lds) {
        while (s > 1 && (size_t)slots * s * 8 > d->lds_budget) s /= 2;
        g.lds_bytes = (size_t)slots * s * 8;
        g.grid = grid_for(s, (int)std::min<size_t>(per_cu_max, std::max<size_t>(1, d->lds_budget / g.lds_bytes)));
    } else {
        const int64_t cap = std::max<int64_t>(std::min<int64_t>((int64_t)1 << 30, d->free_bytes / 4), slots * 8);
        while (s > 1 && (int64_t)grid_for(s, per_cu_max) * slots * s * 8 > cap) s /= 2;
        g.grid = grid_for(s, per_cu_max);
        if ((int64_t)g.grid * slots * s * 8 > cap) g.grid = (int)std::max<int64_t>(1, cap / (slots * s * 8));
    }
    while ((1 << g.log2s) < s) ++g.log2s;
    if (((slots + c.n_out) << g.log2s) >= ((int64_t)1 << 31)) throw std::runtime_error("DAIS level executor: the value file of a tile passes 2^31 entries");
    return g;
}

template <class In, class Out>
void launch_level(DaisDevExec *d, const dais::Chain &c, hipStream_t st, const LevelGeom &g, const void *x, int64_t x_stride, void *y, int64_t y_stride, int64_t n) {
    const int64_t tiles = (n + (1 << g.log2s) - 1) >> g.log2s;
    const int grid = (int)std::min<int64_t>(g.grid, tiles);
    if (g.lds)
        hipLaunchKernelGGL((k_dais_exec_level<In, Out, true>), dim3((unsigned)grid), dim3((unsigned)g.tpb), g.lds_bytes, st, d->lv_steps, d->lv_off,
                           (int)c.lv.n_levels(), d->lv_outs, (int)c.n_out, d->tables, (const In *)x, x_stride, (Out *)y, y_stride, (int64_t *)nullptr, c.lv.n_slots,
                           g.log2s, n, tiles, d->fault);
    else
        hipLaunchKernelGGL((k_dais_exec_level<In, Out, false>), dim3((unsigned)grid), dim3((unsigned)g.tpb), 0, st, d->lv_steps, d->lv_off, (int)c.lv.n_levels(),
                           d->lv_outs, (int)c.n_out, d->tables, (const In *)x, x_stride, (Out *)y, y_stride, (int64_t *)d->lv_file.p, c.lv.n_slots, g.log2s, n,
                           tiles, d->fault);
    DAIS_HIP(hipGetLastError());
}

void launch_level_typed(DaisDevExec *d, const dais::Chain &c, hipStream_t st, const LevelGeom &g, const void *x, int in_type, int64_t x_stride, void *y, int out_type,
                        int64_t y_stride, int64_t n) {
    if (in_type == DA_DAIS_F32)
        out_type == DA_DAIS_F32 ? launch_level<float, float>(d, c, st, g, x, x_stride, y, y_stride, n) : launch_level<float, double>(d, c, st, g, x, x_stride, y, y_stride, n);
    else
        out_type == DA_DAIS_F32 ? launch_level<double, float>(d, c, st, g, x, x_stride, y, y_stride, n) : launch_level<double, double>(d, c, st, g, x, x_stride, y, y_stride, n);
}

// the dynamic LDS the level kernel may ask for beside its static LDS, as sel2_lds_budget (hip_chain_setup.h) works it out for the selection
// kernel; its LDS instantiations are allowed that much
int level_device() {
    int device = 0;
#if defined(__HIPCC__)  // (the HIP stand-in of the emulated build, tests/emu, has the one device 0 and no call to ask for it)
    DAIS_HIP(hipGetDevice(&device));
#endif
    return device;
}
size_t level_lds_budget() {
    const int device = level_device();
    hipFuncAttributes fa;
    DAIS_HIP(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_dais_exec_level<double, double, true>)));
    int limit = 0;
    DAIS_HIP(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (limit < 64 * 1024) limit = 64 * 1024;
    const size_t used = fa.sharedSizeBytes + 256;
    const size_t budget = (size_t)limit > used ? (size_t)limit - used : 0;
    if (budget > 64 * 1024) {
        const int b = (int)budget;
        DAIS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dais_exec_level<double, double, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b));
        DAIS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dais_exec_level<double, float, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b));
        DAIS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dais_exec_level<float, double, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b));
        DAIS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_dais_exec_level<float, float, true>), hipFuncAttributeMaxDynamicSharedMemorySize, b));
    }
    return budget;
}

}  // namespace

DaisDevExec *dais_dev_create(const dais::Chain &c) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return nullptr;
    DaisDevExec *d = new DaisDevExec;
    try {
        auto upload = [&](auto **dst, const auto &v) {
            using T = typename std::remove_reference<decltype(v)>::type::value_type;
            DAIS_HIP(hipMalloc((void **)dst, std::max<size_t>(v.size(), 1) * sizeof(T)));
            if (!v.empty()) DAIS_HIP(hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        };
        upload(&d->steps, c.steps);
        upload(&d->outs, c.outs);
        upload(&d->tables, c.tables);
        DAIS_HIP(hipMalloc((void **)&d->fault, sizeof(unsigned long long)));
        DAIS_HIP(hipMemset(d->fault, 0, sizeof(unsigned long long)));
        DAIS_HIP(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        // tile: as many samples as fit a register-file budget (1/4 of free memory, at most 2^22 samples), as dais_run_gpu
        size_t free_b = 0, total_b = 0;
        DAIS_HIP(hipMemGetInfo(&free_b, &total_b));
        const int64_t per_sample = c.n_slots * 8 + (c.n_in + c.n_out) * 8;
        d->tile_cap = std::min<int64_t>((int64_t)1 << 22, std::max<int64_t>((int64_t)(free_b / 4) / std::max<int64_t>(per_sample, 1), TPB));
        upload(&d->lv_steps, c.lv.steps);
        upload(&d->lv_off, c.lv.level_off);
        upload(&d->lv_outs, c.lv.outs);
        d->free_bytes = (int64_t)free_b;
        d->lds_budget = level_lds_budget();
        hipDeviceProp_t prop;
        DAIS_HIP(hipGetDeviceProperties(&prop, level_device()));
        d->cus = std::max(1, prop.multiProcessorCount);
    } catch (...) {
        dais_dev_free(d);
        throw;
    }
    return d;
}

void dais_dev_scratch(const DaisDevExec *d, int64_t *s3) {
    s3[0] = d ? (int64_t)(intptr_t)d->regs.p : 0, s3[1] = d ? (int64_t)d->regs.bytes : 0, s3[2] = d ? d->allocations : 0;
}

void dais_dev_last(const DaisDevExec *d, int64_t *l2) { l2[0] = d ? d->last_run : -1, l2[1] = d ? d->last_s : 0; }

void dais_dev_run(DaisDevExec *d, const dais::Chain &c, const void *in, int in_type, int64_t in_stride, int64_t n_samples, void *out, int out_type,
                  int64_t out_stride, bool resident, void *stream, int mode) {
    if (!d) throw std::runtime_error("no HIP device: the DAIS device executor needs a GPU (the host executor does not)");
    if (n_samples <= 0) return;
    int64_t tile = std::min(n_samples, d->tile_cap);
    if (const char *e = std::getenv("DA4ML_DAIS_TILE"))  // experiment knob: samples per launch (cache residency vs occupancy)
        tile = std::max<int64_t>(1, std::min<int64_t>(tile, std::atoll(e)));
    tile = (tile + TPB - 1) / TPB * TPB;
    hipStream_t st = stream ? (hipStream_t)stream : d->stream;
    const bool level = mode == dais::MODE_LEVEL;
    LevelGeom g;
    if (level) {  // one geometry for all tiles of the call: that of a whole tile
        g = level_geometry(d, c, tile < n_samples ? tile : n_samples);
        if (!g.lds) d->allocations += d->lv_file.need((size_t)g.grid * (size_t)(c.lv.n_slots << g.log2s) * sizeof(int64_t));
        d->last_run = g.lds ? 1 : 2, d->last_s = 1 << g.log2s;
    } else {
        d->allocations += d->regs.need((size_t)(c.n_slots * tile) * sizeof(int64_t));
        d->last_run = 0;
    }
    auto launch = [&](const void *x, void *y, int64_t n) {
        if (level)
            launch_level_typed(d, c, st, g, x, in_type, in_stride, y, out_type, out_stride, n);
        else
            launch_typed(d, c, st, x, in_type, in_stride, y, out_type, out_stride, tile, n);
    };
    const size_t in_sz = elem_size(in_type), out_sz = elem_size(out_type);
    // a tile of host rows is staged as one span of its rows with their stride
    auto span = [](int64_t rows, int64_t stride, int64_t row) { return (size_t)((rows - 1) * stride + row); };
    if (!resident) {
        d->allocations += d->x.need(std::max<size_t>(span(tile, in_stride, c.n_in) * in_sz, 1));
        d->allocations += d->y.need(std::max<size_t>(span(tile, out_stride, c.n_out) * out_sz, 1));
    }
    for (int64_t s0 = 0; s0 < n_samples; s0 += tile) {
        const int64_t n = std::min(tile, n_samples - s0);
        const char *xi = (const char *)in + (size_t)(s0 * in_stride) * in_sz;
        char *yo = (char *)out + (size_t)(s0 * out_stride) * out_sz;
        if (resident) {
            launch(xi, yo, n);
            continue;
        }
        if (c.n_in > 0) DAIS_HIP(hipMemcpyAsync(d->x.p, xi, span(n, in_stride, c.n_in) * in_sz, hipMemcpyHostToDevice, st));
        launch(d->x.p, d->y.p, n);
        if (c.n_out > 0) {
            if (out_stride == c.n_out)
                DAIS_HIP(hipMemcpyAsync(yo, d->y.p, (size_t)(n * c.n_out) * out_sz, hipMemcpyDeviceToHost, st));
            else  // the elements between the rows of the caller's array are not the executor's to write
                for (int64_t r = 0; r < n; ++r)
                    DAIS_HIP(hipMemcpyAsync(yo + (size_t)(r * out_stride) * out_sz, (const char *)d->y.p + (size_t)(r * out_stride) * out_sz,
                                            (size_t)c.n_out * out_sz, hipMemcpyDeviceToHost, st));
        }
    }
    // queued work of a caller's stream stays queued; a chain with table statements, the handle's own stream and staged runs are waited for
    if (!resident || !stream || c.has_tables) {
        unsigned long long fault = 0;
        if (c.has_tables) {
            DAIS_HIP(hipMemcpyAsync(&fault, d->fault, sizeof fault, hipMemcpyDeviceToHost, st));
            DAIS_HIP(hipStreamSynchronize(st));
            if (fault) DAIS_HIP(hipMemset(d->fault, 0, sizeof fault));  // the handle stays usable
        } else
            DAIS_HIP(hipStreamSynchronize(st));
        if (fault) {
            const int64_t idx = (int64_t)(int32_t)(uint32_t)(fault & 0xFFFFFFFFull);
            throw std::runtime_error("Logic lookup index out of bounds: index=" + std::to_string(idx) +
                                     ", table_size=" + std::to_string((fault >> 32) & 0x7FFFFFFFull));
        }
    }
}
