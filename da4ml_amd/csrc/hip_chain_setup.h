// hip_chain_setup.h -- HipBackend::Impl and the one set-up of a chain: input layout, geometry, arena carve, descriptor, result.
// Host code of the HIP backend: cmvm_engine.hip includes it after the kernels, inside namespace da::gpu; nothing else may.
#pragma once
#ifndef DA_ENGINE_TU
#error "hip_chain_setup.h is a part of cmvm_engine.hip"
#endif

struct HipBackend::Impl {
    int device = 0;
    PinnedBuffer pinned, pinned_up;  // staging of the downloads / of the upload
    hipStream_t stream = nullptr;
    static constexpr int MAX_LANES = 8;
    hipStream_t lanes[MAX_LANES] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // greedy-loop streams of the chain groups
    int launch_threads = 2;  // host threads queueing the greedy loop's launches (each its share of the chain groups); DA4ML_HIP_LAUNCH_THREADS
    int n_lanes = 4;  // chain groups = greedy-loop streams.  Measured (C3 batch 64, loop ms): 2 -> 880, 3 -> 871, 4 -> 838, 5..8 -> 1470:
                      // four hardware queues; the poll stream's rare copies share one of them at no visible cost
    int upd_total_blocks = 2560;  // k_iter_update blocks over all chains of a batch (4 waves x 4 groups each); measured (C3 batch 64,
                                  // solves/s): 1024: 45.3, 1536: 53.3, 2048: 53.8, 2560: 55.5, 4096: 47.5; again with seven resident waves per SIMD
                                  // (profiles/ab_update_register_diet.txt): 1792: 110.9, 2048: 112.8, 2304: 113.4, 2560: 113.2 - 113.7, 3072: 113.7, 3328: 113.0 -- flat around 2560
    DeviceBuffer arena, desc_buf, io_buf, gather_buf, piece_buf, recode_buf;  // gather_buf: the results of a batch, contiguous, before they leave; recode_buf: k_init_cells' side array
    unsigned int *d_done = nullptr;
    unsigned int *h_done = nullptr;  // pinned, two words: done counters of alternating poll windows
    hipStream_t poll_stream = nullptr;
    GpuTimings timings;
    double table_scale = 1.0;  // grows on E_TABLE_CAPACITY retries
    int manycol_from = 0;  // chains of at least so many columns run the many-column selection kernel whatever fits (0: only those whose regular carve does not fit); DA4ML_HIP_MANYCOL_FROM
    struct Batch;  // the state of one run_chains call
};

HipBackend::HipBackend(int device) : impl_(new Impl) {
    impl_->device = device;
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&impl_->stream, hipStreamNonBlocking));
    impl_->lanes[0] = impl_->stream;  // the first group runs on the main stream (hardware queues are a scarce resource)
    for (int l = 1; l < Impl::MAX_LANES; ++l) HIP_CHECK(hipStreamCreateWithFlags(&impl_->lanes[l], hipStreamNonBlocking));
    if (const char *e = std::getenv("DA4ML_HIP_TABLE_SCALE")) impl_->table_scale = std::max(1e-4, std::atof(e));
    if (const char *e = std::getenv("DA4ML_HIP_MANYCOL_FROM")) impl_->manycol_from = std::max(0, std::atoi(e));
    if (const char *e = std::getenv("DA4ML_HIP_ROW_SCALE")) row_scale_ = std::max(1e-4, std::atof(e));
    if (const char *e = std::getenv("DA4ML_HIP_UPD_BLOCKS")) impl_->upd_total_blocks = std::max(2, std::atoi(e));
    if (const char *e = std::getenv("DA4ML_HIP_LAUNCH_THREADS")) impl_->launch_threads = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("DA4ML_HIP_LANES")) impl_->n_lanes = std::max(1, std::min((int)Impl::MAX_LANES, std::atoi(e)));
    HIP_CHECK(hipMalloc(&impl_->d_done, sizeof(unsigned int)));
    HIP_CHECK(hipHostMalloc(&impl_->h_done, 2 * sizeof(unsigned int), hipHostMallocDefault));
    HIP_CHECK(hipStreamCreateWithFlags(&impl_->poll_stream, hipStreamNonBlocking));
    Log2Table t = measure_log2_table();
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_log2), &t, sizeof t));
}
HipBackend::~HipBackend() {
    (void)hipSetDevice(impl_->device);
    if (impl_->d_done) (void)hipFree(impl_->d_done);
    if (impl_->h_done) (void)hipHostFree(impl_->h_done);
    if (impl_->poll_stream) (void)hipStreamDestroy(impl_->poll_stream);
    if (impl_->stream) (void)hipStreamDestroy(impl_->stream);
    for (int l = 1; l < Impl::MAX_LANES; ++l)
        if (impl_->lanes[l]) (void)hipStreamDestroy(impl_->lanes[l]);
}
const GpuTimings &HipBackend::timings() const { return impl_->timings; }
void HipBackend::reset_timings() { impl_->timings = GpuTimings{}; }
void *HipBackend::stream() const { return impl_->stream; }

namespace {

struct Geometry {
    bool wide;  // 64-bit cells and 16-byte list entries (more than 12 digits or more than 256 columns)
    int n_mant = 0;  // distinct non-power-of-two step mantissas of the inputs (StepLog2): rows of the -log2f table
    int n_bits, K, Kpad, rcap, lcap, gs_log2, n_groups, pk_cap, pb_log2;
    uint32_t C, rl_cap;
};

// The unsharded instantiation of k_iter_select2 for a cell width, a carve of the substitution block and a tie order:
// f(Cell{}, std::bool_constant<MANYCOL>{}, std::bool_constant<SEEDED>{})
template <class F> void with_sel2(bool wide, bool manycol, bool seeded, F &&f) {
    with_cell(wide, [&](auto c) { with_flag(manycol, [&](auto mc) { with_flag(seeded, [&](auto sd) { f(c, mc, sd); }); }); });
}
// raises the dynamic-LDS limit of the selection kernel the chains of that width and carve are about to be launched with (column-sharded
// chains have the regular carve only)
template <bool SHARDED> void sel2_allow_lds(bool wide, size_t bytes, bool manycol = false, bool seeded = false) {
    if constexpr (SHARDED)
        with_cell(wide, [&](auto c) {
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_select2<decltype(c), true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        });
    else
        with_sel2(wide, manycol, seeded, [&](auto c, auto mc, auto sd) {
            HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_select2<decltype(c), false, decltype(mc)::value, decltype(sd)::value>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        });
}

// Byte offsets of a chain's inputs in an io buffer: kernel | qints | lats | xint (the centred matrix, written by k_prepare) | shift0 | shift1, each
// rounded to 256 bytes.  Without `lats` (csd_decompose) that part is empty.
struct InputLayout {
    size_t kernel = 0, qints, lats, xint, shift0, shift1, bytes;
};
InputLayout input_layout(int n_in, int n_out, bool lats = true) {
    const size_t e = (size_t)n_in * n_out;
    InputLayout L;
    L.qints = align_up(e * 4, 256);
    L.lats = L.qints + align_up((size_t)n_in * 12, 256);
    L.xint = L.lats + (lats ? align_up((size_t)n_in * 4, 256) : 0);
    L.shift0 = L.xint + align_up(e * 4, 256);
    L.shift1 = L.shift0 + align_up(n_in, 256);
    L.bytes = L.shift1 + align_up(n_out, 256);
    return L;
}

// The latency-penalty weight a chain's -dc / -pdc method scores with: the job's, or the method's constant when the job sets none (always filled in;
// mc, wmc and dummy never read it).  A chain is WEIGHTED -- it runs the instantiations of k_init_pairs and k_iter_update that read the weight from
// the descriptor -- when that is not, bit for bit, the constant its method has as a literal in the other instantiations.
float chain_dc_weight(const ChainJob &j) { return j.dc_weight >= 0.0f ? j.dc_weight : dc_weight_default(j.method); }
bool chain_weighted(const ChainJob &j) {
    const bool dc = j.method == M_MC_DC || j.method == M_MC_PDC || j.method == M_WMC_DC || j.method == M_WMC_PDC;
    return dc && f2u(chain_dc_weight(j)) != f2u(dc_weight_default(j.method));
}

// A chain scores with a slack (entry_rank_slack, cmvm_core.h) -- it runs the SLACK instantiations of k_init_pairs and k_iter_update -- when the job
// sets one and has the seed that keys it (the C entry refuses a slack without a seed; a job without greedy loop reads neither)
bool chain_slack(const ChainJob &j) { return j.slack != 0 && j.tie_seed != 0; }
// f(std::bool_constant<SEEDED>{}, std::bool_constant<WEIGHTED>{}, std::bool_constant<SLACK>{}) for the rank-forming kernels: the slack instantiations
// exist with a seed and a carried weight only
template <class F> void with_rank_flags(bool seeded, bool weighted, bool slack, F &&f) {
    if (slack)
        f(std::true_type{}, std::true_type{}, std::true_type{});
    else
        with_flag(seeded, [&](auto sd) { with_flag(weighted, [&](auto wt) { f(sd, wt, std::false_type{}); }); });
}

// The job fields of a descriptor, all else zero: the chain holds the `n_loc` columns from `col0` on of the job's matrix, whose inputs are at `io`
void fill_job(ChainDev &d, const ChainJob &j, int n_loc, int col0, unsigned char *io, const InputLayout &L) {
    std::memset(&d, 0, sizeof d);
    d.n_in = j.n_in;
    d.n_out = n_loc;
    d.pn_out = j.n_out;
    d.col0 = col0;
    d.method = j.method;
    d.tie_seed = j.tie_seed;
    d.tie_order = j.tie_seed ? j.tie_order : TIE_ORDER_RANDOM;
    d.dc_weight = chain_dc_weight(j);
    d.slack = chain_slack(j) ? j.slack : 0u;
    d.adder_size = j.adder_size;
    d.carry_size = j.carry_size;
    d.kernel = reinterpret_cast<const float *>(io + L.kernel);
    d.qints = reinterpret_cast<const float *>(io + L.qints);
    d.lats = reinterpret_cast<const float *>(io + L.lats);
    d.xint = reinterpret_cast<int32_t *>(io + L.xint);
    d.shift0 = reinterpret_cast<int8_t *>(io + L.shift0);
    d.shift1 = reinterpret_cast<int8_t *>(io + L.shift1);
}

// Dynamic LDS of a k_iter_select2 block WITHOUT the optional claim area (pick_body's carve).  Regular: B's list, six count vectors, five per-column
// arrays.  Many-column: six count vectors, the matched columns' list lengths, three 16-bit per-column arrays (B's list stays in memory)
size_t sel2_fixed_lds(int n_out, const Geometry &g, bool manycol = false) {
    const size_t no = (size_t)n_out, entb = g.wide ? 16 : 4;
    if (manycol) return 6 * (size_t)g.Kpad * 4 + (no + 1) * 4 + 3 * no * 2;
    return no * entb + 6 * (size_t)g.Kpad * 4 + (5 * no + 1) * 4;
}
// What the device leaves for it: the per-workgroup LDS limit less the kernel's STATIC __shared__ arrays (the search block's bound / work lists,
// the substitution block's partner ids: 42 768 bytes with 2048 group records -- asked from the runtime, not assumed), less a small reserve.  Static + dynamic beyond the limit
// fails in hipFuncSetAttribute or at launch with a raw HIP error; the caller turns it into a clear message.
// (asked of the unseeded instantiation: the static arrays of a kernel do not depend on its tie order)
size_t sel2_lds_budget(int device, bool wide, bool manycol = false) {
    static std::mutex mu;
    static size_t cached[2][2] = {{0, 0}, {0, 0}};
    std::lock_guard<std::mutex> lk(mu);
    if (!cached[wide][manycol]) {
        hipFuncAttributes fa;
        const void *fn = nullptr;
        with_sel2(wide, manycol, false, [&](auto c, auto mc, auto) { fn = reinterpret_cast<const void *>(&k_iter_select2<decltype(c), false, decltype(mc)::value>); });
        HIP_CHECK(hipFuncGetAttributes(&fa, fn));
        int limit = 0;
        HIP_CHECK(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
        if (limit < 64 * 1024) limit = 64 * 1024;
        const size_t used = fa.sharedSizeBytes + 256;
        cached[wide][manycol] = (size_t)limit > used ? (size_t)limit - used : 1;
    }
    return cached[wide][manycol];
}
// The carve a chain of a batch runs with: the regular one whenever its fixed part fits (then the chain runs exactly the kernel it always ran);
// the many-column one beyond that, and from `manycol_from` columns on when that knob is set
bool sel2_manycol(int device, int n_out, const Geometry &g, int manycol_from) {
    return (manycol_from > 0 && n_out >= manycol_from) || align_up(sel2_fixed_lds(n_out, g), 16) > sel2_lds_budget(device, g.wide);
}
// k_iter_update's dynamic LDS (UpdLds: the hand-off tables, 22 bytes per column in the wide layout, and the waves' counters) passes the 64 KB a
// kernel may ask for without further ado from about 2800 columns on: the limit of its instantiations of that width is raised then, after a check
// against what the device has per workgroup.  Chains whose blocks ask for no more than 64 KB launch as they always did: nothing is queried or set.
void upd_allow_lds(int device, bool wide, size_t bytes) {
    if (bytes <= 64 * 1024) return;
    hipFuncAttributes fa;
    with_cell(wide, [&](auto c) { HIP_CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(&k_iter_update<decltype(c), false>))); });
    int limit = 0;
    HIP_CHECK(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
    if (fa.sharedSizeBytes + bytes > (size_t)limit)
        throw std::runtime_error("update kernel needs " + std::to_string(bytes) + " bytes of dynamic LDS beside " + std::to_string(fa.sharedSizeBytes) +
                                 " of static arrays, the device has " + std::to_string(limit) + " per workgroup (n_out too large)");
    with_cell(wide, [&](auto c) {
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), false, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), true, false, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), false, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), false, true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_iter_update<decltype(c), true, true, true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    });
}
// words of the optional LDS area in which the substitution block combines the row bitmaps of a young chain: dropped (0: every wave ORs its words
// itself) when it does not fit beside the rest -- the kernel runs either way
int claim_words_for(int n_out, const Geometry &g, size_t budget, bool manycol = false) {
    const size_t words = ((size_t)g.rcap + 31) / 32, fixed = align_up(sel2_fixed_lds(n_out, g, manycol), 16);
    return words * 4 <= 64 * 1024 && fixed + words * 4 + 16 <= budget ? (int)words : 0;
}

// The two range errors of derive_geometry, worded by its caller (the batch and the column-sharded chain word them differently)
struct GeometryErrors {
    const char *digits, *row_ref;
};
// Geometry of a chain of `n_loc` columns (all of the job's in a batch, a rank's slice in a column-sharded chain) from its prepared descriptor:
// k_prepare's statistics are those of the whole matrix, as is the pair table
Geometry derive_geometry(const ChainDev &d, const ChainJob &job, int n_loc, int n_mant, double table_scale, double row_scale, const GeometryErrors &msg) {
    Geometry g;
    g.n_bits = d.prep_nbits;
    if (g.n_bits > 30) throw std::runtime_error(msg.digits);
    g.wide = g.n_bits > 12 || n_loc > 256;  // the narrow list entry is col:8 | minus:12 | plus:12
    g.n_mant = n_mant;
    g.K = key_count(g.n_bits);
    g.Kpad = (g.K + 3) & ~3;
    g.pb_log2 = 5;  // payload line of a pair block: 16-byte header + Kpad u16 counts, padded to a power of two
    while ((1 << g.pb_log2) < 16 + 2 * g.Kpad) ++g.pb_log2;
    const long long D0 = d.prep_digits;
    const TableGeometry tg = table_geometry(job, d.prep_pairs, D0, table_scale, row_scale, MAX_GROUPS);
    g.rcap = tg.rcap < (1 << REF_ROW_BITS) ? (int)tg.rcap : (1 << REF_ROW_BITS);
    g.lcap = job.n_in + d.prep_maxdcol + 1;
    g.pk_cap = (int)std::min<long long>(D0 + 1, (long long)1 << 30);  // digits only ever disappear
    // row lists: the dense lists of the input rows + one entry per (new row, column), each holding at least one of
    // the digits that the substitutions move into new rows (at most D0 over a chain)
    const long long rl_want = (long long)job.n_in * n_loc + D0 + n_loc + 64;
    if (rl_want >= (1ll << REF_OFF_BITS) || g.rcap >= (1 << REF_ROW_BITS) || n_loc >= (1 << REF_LEN_BITS)) throw std::runtime_error(msg.row_ref);
    g.rl_cap = (uint32_t)rl_want;
    g.C = tg.C;
    g.gs_log2 = tg.gs_log2;
    g.n_groups = tg.n_groups;
    return g;
}

// carve one chain's arrays; with base == nullptr only the size is computed
size_t carve_chain(unsigned char *base, int n_loc, const Geometry &g, ChainDev &d) {
    Carver c(base);
    size_t cell = g.wide ? 8 : 4, entry = g.wide ? 16 : 4;
    size_t n_out = n_loc;
    d.rlist = c.take<unsigned char>((size_t)g.rl_cap * entry);
    d.rowoff = c.take<da_u2>(g.rcap);
    d.rows = c.take<RowInfo>(g.rcap);
    d.stamp = c.take<uint32_t>(g.rcap);
    d.collist = c.take<unsigned long long>(n_out * (size_t)g.lcap);
    d.collen = c.take<int>(n_out);
    d.hkey = c.take<unsigned long long>(g.C);
    d.hrank = c.take<uint32_t>((size_t)g.C + ((size_t)g.C + 3) / 4);  // + the best-key indices, one byte per slot, right behind the ranks (hidx_ptr)
    d.hblk = c.take<unsigned char>((size_t)g.C << g.pb_log2);
    d.grec = c.take<GroupRec>(g.n_groups);
    d.mcol = c.take<int>(n_out);
    d.cmap = c.take<uint16_t>(n_out);
    d.colbits = c.take<uint32_t>(n_out * (size_t)((g.rcap + 31) / 32));
    d.pl_ids = c.take<uint32_t>(g.rcap);
    d.mA = c.take<unsigned char>(n_out * cell);
    d.mB = c.take<unsigned char>(n_out * cell);
    d.plist = c.take<unsigned long long>(g.rcap);
    d.sp_cnt = c.take<uint32_t>((size_t)6 * g.Kpad);
    d.picks = c.take<int4>(g.rcap);
    d.fin_row = c.take<uint32_t>(n_out * (size_t)g.lcap);
    d.fin_cell = c.take<unsigned long long>(n_out * (size_t)g.lcap);
    d.fin_count = c.take<uint32_t>(n_out);
    d.fin_start = c.take<uint32_t>(n_out + 1);
    d.pk_cap = g.pk_cap;
    d.pk_row = c.take<uint32_t>((size_t)g.pk_cap);
    d.pk_cell = c.take<unsigned long long>((size_t)g.pk_cap);
    d.pk_lat = c.take<float>(g.rcap);
    d.step_mant = c.take<uint32_t>((size_t)std::max(g.n_mant, 1));  // filled only when an input step is not a power of two (StepLog2)
    d.step_tab = c.take<float>((size_t)std::max(g.n_mant, 1) * 256);
    return align_up(c.off, 256);
}

// The geometry into a descriptor whose job fields are set and whose arrays carve_chain has assigned: the chain before its first step
void apply_geometry(ChainDev &d, const Geometry &g, size_t lds_budget, bool manycol = false) {
    d.n_bits = g.n_bits;
    d.K = g.K;
    d.Kpad = g.Kpad;
    d.rcap = g.rcap;
    d.lcap = g.lcap;
    d.gs_log2 = g.gs_log2;
    d.n_groups = g.n_groups;
    d.C = g.C;
    d.cmask = g.C - 1;
    d.pb_log2 = g.pb_log2;
    d.rl_cap = g.rl_cap;
    d.rl_used = (uint32_t)d.n_in * (uint32_t)d.n_out;
    d.n_rows = d.n_in;
    d.claim_words = claim_words_for(d.n_out, g, lds_budget, manycol);
    d.iter = 0;
    d.cb_words = (g.rcap + 31) / 32;
    d.n_step_mant = g.n_mant;
}
// -log2f tables of non-power-of-two input steps into the chain's arena; `t` is read by asynchronous copies: the caller keeps it until `st` has been synchronised
void upload_step_table(const ChainDev &d, const StepLog2Host &t, hipStream_t st) {
    if (!d.n_step_mant) return;
    HIP_CHECK(hipMemcpyAsync(const_cast<uint32_t *>(d.step_mant), t.mant.data(), t.mant.size() * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(const_cast<float *>(d.step_tab), t.tab.data(), t.tab.size() * 4, hipMemcpyHostToDevice, st));
}

// What a chain reports of itself, from its final descriptor
void fill_result(ChainOut &o, const ChainDev &d) {
    o = ChainOut{};
    o.error = d.error;
    o.unknown_method_hit = d.unknown_hit != 0;
    o.n_bits = d.n_bits;
    o.stats.iterations = d.iter;
    o.stats.digits0 = d.prep_digits;
    o.stats.table_peak = d.live_peak;
    o.stats.scan_slots = (long long)d.st_rescans << d.gs_log2;
    o.stats.partners = (long long)d.st_partners;
    o.stats.matches = (long long)d.st_matches;
}

}  // namespace
