// hip_shard_engine.h -- HipShardEngine, the column-sharded chain on the GPU (k_cs_* kernels), and its factory.
// Host code of the HIP backend: cmvm_engine.hip includes it after the kernels, inside namespace da::gpu; nothing else may.
#pragma once
#ifndef DA_ENGINE_TU
#error "hip_shard_engine.h is a part of cmvm_engine.hip"
#endif

// ------------------------------------------------------------------------------------------------ column-sharded chain
namespace {

// da::ShardEngine on the GPU: one chain, the digits of the columns [c0, c1), a replica of the pair table.  Phases are
// kernel launches on the backend's stream, each followed by a stream synchronisation: the exchange between the phases
// (all-reduce of the buffers handed out here) is issued by the caller on its own stream / library.
class HipShardEngine : public ShardEngine {
  public:
    HipShardEngine(hipStream_t st, int device, const ChainJob &job, int c0, int c1, double table_scale, double row_scale)
        : st_(st), device_(device), job_(job), n_loc_(c1 - c0) {
        HIP_CHECK(hipSetDevice(device_));
        // inputs + centred matrix of the WHOLE matrix (centring and digit width are global properties)
        const InputLayout L = input_layout(job.n_in, job.n_out);
        unsigned char *io = static_cast<unsigned char *>(io_.get(L.bytes + 256));
        fill_job(d_, job, n_loc_, c0, io, L);
        HIP_CHECK(hipMemcpyAsync(io + L.kernel, job.kernel, (size_t)job.n_in * job.n_out * 4, hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(io + L.qints, job.qints, (size_t)job.n_in * 12, hipMemcpyHostToDevice, st_));
        HIP_CHECK(hipMemcpyAsync(io + L.lats, job.lats, (size_t)job.n_in * 4, hipMemcpyHostToDevice, st_));
        dd_ = static_cast<ChainDev *>(desc_.get(sizeof(ChainDev)));
        push();
        hipLaunchKernelGGL(k_prepare, dim3(1), dim3(256), (size_t)job.n_out * 4, st_, dd_);
        HIP_CHECK(hipGetLastError());
        pull();
        // geometry: the batch's, of n_loc_ columns, with the statistics of the whole matrix (the table is global)
        static const GeometryErrors msg{"kernel needs more than 30 CSD digits per entry; unsupported", "problem too large for the row-reference format"};
        if (job.adder_size >= 0 || job.carry_size >= 0) step_tab_.build(job.qints, job.n_in);  // -log2f of non-power-of-two input steps (StepLog2), as in run_chains
        geo_ = derive_geometry(d_, job, n_loc_, (int)step_tab_.mant.size(), table_scale, row_scale, msg);
        const Geometry &g = geo_;
        n_pairs_ = (long long)job.n_in * (job.n_in + 1) / 2;
        // arena: the chain's arrays (local column count) + the exchange buffers
        ChainDev tmp;
        const size_t chain_bytes = carve_chain(nullptr, n_loc_, g, tmp);
        const size_t init_b = align_up((size_t)n_pairs_ * g.K * 4, 256), flag_b = align_up((((size_t)g.rcap + 3) / 4 + SHARD_TRAILER) * 4 + 64, 256),
                     uni_b = align_up((size_t)g.rcap * 4, 256), slab_b = align_up((size_t)(6 + 3 * (size_t)g.rcap) * g.K * 4, 256);
        const size_t need = chain_bytes + init_b + flag_b + uni_b + slab_b;
        {
            size_t free_b = 0, total_b = 0;
            HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
            if (need > free_b)
                throw std::runtime_error("a column-sharded chain needs " + std::to_string(need >> 20) + " MiB of device memory (pair table of " +
                                         std::to_string(g.C) + " slots), " + std::to_string(free_b >> 20) + " MiB are free");
        }
        unsigned char *a = static_cast<unsigned char *>(arena_.get(need));
        carve_chain(a, n_loc_, g, d_);
        d_.cs_init = reinterpret_cast<int32_t *>(a + chain_bytes);
        d_.cs_flags = reinterpret_cast<int32_t *>(a + chain_bytes + init_b);
        d_.cs_uni = reinterpret_cast<uint32_t *>(a + chain_bytes + init_b + flag_b);
        d_.cs_slab = reinterpret_cast<int32_t *>(a + chain_bytes + init_b + flag_b + uni_b);
        apply_geometry(d_, g, sel2_lds_budget(device_, g.wide));
        HIP_CHECK(hipMemsetAsync(d_.stamp, 0, sizeof(uint32_t) * (size_t)g.rcap, st_));
        HIP_CHECK(hipMemsetAsync(d_.hkey, 0xFF, sizeof(unsigned long long) * (size_t)g.C, st_));
        HIP_CHECK(hipMemsetAsync(d_.hrank, 0, sizeof(uint32_t) * (size_t)g.C, st_));
        HIP_CHECK(hipMemsetAsync(d_.grec, 0, sizeof(GroupRec) * (size_t)g.n_groups, st_));  // (bound 0 = nothing in the group: its flag is not looked at; the first entry that rises sets it)
        HIP_CHECK(hipMemsetAsync(d_.colbits, 0, sizeof(uint32_t) * (size_t)n_loc_ * d_.cb_words, st_));
        upload_step_table(d_, step_tab_, st_);  // (step_tab_ is a member: alive until the synchronise below and beyond)
        push();
        report_ = static_cast<volatile int *>(report_buf_.get(64));
        for (int q = 0; q < 5; ++q) report_[q] = 0;
        d_done_ = static_cast<unsigned int *>(done_buf_.get(sizeof(unsigned int)));  // (a member buffer: released also when a later check of this constructor throws)
        HIP_CHECK(hipMemsetAsync(d_done_, 0, sizeof(unsigned int), st_));
        per_cell([&](auto c) { hipLaunchKernelGGL(k_init_cells<decltype(c)>, dim3((n_loc_ + 3) / 4, 1), dim3(256), 0, st_, dd_, (const ChainRecode *)nullptr); });
        HIP_CHECK(hipGetLastError());
        sel_lds_ = align_up(sel2_fixed_lds(n_loc_, g) + (size_t)d_.claim_words * 4, 16);
        if (sel_lds_ > sel2_lds_budget(device_, g.wide)) throw std::runtime_error("selection kernel needs more dynamic LDS than the device leaves beside its static arrays (n_out too large)");
        sel2_allow_lds<true>(g.wide, sel_lds_);
        part_lds_ = align_up(2 * (size_t)n_loc_ * (g.wide ? 8 : 4) + 4 * 3 * (size_t)g.Kpad * 4 + (size_t)n_loc_ * 2, 16);
        HIP_CHECK(hipStreamSynchronize(st_));
    }
    ~HipShardEngine() override { (void)hipSetDevice(device_); }
    bool on_device() const override { return true; }
    int n_keys() const override { return geo_.K; }
    int32_t *init_counts(int64_t &count) override {
        const dim3 grid((unsigned)((n_pairs_ + 3) / 4));
        per_cell([&](auto c) { hipLaunchKernelGGL(k_cs_init_counts<decltype(c)>, grid, dim3(256), (size_t)4 * geo_.Kpad * 4, st_, dd_); });
        sync();
        count = n_pairs_ * geo_.K;
        return d_.cs_init;
    }
    void init_table() override {
        const dim3 grid((unsigned)((n_pairs_ + 3) / 4));
        per_cell([&](auto c) { hipLaunchKernelGGL(k_cs_init_table<decltype(c)>, grid, dim3(256), 0, st_, dd_); });
        HIP_CHECK(hipGetLastError());
    }
    void set_stream_ordered(bool on) override { stream_ordered_ = on; }
    // The host reads NOTHING back between the kernels of a step except, once per step, the summed status trailer and the size
    // of the partner union (one synchronisation): the rows before a step are n_in + the steps taken, and a chain that stops
    // writes its zero flags and trailer on the device (select_body, shard_stop).  With a stream-ordered transport (the library's
    // RCCL transport: collectives queued on this stream) that is the only synchronisation of a step; a callback transport is
    // handed completed buffers, i.e. one synchronisation in front of each of its two calls.
    void select(int32_t *&flags, int64_t &fcount) override {
        fw_ = flag_words(job_.n_in + (int)steps_);  // rows before this step
        if (!stopped_) {
            // the two-block selection of the ordinary chains (search beside substitution, the pick known one step ahead): the table is a replica,
            // so every rank takes the same pick; the substitution block leaves flags and partial special-pair counts instead of a partner list
            per_cell([&](auto c) { hipLaunchKernelGGL((k_iter_select2<decltype(c), true>), dim3(1, 2), dim3(SEL2_THREADS), sel_lds_, st_, dd_, 1, d_done_, (int)steps_); });
            HIP_CHECK(hipGetLastError());
        } else {  // (not reached by ShardedBackend, which leaves the loop with the step that stopped; kept well-defined)
            static const int32_t tr[SHARD_TRAILER] = {1, 0, 0};  // (static: read by an asynchronous copy)
            HIP_CHECK(hipMemsetAsync(d_.cs_flags, 0, (size_t)fw_ * 4, st_));
            HIP_CHECK(hipMemcpyAsync(d_.cs_flags + fw_, tr, sizeof tr, hipMemcpyHostToDevice, st_));
            sync();
        }
        if (!stream_ordered_) sync();
        flags = d_.cs_flags;
        fcount = fw_ + SHARD_TRAILER;
    }
    int32_t *partial(int64_t &scount, int32_t status[SHARD_TRAILER]) override {
        // the summed status and the size of the union come from the device itself: k_cs_union writes them into pinned host memory, the
        // host waits for the step's sequence number -- no copies, no stream synchronisation (the launch is checked; a device fault
        // surfaces through the bounded wait's fall-back synchronisation)
        const int seq = ++report_seq_;
        hipLaunchKernelGGL(k_cs_union, dim3(1), dim3(1024), 0, st_, dd_, report_, seq, (int)fw_);  // (on summed flags that are all zero when every rank has stopped: an empty union)
        HIP_CHECK(hipGetLastError());
        {
            unsigned polls = 0, tries = 0;
            while (__atomic_load_n(&report_[0], __ATOMIC_ACQUIRE) != seq) {
                if (++tries > (1u << 16)) {  // (seconds of polling, most of it asleep) let the runtime wait -- and report a fault, if that is what it is
                    sync();
                    if (__atomic_load_n(&report_[0], __ATOMIC_ACQUIRE) != seq) throw std::runtime_error("column-sharded chain: the device did not report the step's status");
                    break;
                }
                spin_wait_step(polls);
            }
        }
        const int nuni = report_[1];
        for (int q = 0; q < SHARD_TRAILER; ++q) trailer_[q] = report_[2 + q];
        for (int q = 0; q < SHARD_TRAILER; ++q) status[q] = trailer_[q];
        scount = 0;
        if (status[0] != 0) {
            stopped_ = true;
            return nullptr;
        }
        nuni_ = nuni;
        if (nuni > 0) {
            const dim3 grid((unsigned)((nuni + 3) / 4));
            per_cell([&](auto c) { hipLaunchKernelGGL(k_cs_partial<decltype(c)>, grid, dim3(256), part_lds_, st_, dd_); });
        }
        if (!stream_ordered_) sync();
        scount = (int64_t)(6 + 3 * (int64_t)nuni) * geo_.K;
        return d_.cs_slab;
    }
    void apply() override {
        const dim3 grid((unsigned)((nuni_ + 6 + 3) / 4));
        per_cell([&](auto c) { hipLaunchKernelGGL(k_cs_apply<decltype(c)>, grid, dim3(256), 0, st_, dd_); });
        HIP_CHECK(hipGetLastError());
        ++steps_;
    }
    void finish(ChainOut &o) override {
        per_cell([&](auto c) { hipLaunchKernelGGL(k_extract<decltype(c)>, dim3((n_loc_ + 3) / 4, 1), dim3(256), 0, st_, dd_); });
        hipLaunchKernelGGL(k_pack, dim3(1), dim3(256), 0, st_, dd_);
        pull();
        fill_result(o, d_);
        const size_t iters = (size_t)d_.iter;
        o.shift0.resize(job_.n_in);
        o.shift1.resize(job_.n_out);
        o.picks.resize(iters * 4);
        o.row_lat.resize((size_t)d_.n_rows);
        o.col_start.resize((size_t)n_loc_ + 1);
        HIP_CHECK(hipMemcpyAsync(o.shift0.data(), d_.shift0, job_.n_in, hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(o.shift1.data(), d_.shift1, job_.n_out, hipMemcpyDeviceToHost, st_));
        if (iters) HIP_CHECK(hipMemcpyAsync(o.picks.data(), d_.picks, iters * sizeof(int4), hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(o.row_lat.data(), d_.pk_lat, (size_t)d_.n_rows * 4, hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipMemcpyAsync(o.col_start.data(), d_.fin_start, ((size_t)n_loc_ + 1) * 4, hipMemcpyDeviceToHost, st_));
        sync();
        const size_t total = o.col_start[n_loc_];
        o.dig_row.resize(total);
        std::vector<unsigned long long> cells(total);
        if (total) {
            HIP_CHECK(hipMemcpyAsync(o.dig_row.data(), d_.pk_row, total * 4, hipMemcpyDeviceToHost, st_));
            HIP_CHECK(hipMemcpyAsync(cells.data(), d_.pk_cell, total * 8, hipMemcpyDeviceToHost, st_));
            sync();
        }
        o.dig_cell.assign(cells.begin(), cells.end());
    }

  private:
    template <class F> void per_cell(F &&f) { with_cell(geo_.wide, f); }  // f(Cell{}) for this chain's cell type
    void sync() {
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st_));
    }
    void push() { HIP_CHECK(hipMemcpyAsync(dd_, &d_, sizeof d_, hipMemcpyHostToDevice, st_)); }
    void pull() {
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(&d_, dd_, sizeof d_, hipMemcpyDeviceToHost, st_));
        HIP_CHECK(hipStreamSynchronize(st_));
    }
    hipStream_t st_;
    StepLog2Host step_tab_;
    int64_t fw_ = 0;                      // flag words of the current step (the status trailer follows them)
    long long steps_ = 0;                 // greedy steps applied so far (rows = n_in + steps_)
    bool stopped_ = false, stream_ordered_ = false;
    int32_t trailer_[SHARD_TRAILER] = {0, 0, 0};
    int device_;
    ChainJob job_;
    int n_loc_;  // columns of this rank (the first of them is d_.col0)
    ChainDev d_;
    ChainDev *dd_ = nullptr;
    Geometry geo_;
    DeviceBuffer io_, desc_, arena_;
    DeviceBuffer done_buf_;
    unsigned int *d_done_ = nullptr;
    PinnedBuffer report_buf_;          // {sequence number, union size, status[3]} written by k_cs_union (mapped pinned memory)
    volatile int *report_ = nullptr;
    int report_seq_ = 0;
    long long n_pairs_ = 0;
    int nuni_ = 0;
    size_t sel_lds_ = 0, part_lds_ = 0;
};

}  // namespace

std::unique_ptr<ShardEngine> HipBackend::make_shard_engine(const ChainJob &job, int c0, int c1, double capacity_scale) {
    return std::unique_ptr<ShardEngine>(new HipShardEngine(impl_->stream, impl_->device, job, c0, c1, impl_->table_scale * capacity_scale, row_scale_ * capacity_scale));
}
