// hip_batch.h -- HipBackend::Impl::Batch, the phases of one call, and HipBackend::run_chains, which runs them.
// Host code of the HIP backend: cmvm_engine.hip includes it after the kernels, inside namespace da::gpu; nothing else may.
#pragma once
#ifndef DA_ENGINE_TU
#error "hip_batch.h is a part of cmvm_engine.hip"
#endif

// One call of run_chains: what its phases, in the order of their definition, hand to each other.
struct HipBackend::Impl::Batch {
    Impl &im;
    const ChainJob *const jobs;
    ChainOut *const outs;
    const int n;
    const hipStream_t st;
    Batch(Impl &impl, const ChainJob *j, ChainOut *o, int count) : im(impl), jobs(j), outs(o), n(count), st(impl.stream) {}

    // Pageable host memory that asynchronous copies on `st` read or write.  Each stays alive until the stream's next synchronise, which may come
    // in a later phase or, after an exception, not at all: they are members, never locals of a phase.
    std::vector<ChainDev> desc, sorted, fin;  // descriptors: as prepared and set up (job order) | sorted by width (only when that differs) | final (sorted order)
    // -log2f tables of non-power-of-two input steps (rare: the tracer's `variable * 3`), by the host libm, one row per distinct
    // mantissa -- as many as the inputs have (the reference takes log2 of any step, state_opr.cc:57); they stay alive until the
    // set-up stream has been synchronised at the end of init_chains
    std::vector<StepLog2Host> step_tabs;
    std::vector<GatherPiece> pieces;
    std::vector<ChainRecode> recode;  // the digit recoding of every chain, in the order of the device's descriptors: k_init_cells' side array

    ChainDev *d_desc = nullptr;
    int max_n_out = 0;
    std::vector<Geometry> geo;
    std::vector<size_t> a_off;  // of every chain in the arena
    size_t arena_bytes = 0, budget = 0, free_b = 0;
    std::vector<int> order;  // descriptor s of the device is chain order[s] of the call: chains with their method's own penalty weight first, of those the chains of the reference's tie order first, of those the narrow ones first, and of a width those of the regular selection carve first; the chains with a score slack come last
    std::vector<char> manycol;  // per chain: it runs the many-column instantiation of k_iter_select2 (sel2_manycol)
    static constexpr int N_VAR = 20;  // kernel variants of a batch: 8 * weighted + 4 * seeded + 2 * wide + manycol (a batch of restarts mixes tie orders: restart 0 has the reference's;
                                      // a sweep of penalty weights mixes weighted chains with those on their method's constant.  The selection kernel forms no rank: it has no weighted form),
                                      // and from 16 on the chains with a score slack: 16 + 2 * wide + manycol (they have a seed and read their weight from the descriptor, whatever it is)
    int variant(int i) const {
        if (chain_slack(jobs[i])) return 16 + 2 * (int)geo[i].wide + (int)manycol[i];
        return 8 * (int)chain_weighted(jobs[i]) + 4 * (int)(jobs[i].tie_seed != 0) + 2 * (int)geo[i].wide + (int)manycol[i];
    }
    static constexpr int sel_variant(int v) { return v < 16 ? v & 7 : 4 + (v & 3); }  // the selection kernel's instantiation: width, carve and seededness only
    struct Range {
        int first, count;
        bool wide, manycol, seeded, weighted, slack;
    } ranges[N_VAR];
    size_t sel_lds[N_VAR] = {}, upd_lds[N_VAR] = {};  // per variant: dynamic LDS of the loop's kernels, k_iter_update blocks per chain
    int upd_blocks[N_VAR] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    EventGuard events;  // declared before anything greedy_loop declares: destroyed after its streams have been drained, and after extract has read the clocks
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> sample_ev;  // three per sampled iteration
    int sampled_chains = 0;  // chains of the group whose kernels are sampled
    long long launched_iters = 0;
    double host_launch_ms = 0;  // host time spent queueing launches (not waiting for the device)
    float loop_ms = 0;

    // ---- 1. inputs to the device, k_prepare
    void upload_and_prepare() {
        std::vector<size_t> in_off(n);
        size_t in_bytes = 0;
        for (int i = 0; i < n; ++i) {
            in_off[i] = in_bytes;
            in_bytes += input_layout(jobs[i].n_in, jobs[i].n_out).bytes;
            max_n_out = std::max(max_n_out, jobs[i].n_out);
        }
        unsigned char *io = static_cast<unsigned char *>(im.io_buf.get(std::max<size_t>(in_bytes, 256)));
        unsigned char *stage_ptr = static_cast<unsigned char *>(im.pinned_up.get(std::max<size_t>(in_bytes, 256)));  // pinned: the upload is one asynchronous DMA
        desc.resize(n);
        // the inputs into the pinned staging buffer, on a few host threads (16 MB for the 64 matrices of the benchmark)
        parallel_for(n, in_bytes, [&](int i) {
            const ChainJob &j = jobs[i];
            const InputLayout L = input_layout(j.n_in, j.n_out);
            fill_job(desc[i], j, j.n_out, 0, io + in_off[i], L);
            std::memcpy(stage_ptr + in_off[i] + L.kernel, j.kernel, (size_t)j.n_in * j.n_out * 4);
            std::memcpy(stage_ptr + in_off[i] + L.qints, j.qints, (size_t)j.n_in * 12);
            std::memcpy(stage_ptr + in_off[i] + L.lats, j.lats, (size_t)j.n_in * 4);
        });
        HIP_CHECK(hipMemcpyAsync(io, stage_ptr, in_bytes, hipMemcpyHostToDevice, st));
        d_desc = static_cast<ChainDev *>(im.desc_buf.get(sizeof(ChainDev) * (size_t)n));
        HIP_CHECK(hipMemcpyAsync(d_desc, desc.data(), sizeof(ChainDev) * (size_t)n, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_prepare, dim3(n), dim3(256), (size_t)max_n_out * 4, st, d_desc);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(desc.data(), d_desc, sizeof(ChainDev) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // ---- 2. geometry of every chain, size of the arena and what device memory allows; nothing is queued
    void plan(double row_scale) {
        static const GeometryErrors msg{"kernel needs more than 30 CSD digits per entry (the reference overflows int32 there); unsupported",
                                        "problem too large for the row-reference format (rows < 2^24, columns < 4096, list entries < 2^28)"};
        step_tabs.resize(n);
        for (int i = 0; i < n; ++i)
            if (jobs[i].adder_size >= 0 || jobs[i].carry_size >= 0) step_tabs[i].build(jobs[i].qints, jobs[i].n_in);  // (latency model off: steps are never looked at)
        geo.resize(n);
        a_off.resize(n);
        for (int i = 0; i < n; ++i) {
            geo[i] = derive_geometry(desc[i], jobs[i], jobs[i].n_out, (int)step_tabs[i].mant.size(), im.table_scale, row_scale, msg);
            ChainDev tmp;
            a_off[i] = arena_bytes;
            arena_bytes += carve_chain(nullptr, jobs[i].n_out, geo[i], tmp);
        }
        size_t total_b = 0;
        HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
        budget = (size_t)(0.85 * (double)(free_b + im.arena.cap));
        if (const char *e = std::getenv("DA4ML_HIP_MEM_BUDGET_MB")) budget = (size_t)std::atoll(e) << 20;  // test hook
    }

    // ---- 3. arena, descriptors, initial state; launch sizes per cell width (descriptors are grouped so that one launch covers a contiguous range)
    void init_chains() {
        unsigned char *arena = static_cast<unsigned char *>(im.arena.get(arena_bytes));
        manycol.resize(n);
        for (int i = 0; i < n; ++i) {
            carve_chain(arena + a_off[i], jobs[i].n_out, geo[i], desc[i]);
            manycol[i] = sel2_manycol(im.device, jobs[i].n_out, geo[i], im.manycol_from);
            apply_geometry(desc[i], geo[i], sel2_lds_budget(im.device, geo[i].wide, manycol[i]), manycol[i]);
            desc[i].done = (jobs[i].method == M_DUMMY || jobs[i].method < 0) ? 1 : 0;
        }
        for (int i = 0; i < n; ++i) upload_step_table(desc[i], step_tabs[i], st);
        HIP_CHECK(hipMemcpyAsync(d_desc, desc.data(), sizeof(ChainDev) * (size_t)n, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemsetAsync(im.d_done, 0, sizeof(unsigned int), st));
        // initial state of all chains in ONE launch (was six hipMemsetAsync per chain: 384 calls and 384 small kernels per batch)
        hipLaunchKernelGGL(k_init_state, dim3(128, n), dim3(256), 0, st, d_desc);
        HIP_CHECK(hipGetLastError());

        order.resize(n);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return variant(a) < variant(b); });
        bool permuted = false;
        for (int i = 0; i < n; ++i) permuted |= order[i] != i;
        if (permuted) {
            sorted.resize(n);
            for (int i = 0; i < n; ++i) sorted[i] = desc[order[i]];
            HIP_CHECK(hipMemcpyAsync(d_desc, sorted.data(), sizeof(ChainDev) * (size_t)n, hipMemcpyHostToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        // the recoding of every chain beside its descriptor, not in it (k_init_cells alone reads it); a batch of CSD chains passes none
        const ChainRecode *d_recode = nullptr;
        bool recoded = false;
        for (int i = 0; i < n; ++i) recoded |= jobs[i].recode != RECODE_CSD;
        if (recoded) {
            recode.resize(n);
            for (int s = 0; s < n; ++s) recode[s] = ChainRecode{jobs[order[s]].recode == RECODE_SEEDED ? jobs[order[s]].recode_seed : 0ull, jobs[order[s]].recode, 0u};
            ChainRecode *buf = static_cast<ChainRecode *>(im.recode_buf.get(sizeof(ChainRecode) * (size_t)n));
            HIP_CHECK(hipMemcpyAsync(buf, recode.data(), sizeof(ChainRecode) * (size_t)n, hipMemcpyHostToDevice, st));
            d_recode = buf;
        }
        int n_of[N_VAR] = {};
        for (int i = 0; i < n; ++i) ++n_of[variant(i)];
        for (int v = 0, first = 0; v < N_VAR; first += n_of[v], ++v) ranges[v] = Range{first, n_of[v], (v & 2) != 0, (v & 1) != 0, v >= 16 || (v & 4) != 0, v >= 16 || (v & 8) != 0, v >= 16};

        size_t pair_lds[N_VAR] = {};
        long long max_pairs[N_VAR] = {};
        for (int i = 0; i < n; ++i) {
            const int w = variant(i);
            const size_t no = (size_t)jobs[i].n_out, cellb = geo[i].wide ? 8 : 4;
            const size_t s = align_up(sel2_fixed_lds(jobs[i].n_out, geo[i], manycol[i]) + (size_t)desc[i].claim_words * 4, 16);
            if (s > sel2_lds_budget(im.device, geo[i].wide, manycol[i]))
                throw std::runtime_error("selection kernel needs " + std::to_string(s) + " bytes of dynamic LDS, the device leaves it " +
                                         std::to_string(sel2_lds_budget(im.device, geo[i].wide, manycol[i])) + " beside the kernel's static arrays (n_out too large)");
            sel_lds[w] = std::max(sel_lds[w], s);
            upd_lds[w] = std::max(upd_lds[w], align_up(2 * no * cellb + no * 6, 16) + align_up((size_t)UPD_WAVES * (QN * 3 + 1) * (size_t)geo[i].Kpad * 4, 16));  // UpdLds: hand-off tables | counters
            pair_lds[w] = std::max(pair_lds[w], (size_t)4 * geo[i].Kpad * 4);
            max_pairs[w] = std::max(max_pairs[w], (long long)jobs[i].n_in * (jobs[i].n_in + 1) / 2);
        }
        for (int w = 0; w < N_VAR; ++w) {
            const Range &r = ranges[w];
            if (r.count == 0) continue;
            upd_blocks[w] = std::max(2, std::min(64, (im.upd_total_blocks + r.count - 1) / r.count));  // at least 2 and at most 64 blocks per chain
            ChainDev *base = d_desc + r.first;
            const dim3 colgrid((max_n_out + 3) / 4, r.count), pairgrid((unsigned)((max_pairs[w] + 3) / 4), r.count);
            with_cell(r.wide, [&](auto c) {
                hipLaunchKernelGGL(k_init_cells<decltype(c)>, colgrid, dim3(256), 0, st, base, d_recode ? d_recode + r.first : nullptr);
                with_rank_flags(r.seeded, r.weighted, r.slack, [&](auto sd, auto wt, auto sl) {
                    hipLaunchKernelGGL((k_init_pairs<decltype(c), decltype(sd)::value, decltype(wt)::value, decltype(sl)::value>), pairgrid, dim3(256), pair_lds[w], st, base);
                });
            });
            HIP_CHECK(hipGetLastError());
        }
        // one limit per instantiation of the selection kernel: it has no weighted and no slack form, so several ranges launch the same function and
        // the limit must cover the largest of them (set once per instantiation, a second call would lower what the first had just been given)
        for (int sv = 0; sv < 8; ++sv) {
            size_t most = 0;
            bool used = false;
            for (int w = 0; w < N_VAR; ++w)
                if (sel_variant(w) == sv && ranges[w].count) used = true, most = std::max(most, sel_lds[w]);
            if (used) sel2_allow_lds<false>((sv & 2) != 0, most, (sv & 1) != 0, (sv & 4) != 0);
        }
        for (int wide = 0; wide < 2; ++wide) {  // (one limit for all instantiations of a width)
            size_t most = 0;
            for (int w = 0; w < N_VAR; ++w)
                if (((w & 2) != 0) == (wide != 0)) most = std::max(most, upd_lds[w]);
            upd_allow_lds(im.device, wide != 0, most);
        }
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // ---- 4. greedy loop: two kernels per iteration.  The chains are split into up to four groups, each advancing
    // in lockstep on its own stream, so that the one-block-per-chain select kernel of one group overlaps the update
    // kernel of the others.
    // On an exception the helper thread is told to quit and joined, then the group streams and the poll stream are drained, then (with
    // this object) the events are destroyed: the declaration order groups, drain, helper, join_helper below, after the member `events`.
    void greedy_loop() {
        ev0 = events.make(), ev1 = events.make();
        HIP_CHECK(hipEventRecord(ev0, st));
        HIP_CHECK(hipStreamSynchronize(st));  // set-up done before the group streams start
        struct Group {
            int first, count, w;  // descriptor range, kernel variant (index of its range)
            hipStream_t stream;
        };
        std::vector<Group> groups;
        int n_ranges = 0;
        for (int w = 0; w < N_VAR; ++w) n_ranges += ranges[w].count != 0;
        for (int w = 0; w < N_VAR; ++w) {
            const Range &r = ranges[w];
            if (r.count == 0) continue;
            int parts = std::max(1, std::min(im.n_lanes, r.count / 8));
            if (n_ranges > 1) parts = std::max(1, parts / n_ranges);  // (groups beyond MAX_LANES share streams)
            for (int p = 0; p < parts; ++p) {
                int lo = r.first + (int)((long long)r.count * p / parts), hi = r.first + (int)((long long)r.count * (p + 1) / parts);
                groups.push_back(Group{lo, hi - lo, w, im.lanes[groups.size() % Impl::MAX_LANES]});
            }
        }
        sampled_chains = groups.empty() ? 0 : groups[0].count;
        // One greedy iteration of one group = (select, update) on the group's stream.
        // `step` = the number of the lockstep iteration = the iteration count of every chain that has not finished (every launch pair advances
        // each of them by one): a kernel argument, because the search block of the selection must not read a field its sibling writes
        // DA4ML_HIP_STATS=1: k_iter_update tallies the blocks it finds / creates / deletes (da_timings' found / inserts, the "peak pair blocks" of da_result_stats);
        // read at every call, so that a benchmark can count on one pass and time the others
        const char *stats_env = std::getenv("DA4ML_HIP_STATS");
        const bool with_stats = stats_env && std::atoi(stats_env) != 0;
        auto launch_pair = [&](const Group &gr, hipEvent_t *se, int step) {
            ChainDev *base = d_desc + gr.first;
            const dim3 sel_grid((gr.count + 7) & ~7, 2);  // y = 0 search block, y = 1 substitution block
            // (+ 2: the last two blocks of a chain write the six blocks of the pairs among the modified rows)
            const dim3 upd_grid((gr.count + 7) & ~7, upd_blocks[gr.w] + 2);
            with_sel2(ranges[gr.w].wide, ranges[gr.w].manycol, ranges[gr.w].seeded, [&](auto c, auto mc, auto sd) {
                using Cell = decltype(c);
                constexpr bool SEEDED = decltype(sd)::value;
                if (se) HIP_CHECK(hipEventRecord(se[0], gr.stream));
                hipLaunchKernelGGL((k_iter_select2<Cell, false, decltype(mc)::value, SEEDED>), sel_grid, dim3(SEL2_THREADS), sel_lds[gr.w], gr.stream, base, gr.count, im.d_done, step);
                if (se) HIP_CHECK(hipEventRecord(se[1], gr.stream));
                with_flag(with_stats, [&](auto s) {
                    with_flag(ranges[gr.w].weighted, [&](auto wt) {
                        constexpr bool WEIGHTED = decltype(wt)::value;
                        with_flag(SEEDED && WEIGHTED && ranges[gr.w].slack, [&](auto sl) {
                            constexpr bool SLACK = SEEDED && WEIGHTED && decltype(sl)::value;  // (the slack kernels exist with a seed and a carried weight only)
                            hipLaunchKernelGGL((k_iter_update<Cell, decltype(s)::value, SEEDED, WEIGHTED, SLACK>), upd_grid, dim3(UPD_THREADS), upd_lds[gr.w], gr.stream, base, gr.count);
                        });
                    });
                });
                if (se) HIP_CHECK(hipEventRecord(se[2], gr.stream));
            });
        };
        // Windows of up to WINDOW_ITERS iterations x all groups are queued eagerly; one event-bracketed iteration per window
        // samples the kernel durations.  (A hipGraph replay of the window was re-measured in round 2: no gain.)
        constexpr int WINDOW_ITERS = 63, MAX_SAMPLES = 4096;
        long long iter_cap = 0;
        int active = n;  // chains that have not finished: those with a method that takes no step never start
        for (int i = 0; i < n; ++i) {
            iter_cap = std::max<long long>(iter_cap, geo[i].rcap - jobs[i].n_in + 2);
            active -= desc[i].done ? 1 : 0;
        }
        const int poll_every = WINDOW_ITERS + 1, pre_done = n - active;
        // The done counter is read back ONE WINDOW BEHIND on a separate stream: after window w is queued, the poll stream
        // waits for every group's end-of-window event and copies the counter; the host looks at the copy of window w-1 only
        // after window w has been queued, so the queues never drain while the host decides whether to go on.
        std::vector<hipEvent_t> win_ev[2];  // (one per group: a batch can hold more kernel variants than there are streams)
        hipEvent_t copy_ev[2];
        for (int p = 0; p < 2; ++p) {
            copy_ev[p] = events.make(hipEventDisableTiming);
            win_ev[p].resize(groups.size());
            for (size_t gi = 0; gi < groups.size(); ++gi) win_ev[p][gi] = events.make(hipEventDisableTiming);
        }
        im.h_done[0] = im.h_done[1] = 0;
        long long window = 0;
        struct DrainOnError {  // an exception between here and the end of the loop leaves launches queued: let them finish before the arena is reused
            const std::vector<Group> &g;
            hipStream_t poll;
            bool armed = true;
            ~DrainOnError() {
                if (!armed) return;
                for (const Group &gr : g) (void)hipStreamSynchronize(gr.stream);
                (void)hipStreamSynchronize(poll);
            }
        } drain{groups, im.poll_stream};
        // A second launching thread takes every other chain group: with the shorter kernels of round 5 one thread queueing all launches
        // (2.85 us each, 8 per lockstep iteration of 4 groups) is the bound for small problems (64x64: 22.9 of 24.6 us per iteration, measured).
        // It follows the windows of this thread: (first step, iterations) in, its groups' end-of-window events recorded out.
        struct Helper {
            std::atomic<long long> seq{0}, ack{0};
            std::atomic<bool> quit{false};
            long long first_step = 0;
            int iters = 0, parity = 0;
            std::exception_ptr err;
            std::thread th;
        } helper;
        const bool two_threads = im.launch_threads >= 2 && groups.size() >= 2;
        static_assert(Impl::MAX_LANES % 2 == 0, "groups gi and gi + MAX_LANES share a stream: they must be queued by the same launching thread (gi & 1)");
        auto mine = [&](size_t gi, int who) { return !two_threads || (int)(gi & 1) == who; };
        auto window_launches = [&](int who, long long first_step, int iters, int parity, hipEvent_t *se0) {
            for (int it = 0; it < iters; ++it)
                for (size_t gi = 0; gi < groups.size(); ++gi)
                    if (mine(gi, who)) launch_pair(groups[gi], it == 0 && gi == 0 ? se0 : nullptr, (int)(first_step + it));
            HIP_CHECK(hipGetLastError());
            for (size_t gi = 0; gi < groups.size(); ++gi)
                if (mine(gi, who)) HIP_CHECK(hipEventRecord(win_ev[parity][gi], groups[gi].stream));
        };
        if (two_threads)
            helper.th = std::thread([&] {
                long long seen = 0;
                try {
                    HIP_CHECK(hipSetDevice(im.device));
                    while (true) {
                        long long s;
                        unsigned polls = 0;
                        while ((s = helper.seq.load(std::memory_order_acquire)) == seen && !helper.quit.load(std::memory_order_acquire)) spin_wait_step(polls);
                        if (s == seen) break;
                        seen = s;
                        if (!helper.err) window_launches(1, helper.first_step, helper.iters, helper.parity, nullptr);
                        helper.ack.store(seen, std::memory_order_release);
                    }
                } catch (...) {
                    helper.err = std::current_exception();
                    helper.ack.store(helper.seq.load(), std::memory_order_release);  // (whatever window was being served: the main thread rethrows)
                    unsigned polls = 0;
                    while (!helper.quit.load(std::memory_order_acquire)) {  // keep acknowledging until told to leave
                        helper.ack.store(helper.seq.load(), std::memory_order_release);
                        spin_wait_step(polls);
                    }
                }
            });
        struct JoinHelper {
            Helper &h;
            ~JoinHelper() {
                h.quit.store(true, std::memory_order_release);
                if (h.th.joinable()) h.th.join();
            }
        } join_helper{helper};
        while (active > 0) {
            const auto t_q0 = std::chrono::steady_clock::now();
            if (launched_iters > iter_cap + 2 * poll_every) throw std::runtime_error("greedy loop did not terminate within its row capacity (internal error)");
            // small problems finish within a few iterations: start with short windows, double up to the full length
            const int this_window = (int)std::min<long long>(WINDOW_ITERS, (8ll << std::min<long long>(window, 8)) - 1);
            const int p = (int)(window & 1);
            if (two_threads) {
                helper.first_step = launched_iters, helper.iters = this_window + 1, helper.parity = p;
                helper.seq.fetch_add(1, std::memory_order_release);
            }
            // the first iteration of a window is the sampled one: the first group's kernels are bracketed by events on its stream
            hipEvent_t se[3];
            const bool sample = sample_ev.size() < (size_t)3 * MAX_SAMPLES;
            if (sample)
                for (auto &e : se) {
                    e = events.make();
                    sample_ev.push_back(e);
                }
            window_launches(0, launched_iters, this_window + 1, p, sample ? se : nullptr);
            launched_iters += this_window + 1;
            if (two_threads) {
                const long long want = helper.seq.load(std::memory_order_relaxed);
                unsigned polls = 0;
                while (helper.ack.load(std::memory_order_acquire) != want) spin_wait_step(polls);
                if (helper.err) std::rethrow_exception(helper.err);
            }
            for (size_t gi = 0; gi < groups.size(); ++gi) HIP_CHECK(hipStreamWaitEvent(im.poll_stream, win_ev[p][gi], 0));
            HIP_CHECK(hipMemcpyAsync(&im.h_done[p], im.d_done, sizeof(unsigned int), hipMemcpyDeviceToHost, im.poll_stream));
            HIP_CHECK(hipEventRecord(copy_ev[p], im.poll_stream));
            host_launch_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_q0).count();
            if (window > 0) {
                HIP_CHECK(hipEventSynchronize(copy_ev[p ^ 1]));
                active = n - pre_done - (int)im.h_done[p ^ 1];
            }
            ++window;
        }
        for (const Group &gr : groups) HIP_CHECK(hipStreamSynchronize(gr.stream));
        HIP_CHECK(hipStreamSynchronize(im.poll_stream));
        drain.armed = false;
        HIP_CHECK(hipEventRecord(ev1, st));
    }

    // ---- 5. extraction, the final descriptors and the loop's clocks; every outs[] reset to what its chain reports.  True: some chain outgrew its arena
    bool extract() {
        for (int w = 0; w < N_VAR; ++w) {
            const Range &r = ranges[w];
            if (r.count == 0) continue;
            const dim3 colgrid((max_n_out + 3) / 4, r.count);
            with_cell(r.wide, [&](auto c) { hipLaunchKernelGGL(k_extract<decltype(c)>, colgrid, dim3(256), 0, st, d_desc + r.first); });
        }
        hipLaunchKernelGGL(k_pack, dim3(n), dim3(256), 0, st, d_desc);
        HIP_CHECK(hipGetLastError());
        fin.resize(n);
        HIP_CHECK(hipMemcpyAsync(fin.data(), d_desc, sizeof(ChainDev) * (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipEventElapsedTime(&loop_ms, ev0, ev1));
        const int n_samples = (int)(sample_ev.size() / 3);
        for (int k = 0; k < n_samples; ++k) {
            float a = 0, b = 0;
            HIP_CHECK(hipEventElapsedTime(&a, sample_ev[3 * k], sample_ev[3 * k + 1]));
            HIP_CHECK(hipEventElapsedTime(&b, sample_ev[3 * k + 1], sample_ev[3 * k + 2]));
            im.timings.select_ms_sampled += a;
            im.timings.update_ms_sampled += b;
        }
        im.timings.samples += n_samples;
        im.timings.sampled_chain_launches += (double)n_samples * sampled_chains;
        bool need_retry = false;
        for (int s = 0; s < n; ++s) {
            fill_result(outs[order[s]], fin[s]);
            need_retry |= fin[s].error == E_TABLE_CAPACITY || fin[s].error == E_ROW_CAPACITY;
        }
        return need_retry;
    }

    // ---- 6. Results: the seven arrays of every chain (column offsets, shifts, picks, row latencies, surviving digits) are gathered
    // into one contiguous device buffer by k_gather and leave in ONE copy into pinned memory (they used to leave one by one:
    // 448 copies per 64-chain batch in two synchronised phases).
    void download() {
        struct ResultOffsets {
            size_t st, s0, s1, pk, lat, row, cell;
            uint32_t total;
        };
        std::vector<ResultOffsets> roff(n);
        pieces.reserve((size_t)n * 7);
        size_t gather_bytes = 0;
        auto piece = [&](const void *src, size_t bytes) {
            const size_t at = gather_bytes;
            if (bytes) pieces.push_back(GatherPiece{src, (unsigned long long)at, (unsigned long long)bytes});
            gather_bytes += align_up(bytes, 64);
            return at;
        };
        for (int s = 0; s < n; ++s) {
            const ChainDev &d = fin[s];
            const ChainJob &j = jobs[order[s]];
            ResultOffsets &ro = roff[s];
            ro.total = d.error == E_OK ? d.pk_total : 0u;  // a failed chain delivers no digits (finalize_chain raises for it)
            ro.st = piece(d.fin_start, ((size_t)j.n_out + 1) * 4);
            ro.s0 = piece(d.shift0, (size_t)j.n_in);
            ro.s1 = piece(d.shift1, (size_t)j.n_out);
            ro.pk = piece(d.picks, (size_t)d.iter * sizeof(int4));
            ro.lat = piece(d.pk_lat, (size_t)d.n_rows * 4);
            ro.row = piece(d.pk_row, (size_t)ro.total * 4);
            ro.cell = piece(d.pk_cell, (size_t)ro.total * 8);
        }
        unsigned char *pin = static_cast<unsigned char *>(im.pinned.get(std::max<size_t>(gather_bytes, 64)));
        unsigned char *gbuf = static_cast<unsigned char *>(im.gather_buf.get(std::max<size_t>(gather_bytes, 64)));
        GatherPiece *d_pieces = static_cast<GatherPiece *>(im.piece_buf.get(std::max<size_t>(pieces.size(), 1) * sizeof(GatherPiece)));
        HIP_CHECK(hipMemcpyAsync(d_pieces, pieces.data(), pieces.size() * sizeof(GatherPiece), hipMemcpyHostToDevice, st));
        for (size_t first = 0; first < pieces.size(); first += 32768) {  // grid.y is a 16-bit quantity
            const unsigned cnt = (unsigned)std::min<size_t>(32768, pieces.size() - first);
            hipLaunchKernelGGL(k_gather, dim3(16, cnt), dim3(256), 0, st, d_pieces + first, gbuf);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(pin, gbuf, gather_bytes, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        // out of the pinned buffer into the result vectors: the chains on a few host threads (45 MB per 64-chain batch)
        parallel_for(n, gather_bytes, [&](int s) {
            const ChainDev &d = fin[s];
            const ChainJob &j = jobs[order[s]];
            const ResultOffsets &ro = roff[s];
            ChainOut &o = outs[order[s]];
            const uint32_t *cs = reinterpret_cast<const uint32_t *>(pin + ro.st);
            o.col_start.assign(cs, cs + j.n_out + 1);
            o.shift0.assign(reinterpret_cast<const int8_t *>(pin + ro.s0), reinterpret_cast<const int8_t *>(pin + ro.s0) + j.n_in);
            o.shift1.assign(reinterpret_cast<const int8_t *>(pin + ro.s1), reinterpret_cast<const int8_t *>(pin + ro.s1) + j.n_out);
            const int32_t *pk = reinterpret_cast<const int32_t *>(pin + ro.pk);
            o.picks.assign(pk, pk + (size_t)d.iter * 4);
            const float *lat = reinterpret_cast<const float *>(pin + ro.lat);
            o.row_lat.assign(lat, lat + d.n_rows);
            const uint32_t *pr = reinterpret_cast<const uint32_t *>(pin + ro.row);
            const unsigned long long *pc = reinterpret_cast<const unsigned long long *>(pin + ro.cell);
            o.dig_row.assign(pr, pr + ro.total);
            o.dig_cell.assign(pc, pc + ro.total);
        });
    }

    // ---- 7. the call into the backend's timings (a call that hands its chains to other calls -- halves, a retry -- does not get here)
    void account() {
        GpuTimings &tm = im.timings;
        for (int s = 0; s < n; ++s) {
            const ChainDev &d = fin[s];
            for (int q = 0; q < 12; ++q) tm.phase_cycles[q] += (double)d.st_phase[q];
            for (int q = 0; q < 4; ++q) tm.search_cycles[q] += (double)d.st_qphase[q];
            tm.search_diag[0] += (double)d.st_qdiag[0], tm.search_diag[1] += (double)d.st_qdiag[1], tm.search_diag[2] += (double)d.st_qdiag[4];
            tm.search_diag[3] += (double)d.st_qdiag[5], tm.search_diag[4] = std::max(tm.search_diag[4], (double)d.st_qdiag[6]), tm.search_diag[5] += (double)d.st_qdiag[7], tm.search_diag[6] += (double)d.st_qdiag[8];
            tm.fast_steps += (long long)d.st_fast;
            tm.found += (long long)d.st_found;
            tm.inserts += (long long)d.st_inserts;
            tm.cell_reads += (long long)d.st_cells;
            tm.key_bytes += 2.0 * d.K * (double)(d.st_found + d.st_inserts);
            tm.cell_bytes += (geo[order[s]].wide ? 8.0 : 4.0) * (double)d.st_cells;
            tm.iterations += d.iter;
            tm.rescans += (long long)d.st_rescans;
            // + the search block: bound, flags, tie word and lowered-value mark of every group per step (28 B), and per re-read group its ranks and ~2 slots' key and index
            tm.select_bytes += (double)d.st_sel_bytes + 32.0 * (double)d.n_groups * (double)d.iter + (double)d.st_rescans * ((double)(4u << d.gs_log2) + 24.0);
            tm.partners += (long long)d.st_partners;
            tm.table_bytes += (double)d.C * (8.0 + 4.0 + (double)(1 << d.pb_log2));
        }
        tm.loop_ms += loop_ms;
        tm.host_launch_ms += host_launch_ms;
        tm.lockstep_iters += launched_iters;
        tm.chains += n;
        for (int i = 0; i < n; ++i) tm.manycol_chains += manycol[i] ? 1 : 0;
        tm.arena_bytes = std::max(tm.arena_bytes, (double)arena_bytes);
    }
};

// Runs the chains of a batch to completion: the phases of Impl::Batch, and the two ways a call hands its chains on to other calls.
void HipBackend::run_chains(const ChainJob *jobs, ChainOut *outs, int n) {
    if (n <= 0) return;
    Impl &im = *impl_;
    HIP_CHECK(hipSetDevice(im.device));
    auto t_begin = std::chrono::steady_clock::now();
    const bool verbose = std::getenv("DA4ML_HIP_VERBOSE") != nullptr;
    auto lap = [&, last = t_begin](const char *what) mutable {
        auto now = std::chrono::steady_clock::now();
        if (verbose) std::fprintf(stderr, "[da4ml_hip] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    };
    Impl::Batch b(im, jobs, outs, n);
    b.upload_and_prepare();
    lap("upload + k_prepare");
    b.plan(row_scale_);
    // a batch whose arena does not fit into (most of) the free device memory is processed in two halves
    if (b.arena_bytes > b.budget) {
        if (n == 1)
            throw std::runtime_error("a single chain needs " + std::to_string(b.arena_bytes >> 20) + " MiB of device memory (pair table of " +
                                     std::to_string(b.geo[0].C) + " slots), " + std::to_string(b.free_b >> 20) + " MiB are free (budget " +
                                     std::to_string(b.budget >> 20) + " MiB)");
        const int half_n = n / 2;
        run_chains(jobs, outs, half_n);
        run_chains(jobs + half_n, outs + half_n, n - half_n);
        return;
    }
    b.init_chains();
    lap("arena + init kernels");
    b.greedy_loop();
    lap("greedy loop");
    if (b.extract() && retry_depth_ < 4) {
        // some chain outgrew its arena: rerun the whole group with larger capacities (rare; sizes are heuristics)
        struct Restore {  // however the rerun ends
            double &table_scale, &row_scale;
            int &depth;
            const double keep_t = table_scale, keep_r = row_scale;
            ~Restore() {
                table_scale = keep_t;
                row_scale = keep_r;
                --depth;
            }
        } restore{im.table_scale, row_scale_, retry_depth_};
        ++retry_depth_;
        im.timings.retries += 1;
        im.table_scale *= 4.0;
        row_scale_ *= 4.0;
        run_chains(jobs, outs, n);
        return;
    }
    b.download();
    b.account();
    lap("extract + download + unpack");
    im.timings.total_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
}
