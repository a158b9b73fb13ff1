// hip_host_util.h -- HIP_CHECK, grow-only device / pinned buffers, event guard, arena carver, cell-type dispatch, parallel_for.
// Host code of the HIP backend: cmvm_engine.hip includes it after the kernels, inside namespace da::gpu; nothing else may.
#pragma once
#ifndef DA_ENGINE_TU
#error "hip_host_util.h is a part of cmvm_engine.hip"
#endif

#define HIP_CHECK(expr)                                                                                          \
    do {                                                                                                         \
        hipError_t _e = (expr);                                                                                  \
        if (_e != hipSuccess)                                                                                    \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(_e) + " at " #expr);         \
    } while (0)

namespace {

struct DeviceBuffer {  // grow-only device allocation reused across calls
    void *ptr = nullptr;
    size_t cap = 0;
    void *get(size_t bytes) {
        if (bytes > cap) {
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr;
            cap = 0;
            size_t want = bytes + bytes / 8;
            HIP_CHECK(hipMalloc(&ptr, want));
            cap = want;
        }
        return ptr;
    }
    ~DeviceBuffer() {
        if (ptr) (void)hipFree(ptr);
    }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// spin-wait step of the two launch threads' hand-shake: a pause for the first few thousand polls (the partner answers within microseconds while both are
// queueing launches), then the core is given up between polls -- the waits that last (the main thread waiting for the device, the helper between
// windows) must not hold a core at 100 % (ranks of one host share its cores)
inline void spin_wait_step(unsigned &polls) {
    if (++polls < 4096u) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#elif defined(__aarch64__)
        asm volatile("yield");
#endif
    } else if (polls < 8192u)
        std::this_thread::yield();
    else
        std::this_thread::sleep_for(std::chrono::microseconds(50));
}

// Events of one call, destroyed however the call ends (a HIP error or the termination guard of the greedy loop used to leak
// the timing, window and sample events of the call -- up to 12 k of them).
struct EventGuard {
    std::vector<hipEvent_t> all;
    hipEvent_t make(unsigned flags = 0) {
        hipEvent_t e = nullptr;
        HIP_CHECK(flags ? hipEventCreateWithFlags(&e, flags) : hipEventCreate(&e));
        all.push_back(e);
        return e;
    }
    ~EventGuard() {
        for (hipEvent_t e : all) (void)hipEventDestroy(e);
    }
};

struct Carver {  // bump allocator over the arena; first pass sizes, second pass assigns
    unsigned char *base;
    size_t off = 0;
    explicit Carver(unsigned char *b) : base(b) {}
    template <class T> T *take(size_t count) {
        off = align_up(off, 256);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

}  // namespace

struct PinnedBuffer {  // grow-only pinned host allocation reused across calls
    void *ptr = nullptr;
    size_t cap = 0;
    void *get(size_t bytes) {
        if (bytes > cap) {
            if (ptr) (void)hipHostFree(ptr);
            ptr = nullptr;
            cap = 0;
            size_t want = bytes + bytes / 4 + 4096;
            HIP_CHECK(hipHostMalloc(&ptr, want, hipHostMallocDefault));
            cap = want;
        }
        return ptr;
    }
    ~PinnedBuffer() {
        if (ptr) (void)hipHostFree(ptr);
    }
};

namespace {

// `wide` (and a flag) as template arguments: f is called with a value of the cell type (with std::true_type / std::false_type)
template <class F> void with_cell(bool wide, F &&f) {
    if (!wide)
        f(uint32_t{});
    else
        f(uint64_t{});
}
template <class F> void with_flag(bool on, F &&f) {
    if (!on)
        f(std::false_type{});
    else
        f(std::true_type{});
}

// f(0) .. f(n - 1) on a few host threads, the caller among them: min(n, 8, one per MiB of `bytes` moved); the first exception is rethrown here
template <class F> void parallel_for(int n, size_t bytes, F &&f) {
    const int workers = (int)std::min<size_t>({(size_t)n, (size_t)8, bytes / (1u << 20) + 1});
    std::atomic<int> next{0};
    std::exception_ptr err;
    std::mutex err_mu;
    auto work = [&] {
        try {
            for (int i = next++; i < n; i = next++) f(i);
        } catch (...) {
            std::lock_guard<std::mutex> lk(err_mu);
            if (!err) err = std::current_exception();
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < workers; ++t) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    if (err) std::rethrow_exception(err);
}

}  // namespace
