// hip_stage01.h -- stage-0/1 entry points of HipBackend (column_distances, int_to_csd, csd_decompose) and device_count.
// Host code of the HIP backend: cmvm_engine.hip includes it after the kernels, inside namespace da::gpu; nothing else may.
#pragma once
#ifndef DA_ENGINE_TU
#error "hip_stage01.h is a part of cmvm_engine.hip"
#endif

void HipBackend::column_distances(const int32_t *aug, int n_in, int W, int64_t *d0, int64_t *d1) {
    Impl &im = *impl_;
    HIP_CHECK(hipSetDevice(im.device));
    hipStream_t st = im.stream;
    size_t a_bytes = align_up((size_t)n_in * W * 4, 256), d_bytes = align_up((size_t)W * W * 8, 256);
    unsigned char *buf = static_cast<unsigned char *>(im.io_buf.get(a_bytes + 2 * d_bytes));
    HIP_CHECK(hipMemcpyAsync(buf, aug, (size_t)n_in * W * 4, hipMemcpyHostToDevice, st));
    auto *dd0 = reinterpret_cast<long long *>(buf + a_bytes), *dd1 = reinterpret_cast<long long *>(buf + a_bytes + d_bytes);
    EventGuard events;
    hipEvent_t e0 = events.make(), e1 = events.make();
    HIP_CHECK(hipEventRecord(e0, st));
    hipLaunchKernelGGL(k_col_dist, dim3((W + 15) / 16, (W + 15) / 16), dim3(16, 16), 0, st, reinterpret_cast<const int32_t *>(buf), n_in, W, dd0, dd1);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(e1, st));
    HIP_CHECK(hipMemcpyAsync(d0, dd0, (size_t)W * W * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(d1, dd1, (size_t)W * W * 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    im.timings.dist_ms += ms;
    im.timings.dist_calls += 1;
}

int HipBackend::int_to_csd(const int32_t *x, int64_t n, std::vector<int8_t> &csd) {
    Impl &im = *impl_;
    HIP_CHECK(hipSetDevice(im.device));
    hipStream_t st = im.stream;
    size_t xb = align_up(std::max<size_t>((size_t)n * 4, 4), 256);
    // two-step: global |max| -> N, then the digits
    unsigned char *buf = static_cast<unsigned char *>(im.io_buf.get(xb + 256 + (size_t)n * 33));
    auto *dx = reinterpret_cast<int32_t *>(buf);
    auto *dmax = reinterpret_cast<unsigned int *>(buf + xb);
    auto *dout = reinterpret_cast<int8_t *>(buf + xb + 256);
    HIP_CHECK(hipMemcpyAsync(dx, x, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(dmax, 0, 4, st));
    unsigned int mx = 0;
    if (n > 0) {
        int blocks = (int)std::min<int64_t>(1024, (n + 255) / 256);
        hipLaunchKernelGGL(k_absmax, dim3(blocks), dim3(256), 0, st, dx, (long long)n, dmax);
        HIP_CHECK(hipMemcpyAsync(&mx, dmax, 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    int N = csd_width(mx);
    csd.assign((size_t)n * N, 0);
    if (n > 0) {
        hipLaunchKernelGGL(k_naf_digits, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dx, (long long)n, N, dout);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(csd.data(), dout, (size_t)n * N, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    }
    return N;
}

int HipBackend::csd_decompose(const float *kernel, int n_in, int n_out, bool center, std::vector<int8_t> &csd,
                              std::vector<int8_t> &s0, std::vector<int8_t> &s1) {
    // centring on the device through k_prepare of a one-chain batch, then the digit kernel
    Impl &im = *impl_;
    HIP_CHECK(hipSetDevice(im.device));
    hipStream_t st = im.stream;
    size_t e = (size_t)n_in * n_out;
    std::vector<int32_t> xi(e);
    if (center) {
        const InputLayout L = input_layout(n_in, n_out, false);  // (no latencies: k_prepare does not read them)
        unsigned char *buf = static_cast<unsigned char *>(im.io_buf.get(L.bytes + 512));
        ChainDev d;
        std::memset(&d, 0, sizeof d);
        d.n_in = n_in;
        d.n_out = n_out;
        d.pn_out = n_out;
        d.kernel = reinterpret_cast<const float *>(buf + L.kernel);
        d.qints = reinterpret_cast<const float *>(buf + L.qints);
        d.xint = reinterpret_cast<int32_t *>(buf + L.xint);
        d.shift0 = reinterpret_cast<int8_t *>(buf + L.shift0);
        d.shift1 = reinterpret_cast<int8_t *>(buf + L.shift1);
        std::vector<float> ones((size_t)n_in * 3, 1.0f);  // no row is treated as dead here
        HIP_CHECK(hipMemcpyAsync(buf + L.kernel, kernel, e * 4, hipMemcpyHostToDevice, st));
        HIP_CHECK(hipMemcpyAsync(buf + L.qints, ones.data(), ones.size() * 4, hipMemcpyHostToDevice, st));
        ChainDev *dd = static_cast<ChainDev *>(im.desc_buf.get(sizeof(ChainDev)));
        HIP_CHECK(hipMemcpyAsync(dd, &d, sizeof d, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_prepare, dim3(1), dim3(256), (size_t)n_out * 4, st, dd);
        HIP_CHECK(hipGetLastError());
        s0.resize(n_in);
        s1.resize(n_out);
        HIP_CHECK(hipMemcpyAsync(xi.data(), d.xint, e * 4, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s0.data(), d.shift0, n_in, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(s1.data(), d.shift1, n_out, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
    } else {
        s0.assign(n_in, 0);
        s1.assign(n_out, 0);
        for (size_t k = 0; k < e; ++k) xi[k] = (int32_t)kernel[k];
    }
    return int_to_csd(xi.data(), (int64_t)e, csd);
}

int device_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
