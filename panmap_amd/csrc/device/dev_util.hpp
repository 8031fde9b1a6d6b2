// Host-side helpers for the device translation units: error plumbing, RAII device buffers, context.
#pragma once
#include "pmx_options.hpp"
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <exception>
#include <map>
#include <string>
#include <vector>

#include "../api_internal.hpp"

namespace pmx {

struct HipError {
    std::string msg;
};

#define PMX_HIP(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            throw pmx::HipError{std::string(#expr) + ": " + hipGetErrorString(_e)};                        \
    } while (0)

// the C ABI's way out of an entry point: the message for pmx_last_error, the code for the caller; PMX_TRY ... PMX_CATCH
// around an entry point's body turn what it throws into PMX_ERR_DEVICE
inline int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}
#define PMX_TRY try {
#define PMX_CATCH                                                               \
    }                                                                           \
    catch (const pmx::HipError& e) { return pmx::fail(PMX_ERR_DEVICE, e.msg); } \
    catch (const std::exception& e) { return pmx::fail(PMX_ERR_DEVICE, e.what()); }

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    bool owned = true;
    DevBuf() {}
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && owned) (void)hipFree(p);
        p = nullptr;
        n = 0;
        owned = true;
    }
    void alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        PMX_HIP(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
    }
    void ensure(size_t count) {
        if (count > n) alloc(count);
    }
    void wrap(T* ptr, size_t count) {
        release();
        p = ptr;
        n = count;
        owned = false;
    }
    void swap(DevBuf& o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(owned, o.owned);
    }
};

// rocprim's two-call protocol: `call(storage, bytes)` with no storage reports the temporary bytes it needs, `tmp` grows to
// them, the second call does the work.  PMX_ROCPRIM(tmp, algorithm, arguments...) binds everything behind rocprim's first
// two parameters, written once: PMX_ROCPRIM(pl->tmp, radix_sort_pairs, keys_in, keys_out, vals_in, vals_out, n, 0, 64, stream).
// (The macro is for translation units that include rocprim; this header does not.)
template <class Call>
inline void rocprim_two_calls(DevBuf<char>& tmp, Call call) {
    size_t bytes = 0;
    PMX_HIP(call((void*)nullptr, bytes));
    tmp.ensure(bytes);
    PMX_HIP(call((void*)tmp.p, bytes));
}
#define PMX_ROCPRIM(tmp, algorithm, ...) \
    pmx::rocprim_two_calls(tmp, [&](void* storage_, size_t& bytes_) { return rocprim::algorithm(storage_, bytes_, __VA_ARGS__); })

// A stream with a HARDWARE queue of its own.  HIP multiplexes ordinary streams onto a few hardware queues
// (GPU_MAX_HW_QUEUES, 4 by default); streams that land on one queue execute strictly in submission order: kernels of two
// contexts then never overlap, and a kernel queued behind the barrier packet of a long host-to-device copy of ANOTHER stream
// waits for that copy.  A stream created with a CU mask gets its own queue; the mask enables every CU.
inline hipStream_t create_dedicated_stream(int n_cu) {
    hipStream_t st = nullptr;
    if (n_cu > 0) {
        std::vector<uint32_t> mask((size_t)(n_cu + 31) / 32, 0xffffffffu);
        if (n_cu % 32) mask.back() = (1u << (n_cu % 32)) - 1u;
        if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
            (void)hipGetLastError();
            st = nullptr;
        }
    }
    if (!st) PMX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    return st;
}

struct KernelTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int launches = 0;
    bool pending = false;
    bool summed = false;   // a span in pieces (timer_sum_*): sum_ms is its duration
    double sum_ms = 0.0;
};

}  // namespace pmx

struct pmx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::map<std::string, pmx::KernelTimer> timers;
    int n_cu = 256;
    // Side streams of the seeding stage (hardware queues of their own, see create_dedicated_stream) and the events that order
    // them against the context's stream.  They belong to the CONTEXT, made on first use and kept until it is destroyed: a
    // placer that made and destroyed its own left the next placer's kernels on a recycled queue hanging (round 4).
    hipStream_t pair_stream = nullptr;       // pmx_readset_order_pairs
    hipStream_t seed_streams[3] = {nullptr, nullptr, nullptr};
    hipEvent_t seed_go = nullptr, seed_done[3] = {nullptr, nullptr, nullptr};
};

namespace pmx {
inline void timer_begin(pmx_ctx* ctx, const char* name) {
    KernelTimer& t = ctx->timers[name];
    if (!t.e0) { PMX_HIP(hipEventCreate(&t.e0)); PMX_HIP(hipEventCreate(&t.e1)); }
    PMX_HIP(hipEventRecord(t.e0, ctx->stream));
}
inline void timer_end(pmx_ctx* ctx, const char* name, int launches) {
    KernelTimer& t = ctx->timers[name];
    PMX_HIP(hipEventRecord(t.e1, ctx->stream));
    t.launches = launches;
    t.pending = true;
}
// "No such span in this call": what an earlier call recorded under `name` is not reported again (pmx_last_kernel_ms < 0).
inline void timer_cancel(pmx_ctx* ctx, const char* name) {
    if (auto t = ctx->timers.find(name); t != ctx->timers.end()) t->second.pending = false;
}
// A span made of several pieces with host work between them (the chunks of pmx_meta_assign): timer_sum_reset, then per piece
// timer_begin / timer_end and, once the stream was synchronized, timer_sum_add; pmx_last_kernel_ms reports the sum.
inline void timer_sum_reset(pmx_ctx* ctx, const char* name) {
    KernelTimer& t = ctx->timers[name];
    t.summed = true;
    t.sum_ms = 0.0;
}
inline void timer_sum_add(pmx_ctx* ctx, const char* name) {
    KernelTimer& t = ctx->timers[name];
    float ms = 0.f;
    PMX_HIP(hipEventElapsedTime(&ms, t.e0, t.e1));
    t.sum_ms += (double)ms;
}
inline int grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}
}  // namespace pmx
