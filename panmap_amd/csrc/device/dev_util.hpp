// Host-side helpers for the device translation units: error plumbing, RAII device buffers, context.
#pragma once
#include "pmx_options.hpp"
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <exception>
#include <map>
#include <string>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../api_internal.hpp"

namespace pmx {

struct HipError {
    std::string msg;
};

#define PMX_HIP_AT(what, expr)                                                                             \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            throw pmx::HipError{std::string(what) + ": " + hipGetErrorString(_e)};                         \
    } while (0)
#define PMX_HIP(expr) PMX_HIP_AT(#expr, expr)

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

// ---- Launches, copies and clears.  Nothing else under csrc calls the runtime for these. ----
//
// PMX_LAUNCH(kernel, grid, block, lds_bytes, stream, arguments...) launches and checks: a launch that the runtime refuses
// throws HipError with the kernel named.  The parameter types come from the kernel pointer alone, so the arguments convert
// at the call site as they would in a direct call; a kernel template with commas in its arguments goes in parentheses.
template <class T>
struct same_type { using type = T; };
template <class... P>
inline void launch(const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t st,
                   const typename same_type<P>::type&... args) {
    hipLaunchKernelGGL(kernel, grid, block, lds_bytes, st, args...);
    PMX_HIP_AT(std::string("launch of ") + name, hipGetLastError());
}
#define PMX_LAUNCH(kernel, ...) pmx::launch(#kernel, kernel, __VA_ARGS__)

// The device end of a copy or clear: a DevBuf (from its start), pmx::at(buf, offset), or a raw device pointer that came in
// through the C ABI.  The first two know how many elements lie behind them and the count is checked against that on the
// host, before the runtime is called; a raw pointer is taken on trust (`void*` too: the host end then gives the type).
constexpr size_t kUnsized = ~(size_t)0;
template <class T>
struct DevSpan {
    T* p;
    size_t room;
};
template <class T>
inline DevSpan<T> at(DevBuf<T>& b, size_t offset) { return {b.p + offset, offset <= b.n ? b.n - offset : 0}; }
template <class T>
inline DevSpan<const T> at(const DevBuf<T>& b, size_t offset) { return {b.p + offset, offset <= b.n ? b.n - offset : 0}; }
// a byte buffer that holds elements of U
template <class U, class T>
inline DevSpan<U> as(DevBuf<T>& b) { return {reinterpret_cast<U*>(b.p), b.n * sizeof(T) / sizeof(U)}; }

namespace detail {
template <class T> inline DevSpan<T> span(DevBuf<T>& b) { return {b.p, b.n}; }
template <class T> inline DevSpan<const T> span(const DevBuf<T>& b) { return {b.p, b.n}; }
template <class T> inline DevSpan<T> span(DevSpan<T> s) { return s; }
template <class T> inline DevSpan<T> span(T* p) { return {p, kUnsized}; }
template <class T> inline constexpr size_t elem_size = sizeof(T);
template <> inline constexpr size_t elem_size<void> = 0;   // void*: the other end gives the type
template <> inline constexpr size_t elem_size<const void> = 0;
// the device pointer of `n` elements of the host's type H, or a throw that names the buffer expression
template <class H, class D>
inline D* checked(const char* what, DevSpan<D> s, size_t n) {
    static_assert(elem_size<D> == 0 || elem_size<D> == sizeof(H), "host and device elements differ in size");
    if (s.room != kUnsized && n > s.room)
        throw HipError{std::string(what) + ": " + std::to_string(n) + " elements asked of the " + std::to_string(s.room) + " behind it"};
    return s.p;
}
template <class H>
inline void fits(const char* what, const std::vector<H>& v, size_t n) {
    if (n > v.size()) throw HipError{std::string(what) + ": " + std::to_string(n) + " elements against a host vector of " + std::to_string(v.size())};
}
template <class... A>
inline hipStream_t stream_of(A&&... a) { return std::get<sizeof...(A) - 1>(std::forward_as_tuple(a...)); }
}  // namespace detail

// Counts are in elements; a count of zero does nothing.  PMX_H2D(device, host, [n,] stream): `host` is a pointer with n,
// a vector (all of it, or its first n) or a fixed array.  PMX_D2H(host, device, [n,] stream) likewise; PMX_D2H_SYNC also
// waits for the stream.  PMX_D2D(to, from, n, stream); PMX_ZERO(device, n, stream); PMX_FILL(device, byte, n, stream).
template <class H, class Dst>
inline void h2d(const char* what, Dst&& dst, const H* src, size_t n, hipStream_t st) {
    auto* p = detail::checked<H>(what, detail::span(dst), n);
    if (n) PMX_HIP_AT(what, hipMemcpyAsync(p, src, sizeof(H) * n, hipMemcpyHostToDevice, st));
}
template <class H, class Dst>
inline void h2d(const char* what, Dst&& dst, const std::vector<H>& src, size_t n, hipStream_t st) {
    detail::fits(what, src, n);
    h2d(what, dst, src.data(), n, st);
}
template <class H, class Dst>
inline void h2d(const char* what, Dst&& dst, const std::vector<H>& src, hipStream_t st) { h2d(what, dst, src.data(), src.size(), st); }
template <class H, size_t N, class Dst>
inline void h2d(const char* what, Dst&& dst, const H (&src)[N], hipStream_t st) { h2d(what, dst, &src[0], N, st); }
// a whole host vector into a buffer that grows to hold it
template <class T>
inline void upload(DevBuf<T>& dst, const std::vector<T>& src, hipStream_t st) {
    dst.ensure(src.size());
    h2d("upload", dst, src, st);
}

template <class H, class Src>
inline void d2h(const char* what, H* dst, Src&& src, size_t n, hipStream_t st) {
    const auto* p = detail::checked<H>(what, detail::span(src), n);
    if (n) PMX_HIP_AT(what, hipMemcpyAsync(dst, p, sizeof(H) * n, hipMemcpyDeviceToHost, st));
}
template <class H, class Src>
inline void d2h(const char* what, std::vector<H>& dst, Src&& src, size_t n, hipStream_t st) {
    detail::fits(what, dst, n);
    d2h(what, dst.data(), src, n, st);
}
template <class H, class Src>
inline void d2h(const char* what, std::vector<H>& dst, Src&& src, hipStream_t st) { d2h(what, dst.data(), src, dst.size(), st); }
template <class H, size_t N, class Src>
inline void d2h(const char* what, H (&dst)[N], Src&& src, hipStream_t st) { d2h(what, &dst[0], src, N, st); }
template <class... A>
inline void d2h_sync(const char* what, A&&... a) {
    d2h(what, a...);
    PMX_HIP(hipStreamSynchronize(detail::stream_of(a...)));
}

template <class Dst, class Src>
inline void d2d(const char* what_dst, const char* what_src, Dst&& dst, Src&& src, size_t n, hipStream_t st) {
    auto to = detail::span(dst);
    auto from = detail::span(src);
    using To = std::remove_pointer_t<decltype(to.p)>;   // the element type is the destination's, or the source's where the destination is void*
    using E = std::conditional_t<std::is_void_v<To>, std::remove_const_t<std::remove_pointer_t<decltype(from.p)>>, To>;
    auto* p = detail::checked<E>(what_dst, to, n);
    const auto* q = detail::checked<E>(what_src, from, n);
    if (n) PMX_HIP_AT(what_dst, hipMemcpyAsync(p, q, sizeof(E) * n, hipMemcpyDeviceToDevice, st));
}
template <class Dst>
inline void fill(const char* what, Dst&& dst, int byte, size_t n, hipStream_t st) {
    auto to = detail::span(dst);
    using E = std::remove_pointer_t<decltype(to.p)>;
    auto* p = detail::checked<E>(what, to, n);
    if (n) PMX_HIP_AT(what, hipMemsetAsync(p, byte, sizeof(E) * n, st));
}
template <class Dst>
inline void zero(const char* what, Dst&& dst, size_t n, hipStream_t st) { fill(what, dst, 0, n, st); }

// The blocking copies on the null stream, for callers that have no stream of their own to order against.
template <class H, class Dst>
inline void h2d_blocking(const char* what, Dst&& dst, const H* src, size_t n) {
    auto* p = detail::checked<H>(what, detail::span(dst), n);
    if (n) PMX_HIP_AT(what, hipMemcpy(p, src, sizeof(H) * n, hipMemcpyHostToDevice));
}
template <class H, class Src>
inline void d2h_blocking(const char* what, H* dst, Src&& src, size_t n) {
    const auto* p = detail::checked<H>(what, detail::span(src), n);
    if (n) PMX_HIP_AT(what, hipMemcpy(dst, p, sizeof(H) * n, hipMemcpyDeviceToHost));
}
#define PMX_H2D(dst, ...) pmx::h2d(#dst, dst, __VA_ARGS__)
#define PMX_D2H(dst, src, ...) pmx::d2h(#src, dst, src, __VA_ARGS__)
#define PMX_D2H_SYNC(dst, src, ...) pmx::d2h_sync(#src, dst, src, __VA_ARGS__)
#define PMX_D2D(dst, src, ...) pmx::d2d(#dst, #src, dst, src, __VA_ARGS__)
#define PMX_ZERO(dst, ...) pmx::zero(#dst, dst, __VA_ARGS__)
#define PMX_FILL(dst, ...) pmx::fill(#dst, dst, __VA_ARGS__)
#define PMX_H2D_BLOCKING(dst, ...) pmx::h2d_blocking(#dst, dst, __VA_ARGS__)
#define PMX_D2H_BLOCKING(dst, src, ...) pmx::d2h_blocking(#src, dst, src, __VA_ARGS__)

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
