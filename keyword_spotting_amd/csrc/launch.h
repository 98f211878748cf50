// Host side of every kernel launch in libkws_amd.so: grid arithmetic, the dynamic-LDS grant, the launch itself, and the way
// from run-time shape parameters to template arguments.  Host-only; included by the kernel files and api_step.hip.
#pragma once
#include <atomic>
#include <type_traits>

#include "kws_internal.h"

namespace kws {

constexpr int kMaxDevices = 64;     // devices with a cache slot below; a device past them is asked every time

inline int groups_of(int B) { return (B + kStreamsPerGroup - 1) / kStreamsPerGroup; }      // 16-stream groups of a batch

// CUs of the current device (256 when it cannot be asked): the grid of a persistent kernel is min(groups, CUs)
inline int device_cu_count() {
    static std::atomic<int> cached[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 256;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n <= 0) {
        hipDeviceProp_t prop;
        n = hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
inline int persistent_grid(int B) { const int groups = groups_of(B), cus = device_cu_count(); return groups < cus ? groups : cus; }

// A launch that asks for more than half a CU's LDS (160 KB) gets one workgroup per CU: the workgroups of a layer-pipelined
// grid, or of two kernels running side by side, spread over the CUs instead of doubling up on some of them.
constexpr size_t kOneWorkgroupPerCuLds = 82 * 1024;
inline size_t one_workgroup_per_cu(size_t lds) { return lds < kOneWorkgroupPerCuLds ? kOneWorkgroupPerCuLds : lds; }

// Layer-pipelined grid of L layers x G groups.  L divides 8: block i runs on XCD i % 8 and serves layer (i % 8) % L, so the
// workgroups behind one L2 stream the same layer's weights; the grid is then whole rounds of 8 blocks (8 / L groups each),
// padding blocks included.  Otherwise layer-major, L x G blocks.
inline int pipelined_xcd_affine(int L) { return 8 % L == 0 ? 1 : 0; }
inline int pipelined_grid(int L, int G, int affine) {
    if (!affine) return G * L;
    const int per = 8 / L;
    return 8 * ((G + per - 1) / per);
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: one process may drive several GPUs
// (one handle each) from several host threads, so the "already granted" cache is per (kernel, device) and atomic.
// Setting the attribute twice is harmless; skipping it on a second device makes the launch fail there.
struct LdsGrant { std::atomic<size_t> bytes[kMaxDevices]; };
template <typename K>
inline hipError_t grant_dynamic_lds(K kernel, LdsGrant& cache, size_t lds) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool cached = dev >= 0 && dev < kMaxDevices;
    if (cached && cache.bytes[dev].load(std::memory_order_acquire) >= lds) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (cached) {
        size_t seen = cache.bytes[dev].load(std::memory_order_relaxed);
        while (seen < lds && !cache.bytes[dev].compare_exchange_weak(seen, lds, std::memory_order_release)) {}
    }
    return hipSuccess;
}

// The one launch: grant (lds > 0), launch, hipGetLastError.  The kernel is a template ARGUMENT, not a function parameter:
// instantiations of one kernel template share their pointer type, and a static keyed on that type would be one grant cache
// for the whole family -- a kernel first launched after a sibling with a larger request would never be granted its own.
template <auto Kernel, typename... A>
inline hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    if (lds > 0) {
        static LdsGrant granted;
        const hipError_t e = grant_dynamic_lds(Kernel, granted, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}

// Run-time values -> template arguments: f is a generic lambda and receives std::bool_constant / std::integral_constant
// objects, whose values are constant expressions inside it (`kernel<tpw(), first()>`).  A value outside Vs...:
// hipErrorInvalidValue, f not called.
template <typename F>
inline hipError_t with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }
template <int... Vs, typename F>
inline hipError_t with_int(int v, F&& f) {
    hipError_t e = hipErrorInvalidValue;
    (void)((v == Vs && ((e = f(std::integral_constant<int, Vs>{})), true)) || ...);
    return e;
}
// hidden -> TPW (16-unit tiles per wave: hidden / 64) among the instantiated TPWs..., and with (first, last) behind it
template <int... TPWs, typename F>
inline hipError_t with_tpw(int hidden, F&& f) { return with_int<TPWs...>(hidden % 64 == 0 ? hidden / 64 : -1, f); }
template <int... TPWs, typename F>
inline hipError_t with_layer_shape(int hidden, bool first, bool last, F&& f) {
    return with_tpw<TPWs...>(hidden, [&](auto tpw) {
        return with_bool(first, [&](auto fi) { return with_bool(last, [&](auto la) { return f(tpw, fi, la); }); });
    });
}

}  // namespace kws
