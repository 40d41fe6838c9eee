// Shared device/host helpers for the gtsfm_amd HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>
#include <utility>

#include "gtsfm_hip.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define GTSFM_CHECK_HIP(expr)                          \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return GTSFM_ERR_HIP;    \
    } while (0)

// Raises a kernel's dynamic-LDS limit to `bytes` on the CURRENT device, once per (kernel, device) and size;
// thread-safe (the attribute is per device, so a process-global "done" flag would skip the second GPU).
static inline hipError_t gtsfm_set_dynamic_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::map<std::pair<const void*, int>, int> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    int& have = done[{fn, dev}];
    if (have >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

__host__ __device__ static inline size_t gtsfm_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Workgroups of b lanes that cover n items.
static inline unsigned blocks_for(size_t n, unsigned b) { return (unsigned)((n + b - 1) / b); }

// Lays a device workspace out: take(bytes) is the offset of the next 256-byte aligned piece and `o` the bytes taken so
// far. An empty piece still takes 256 bytes, so no two pieces share an address.
struct WsCarver {
    size_t o = 0;
    size_t take(size_t bytes) {
        const size_t at = o;
        o += gtsfm_align_up(bytes ? bytes : 1, 256);
        return at;
    }
};

// Reads count elements back from the device on `stream` and waits for them.
template <class T>
static inline int read_back(T* host, const T* dev, size_t count, hipStream_t stream) {
    GTSFM_CHECK_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, stream));
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    return GTSFM_OK;
}

// Relaxed agent-scope load and store of an int that other lanes change with atomics while the kernel runs.
__device__ __forceinline__ int ld_int(const int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_int(int* p, int v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// x = h + m + l exactly, each plane the bf16 rounding of what the planes above it leave (both subtractions are
// exact): the operand split of the fp32-accurate bf16 MFMA products (conv3.hpp, sg_kernels.hpp).
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)x;
    const float r = x - (float)h;
    m = (__bf16)r;
    l = (__bf16)(r - (float)m);
}

// Sum / maximum of a float over the 64 lanes, every lane getting the result: the xor butterfly from offset 32 down
// to 1, an order the bit-exact tests of its callers depend on. (The double-precision wave sums of ba2.hip and
// transavg.hip have orders of their own, which their oracles restate.)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// Lane-wise min/max/median of three unsigned keys (v_min_u32 / v_med3_u32).
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t umed3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;  // one v_med3_u32 (the generic min/max form is not always matched by the backend)
    asm volatile("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

__device__ __forceinline__ uint32_t umin3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;  // one v_min3_u32
    asm volatile("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Insert two keys a, b into a running (b1 <= b2) top-2: 3 ops instead of 4. The second smallest of
// {b1, b2, a, b} is min(b2, med3(b1, a, b)) because b2 >= b1.
__device__ __forceinline__ void top2_insert2(uint32_t& b1, uint32_t& b2, uint32_t a, uint32_t b) {
    const uint32_t m = umed3(b1, a, b);
    b1 = umin3(b1, a, b);
    b2 = umin(b2, m);
}

// (a << s) | b in one v_lshl_or_b32 (keeps the backend from splitting shared shifts into shift + or pairs)
__device__ __forceinline__ uint32_t lshl_or(uint32_t a, uint32_t s, uint32_t b) {
    uint32_t r;
    asm volatile("v_lshl_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(s), "v"(b));
    return r;
}

// Insert key k into a running (b1 <= b2) top-2 of packed keys: second = med3(b1, b2, k), first = min(b1, k).
__device__ __forceinline__ void top2_insert(uint32_t& b1, uint32_t& b2, uint32_t k) {
    b2 = umed3(b1, b2, k);
    b1 = umin(b1, k);
}

// Merge two top-2 lists (a1 <= a2, c1 <= c2) into a.
__device__ __forceinline__ void top2_merge(uint32_t& a1, uint32_t& a2, uint32_t c1, uint32_t c2) {
    uint32_t n1 = umin(a1, c1);
    uint32_t n2 = umin(umax(a1, c1), umin(a2, c2));
    a1 = n1;
    a2 = n2;
}
