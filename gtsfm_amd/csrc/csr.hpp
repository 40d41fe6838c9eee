// Node-major lists by a stable counting sort: items 0..count are grouped by key (a node in [0, n)), ascending item
// index inside a node, without atomics, so two builds give the same bytes. gba.hip groups measurements by camera;
// transavg.hip and rotavg.hip list every edge at both of its ends.
//
// The items are cut into chunks, one lane per chunk:
//   csr_hist     a histogram per chunk, hist[chunk][node] (zeroed by csr_build);
//   csr_colscan  per node, an exclusive scan over the chunks: each chunk's first slot inside the node; off[v + 1] = the
//                node's count;
//   csr_scan     one lane: the counts become offsets, off[0..n];
//   csr_scatter  each chunk walks its items again and hands every entry its slot.
// What an item is comes from the caller's source Src, passed to the kernels by value:
//   static constexpr int kKeys                     keys per item: 1, or 2 for an edge listed at both of its ends
//   __device__ bool keys(long long m, int* k) const
//                                                  false: item m is left out; else its keys are in k[0..kKeys)
//   __device__ void put(long long m, const int* k, const size_t* slot) const
//                                                  writes item m's entries, one at each slot[i] (in node k[i])
// Sets no fp-contract pragma: include it after the includer's own (see se3.hpp).
#pragma once
#include "common.hpp"

namespace {

struct CsrChunks {
    int n, size;  // chunks, items per chunk
};

// One chunk per 64 items until max_chunks is reached, then larger chunks. The result of the sort does not depend on
// it; the size of hist does.
inline CsrChunks csr_chunks(long long count, int max_chunks) {
    CsrChunks c;
    c.n = (int)((count + 63) / 64 < max_chunks ? (count + 63) / 64 : max_chunks);
    c.size = (int)((count + c.n - 1) / c.n);
    return c;
}

inline size_t csr_hist_bytes(CsrChunks ch, size_t n) { return (size_t)ch.n * n * sizeof(int); }

template <class Src>
__global__ void csr_hist(Src src, long long count, int n, CsrChunks ch, int* hist) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ch.n) return;
    int* h = hist + (size_t)j * n;
    const long long b = (long long)j * ch.size;
    const long long e = b + ch.size < count ? b + ch.size : count;
    for (long long m = b; m < e; ++m) {
        int k[Src::kKeys];
        if (!src.keys(m, k)) continue;
#pragma unroll
        for (int i = 0; i < Src::kKeys; ++i) ++h[k[i]];
    }
}

__global__ void csr_colscan(int n, CsrChunks ch, int* hist, int* off) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    int run = 0;
    for (int j = 0; j < ch.n; ++j) {
        const int c = hist[(size_t)j * n + v];
        hist[(size_t)j * n + v] = run;
        run += c;
    }
    off[v + 1] = run;  // the node's count; csr_scan turns the counts into offsets
}

__global__ void csr_scan(int n, int* off) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int run = 0;
    off[0] = 0;
    for (int v = 0; v < n; ++v) {
        run += off[v + 1];
        off[v + 1] = run;
    }
}

template <class Src>
__global__ void csr_scatter(Src src, long long count, int n, CsrChunks ch, int* hist, const int* off) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ch.n) return;
    int* h = hist + (size_t)j * n;
    const long long b = (long long)j * ch.size;
    const long long e = b + ch.size < count ? b + ch.size : count;
    for (long long m = b; m < e; ++m) {
        int k[Src::kKeys];
        size_t slot[Src::kKeys];
        if (!src.keys(m, k)) continue;
#pragma unroll
        for (int i = 0; i < Src::kKeys; ++i) slot[i] = (size_t)off[k[i]] + h[k[i]]++;
        src.put(m, k, slot);
    }
}

// off [n + 1] and hist [ch.n][n] are the caller's; the entries go wherever src.put writes them.
template <class Src>
int csr_build(const Src& src, long long count, int n, CsrChunks ch, int* hist, int* off, hipStream_t stream) {
    GTSFM_CHECK_HIP(hipMemsetAsync(hist, 0, csr_hist_bytes(ch, n), stream));
    hipLaunchKernelGGL(csr_hist<Src>, dim3(blocks_for(ch.n, 64)), dim3(64), 0, stream, src, count, n, ch, hist);
    hipLaunchKernelGGL(csr_colscan, dim3(blocks_for(n, 256)), dim3(256), 0, stream, n, ch, hist, off);
    hipLaunchKernelGGL(csr_scan, dim3(1), dim3(64), 0, stream, n, off);
    hipLaunchKernelGGL(csr_scatter<Src>, dim3(blocks_for(ch.n, 64)), dim3(64), 0, stream, src, count, n, ch, hist, off);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // namespace
