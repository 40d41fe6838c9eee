// Fixed-order workgroup sums and the lock-free union-find of the back-end kernels (gba.hip, transavg.hip, tracks.hip,
// rotavg.hip). Sets no fp-contract pragma: include it after the includer's own (see se3.hpp).
#pragma once
#include "common.hpp"

namespace {

// Sum of v[0..NV) over the workgroup (a multiple of 64 lanes, at most 1024), the same on every lane: 64-lane butterfly,
// then the waves in order. sh holds 16 * NV doubles.
template <int NV>
__device__ __forceinline__ void block_sum(double* v, double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
    }
    if (lane == 0)
        for (int k = 0; k < NV; ++k) sh[wave * NV + k] = v[k];
    __syncthreads();
    for (int k = 0; k < NV; ++k) {
        double s = sh[k];
        for (int w = 1; w < nw; ++w) s += sh[w * NV + k];
        v[k] = s;
    }
    __syncthreads();
}

// Root of x with path halving. parent[y] <= y everywhere, so x strictly decreases until it is a root. parent is read
// and halved with relaxed loads and stores: a stale value is an older ancestor of the same component, still on a
// decreasing chain to the root.
__device__ __forceinline__ int uf_find(int* parent, int x) {
    for (;;) {
        const int p = ld_int(parent + x);
        if (p == x) return x;
        const int gp = ld_int(parent + p);
        if (gp != p) st_int(parent + x, gp);  // x is no root: only roots are CAS targets, so this races with none
        x = gp;
    }
}

// Hooks the larger root onto the smaller: a node becomes a non-root exactly once, so a component's root ends as its
// smallest index whatever the arrival order.
__device__ __forceinline__ void uf_unite(int* parent, int u, int v) {
    int a = uf_find(parent, u), b = uf_find(parent, v);
    while (a != b) {
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = uf_find(parent, old);  // a was hooked by someone else meanwhile: old < a
        b = uf_find(parent, b);
    }
}

}  // namespace
