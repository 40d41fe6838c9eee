// Prefix scans and the exact top-k selection of the two detectors (superpoint.hip, d2net.hip): the 256-lane exclusive
// scan, the per-image scan of a count array, and the radix select that keeps the k highest scores in list order.
// (compact.hip's 1024-lane `long long` scan is another algorithm and stays where it is.)
// Sets no fp-contract pragma: include it after the includer's own (see se3.hpp).
#pragma once
#include "common.hpp"

namespace {

constexpr int kScanThreads = 256;

// Exclusive scan of v over a workgroup of kScanThreads lanes, `total` its sum: wave-level inclusive scan, then across
// the 4 waves. sh holds 4 ints. Two barriers: every thread of the workgroup calls it, on uniform control flow.
__device__ __forceinline__ int block_excl_scan(int v, int* sh, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    int off = 0;
    for (int w = 0; w < wave; ++w) off += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    return off + x - v;
}

// Workgroup = image: off = exclusive scan of the image's per_image counts, total[image] = their sum.
__global__ __launch_bounds__(kScanThreads) void image_excl_scan_kernel(const int* __restrict__ cnt, int per_image,
                                                                       int* __restrict__ off,
                                                                       int* __restrict__ total) {
    __shared__ int sh[4];
    const int img = blockIdx.x;
    int carry = 0;
    for (int base = 0; base < per_image; base += kScanThreads) {
        const int e = base + threadIdx.x;
        const int v = e < per_image ? cnt[(size_t)img * per_image + e] : 0;
        int tot;
        const int ex = block_excl_scan(v, sh, tot);
        if (e < per_image) off[(size_t)img * per_image + e] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) total[img] = carry;
}

// ------------------------------------------------------------------ top-k by score, kept in list order
// The k highest of N positive scores, exactly: the key of a score is ~bits (positive floats order as their bits, so
// a larger score is a smaller key), and the selection is "every key < T, and the first need_eq keys == T in list
// order", T being the k-th smallest key. Equal scores at the cut therefore go to the earliest list positions, the rule
// tests/test_select_gpu.py, tests/test_d2net_planted.py and the SuperPoint 1080p tests pin down.
struct TopkCut {
    uint32_t T;
    int need_eq;
};

// T and need_eq by four 8-bit radix passes over score_at(0 .. N - 1). With N <= k everything is kept and the passes
// are skipped. histo holds 256 ints, pick 2. Barriers inside: every thread of the kScanThreads-lane workgroup calls
// it, with the same N and k.
template <class ScoreAt>
__device__ __forceinline__ TopkCut topk_cut(int N, int k, int* histo, int* pick, ScoreAt score_at) {
    const int tid = threadIdx.x;
    TopkCut cut{0xFFFFFFFFu, 0};
    if (N > k) {
        uint32_t prefix = 0;
        int need = k;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            const uint32_t pmask = pass == 0 ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < 256; i += kScanThreads) histo[i] = 0;
            __syncthreads();
            for (int i = tid; i < N; i += kScanThreads) {
                const uint32_t key = ~__float_as_uint(score_at(i));
                if ((key & pmask) == (prefix & pmask)) atomicAdd(&histo[(key >> shift) & 255], 1);
            }
            __syncthreads();
            if (tid == 0) {
                int acc = 0, d = 0;
                for (; d < 256; ++d) {
                    if (acc + histo[d] >= need) break;
                    acc += histo[d];
                }
                pick[0] = d;
                pick[1] = need - acc;
            }
            __syncthreads();
            prefix |= (uint32_t)pick[0] << shift;
            need = pick[1];
            __syncthreads();
        }
        cut.T = prefix;
        cut.need_eq = need;
    }
    return cut;
}

// The stable emit: emit(i, row) for every kept candidate i, row = the number of kept candidates before it. sh holds 4
// ints. Barriers inside (two scans per 256 candidates): every thread of the workgroup calls it, with the same N, k
// and cut.
template <class ScoreAt, class Emit>
__device__ __forceinline__ void topk_emit(int N, int k, TopkCut cut, int* sh, ScoreAt score_at, Emit emit) {
    const int tid = threadIdx.x;
    int written = 0, eq_seen = 0;
    for (int base = 0; base < N; base += kScanThreads) {
        const int i = base + tid;
        int sel = 0, eq = 0;
        if (i < N) {
            const uint32_t key = ~__float_as_uint(score_at(i));
            if (N <= k || key < cut.T) sel = 1;
            else if (key == cut.T) eq = 1;
        }
        int eq_total;
        const int eq_ex = block_excl_scan(eq, sh, eq_total);
        if (eq && eq_seen + eq_ex < cut.need_eq) sel = 1;
        int total;
        const int ex = block_excl_scan(sel, sh, total);
        if (sel) emit(i, written + ex);
        written += total;
        eq_seen += eq_total;
    }
}

}  // namespace
