// Cycle-consistent rotation view-graph filter: per-edge min / median of the 3-cycle rotation errors.
//
// Reference: gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:78-152 run (a Python loop over
// triplets), gtsfm/utils/graph.py:100-135 extract_cyclic_triplets_from_edges (adjacency-set intersection) and
// gtsfm/utils/geometry_comparisons.py:355-370 compute_cyclic_rotation_error:
//   for images i0 < i1 < i2 with all three edges present, M = R(i0,i2)^T R(i1,i2) R(i0,i1), error = angle(M) in degrees;
//   an edge's aggregate is np.amin / np.median over the triplets that contain it; keep iff aggregate < threshold.
//
// Workspace: an adjacency bit matrix bits[n_img][nw] (nw = ceil(n_img / 32) words) and a symmetric dense edge lookup
// tab[n_img][n_img] (edge index + 1, 0 = no edge), both zeroed and refilled on every call, and 256 partial sums for the
// triplet total.
// One workgroup per edge (a, b): it ANDs the bit rows of a and b, compacts the common neighbours c into LDS in
// ascending order, evaluates the cycle error of every sorted triple {a, b, c} into LDS and selects the min or the exact
// median there (an 8-bit radix select on the fp64 bit patterns: angles are >= +0, so the patterns order like the
// values). A triplet is evaluated once per edge it contains, by the same expression on the same sorted triple, so the
// three results are bit-identical and no atomics or per-edge lists in HBM are needed. LDS is sized for n_img - 2
// errors, the most one edge can have, so there is no per-pass capacity to exceed.
// Locality: lanes take consecutive c, so tab[a][c], tab[b][c] are coalesced row reads, and with edges sorted by
// (i1, i2) (the front-end's order) R(a, c) of consecutive c are adjacent 72-byte rows and consecutive workgroups share
// a's rows in L2.
#include <math.h>

#include <algorithm>

#include "common.hpp"

#define GTSFM_VG_MAX_IMAGES 8192

namespace {

typedef unsigned long long u64;

__host__ __device__ inline int vg_words(int n_img) { return (n_img + 31) / 32; }

#define VG_TOTAL_BLOCKS 256  // partial sums of the triplet total (<= 1024, vg_total_kernel's block)

struct VgLayout {
    size_t bits, tab, partial, total;
};

inline VgLayout vg_layout(int n_img) {
    VgLayout L;
    L.bits = 0;
    L.tab = gtsfm_align_up((size_t)n_img * vg_words(n_img) * sizeof(uint32_t), 256);
    L.partial = L.tab + gtsfm_align_up((size_t)n_img * n_img * sizeof(int), 256);
    L.total = L.partial + VG_TOTAL_BLOCKS * sizeof(u64);
    return L;
}

// dynamic LDS of the edge kernel: keys[cap] u64, hist[256] u32, red[8] u64, list[cap] u16 (cap = 32 * nw)
inline size_t vg_lds_bytes(int n_img) {
    const size_t cap = (size_t)vg_words(n_img) * 32;
    return cap * 8 + 256 * 4 + 8 * 8 + cap * 2;
}

// the edge takes part in the graph: flagged valid, indices in range and ordered
__device__ __forceinline__ bool vg_edge_ok(const int* __restrict__ edges, const uint8_t* __restrict__ valid, int n_img,
                                           int e, int& a, int& b) {
    a = edges[2 * e];
    b = edges[2 * e + 1];
    if (valid && !valid[e]) return false;
    return a >= 0 && a < b && b < n_img;
}

__global__ __launch_bounds__(256) void vg_fill_kernel(const int* __restrict__ edges, const uint8_t* __restrict__ valid,
                                                      int n_img, int n_edges, uint32_t* __restrict__ bits,
                                                      int* __restrict__ tab) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_edges) return;
    int a, b;
    if (!vg_edge_ok(edges, valid, n_img, e, a, b)) return;
    const int nw = vg_words(n_img);
    tab[(size_t)a * n_img + b] = e + 1;
    tab[(size_t)b * n_img + a] = e + 1;
    atomicOr(&bits[(size_t)a * nw + (b >> 5)], 1u << (b & 31));
    atomicOr(&bits[(size_t)b * nw + (a >> 5)], 1u << (a & 31));
}

template <int BLOCK>
__device__ __forceinline__ u64 vg_block_min(u64 v, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    if (BLOCK == 64) return v;
    __syncthreads();  // red is reused between calls
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) v = red[w] < v ? red[w] : v;
    return v;
}

template <int BLOCK>
__device__ __forceinline__ u64 vg_block_sum(u64 v, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (BLOCK == 64) return v;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = red[0];
#pragma unroll
    for (int w = 1; w < BLOCK / 64; ++w) v += red[w];
    return v;
}

// Cycle error in degrees of the sorted triple whose edges are rows e01, e12, e02 of R (row-major i2Ri1):
// M = R02^T (R12 R01), angle = atan2(|vee(M - M^T)| / 2, (tr M - 1) / 2). Every product is an explicit fma chain, so the
// value depends on the three matrices alone.
__device__ __forceinline__ double vg_cycle_error_deg(const double* __restrict__ R, int e01, int e12, int e02) {
    double A[9], B[9], C[9], T[9], M[9];
    const double* p01 = R + 9 * (size_t)e01;
    const double* p12 = R + 9 * (size_t)e12;
    const double* p02 = R + 9 * (size_t)e02;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        A[k] = p01[k];
        B[k] = p12[k];
        C[k] = p02[k];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            T[3 * i + j] = fma(B[3 * i + 2], A[6 + j], fma(B[3 * i + 1], A[3 + j], B[3 * i] * A[j]));
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = fma(C[6 + i], T[6 + j], fma(C[3 + i], T[3 + j], C[i] * T[j]));
    const double x = M[7] - M[5], y = M[2] - M[6], z = M[3] - M[1];
    const double s = 0.5 * sqrt(fma(x, x, fma(y, y, z * z)));
    const double c = 0.5 * (M[0] + M[4] + M[8] - 1.0);
    return atan2(s, c) * 57.295779513082320876798154814105;
}

// The key of rank k (0-based, ascending) among keys[0..n): 8 passes of an 8-bit radix select, most significant first.
// Every wave reads the finished histogram and derives the same digit, so nothing is broadcast through LDS.
template <int BLOCK>
__device__ __forceinline__ u64 vg_select(const u64* keys, int n, int k, uint32_t* hist) {
    const int t = threadIdx.x, lane = t & 63;
    u64 prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        __syncthreads();  // the previous pass's histogram has been read by every wave
        for (int i = t; i < 256; i += BLOCK) hist[i] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < n; i0 += BLOCK) {  // wave-uniform trip count: the ballots below see whole waves
            const int i = i0 + t;
            const u64 key = i < n ? keys[i] : 0;
            const bool in = i < n && (key & mask) == prefix;
            const int d = (int)((key >> shift) & 255);
            const u64 act = __ballot(in);
            if (act == 0) continue;
            // the leading bytes of angles in one range agree: one add per wave instead of 64 on one address
            const int d0 = __shfl(d, __ffsll((long long)act) - 1, 64);
            if (__ballot(in && d == d0) == act) {
                if (lane == __ffsll((long long)act) - 1) atomicAdd(&hist[d0], (uint32_t)__popcll(act));
            } else if (in) {
                atomicAdd(&hist[d], 1u);
            }
        }
        __syncthreads();
        const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
        const uint32_t s = h0 + h1 + h2 + h3;
        uint32_t incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        const u64 hit = __ballot((uint32_t)k < incl);  // never empty: the last lane's incl is the bucket's size > k
        const int src = __ffsll((long long)hit) - 1;
        uint32_t kk = (uint32_t)k - (incl - s);  // rank inside this lane's four bins
        int digit = 4 * lane;
        if (kk >= h0) {
            kk -= h0;
            ++digit;
            if (kk >= h1) {
                kk -= h1;
                ++digit;
                if (kk >= h2) {
                    kk -= h2;
                    ++digit;
                }
            }
        }
        digit = __shfl(digit, src, 64);
        k = (int)__shfl(kk, src, 64);
        prefix |= (u64)digit << shift;
        mask |= (u64)255 << shift;
    }
    return prefix;
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void vg_edge_kernel(const int* __restrict__ edges, const double* __restrict__ R,
                                                        const uint8_t* __restrict__ valid, int n_img, int criterion,
                                                        double thr_deg, const uint32_t* __restrict__ bits,
                                                        const int* __restrict__ tab, double* __restrict__ out_agg,
                                                        int* __restrict__ out_n, uint8_t* __restrict__ out_keep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char vg_lds[];
    const int nw = vg_words(n_img), cap = nw * 32;
    u64* keys = (u64*)vg_lds;
    uint32_t* hist = (uint32_t*)(keys + cap);
    u64* red = (u64*)(hist + 256);
    uint16_t* list = (uint16_t*)(red + 8);

    const int e = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    int a, b;
    if (!vg_edge_ok(edges, valid, n_img, e, a, b)) {  // block-uniform
        if (t == 0) {
            out_agg[e] = nan;
            out_n[e] = 0;
            out_keep[e] = 0;
        }
        return;
    }

    // common neighbours: one bitmap word per thread (nw <= BLOCK by the launcher's choice), compacted in order
    const uint32_t m = t < nw ? bits[(size_t)a * nw + t] & bits[(size_t)b * nw + t] : 0u;
    const int cnt = __popc(m);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    int base = 0, n = 0;
    if (BLOCK == 64) {
        n = __shfl(incl, 63, 64);
    } else {
        if (lane == 63) red[t >> 6] = (u64)incl;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < BLOCK / 64; ++w) {
            const int tot = (int)red[w];
            if (w < (t >> 6)) base += tot;
            n += tot;
        }
    }
    {
        int pos = base + incl - cnt;
        for (uint32_t mm = m; mm; mm &= mm - 1) list[pos++] = (uint16_t)(32 * t + __ffs((int)mm) - 1);
    }
    __syncthreads();

    if (n == 0) {  // in no triplet: the reference never enters the edge into per_edge_errors
        if (t == 0) {
            out_agg[e] = nan;
            out_n[e] = 0;
            out_keep[e] = 0;
        }
        return;
    }

    const int* ta = tab + (size_t)a * n_img;
    const int* tb = tab + (size_t)b * n_img;
    int any_nan = 0;
    u64 kmin = ~0ull;
    for (int i = t; i < n; i += BLOCK) {
        const int c = list[i];
        const int ea = ta[c] - 1, eb = tb[c] - 1;  // edges {a, c} and {b, c}
        int e01, e12, e02;
        if (c < a) {  // (c, a, b)
            e01 = ea, e02 = eb, e12 = e;
        } else if (c < b) {  // (a, c, b)
            e01 = ea, e12 = eb, e02 = e;
        } else {  // (a, b, c)
            e01 = e, e02 = ea, e12 = eb;
        }
        const double err = vg_cycle_error_deg(R, e01, e12, e02);
        any_nan |= err != err;
        const u64 key = (u64)__double_as_longlong(err);
        keys[i] = key;
        kmin = key < kmin ? key : kmin;
    }
    any_nan = __syncthreads_or(any_nan);  // also publishes keys

    double agg;
    if (any_nan) {  // np.amin and np.median both return NaN
        agg = nan;
    } else if (criterion == GTSFM_VG_MIN_EDGE_ERROR) {
        agg = __longlong_as_double((long long)vg_block_min<BLOCK>(kmin, red));
    } else {
        const int k0 = (n - 1) >> 1;
        const u64 v0 = vg_select<BLOCK>(keys, n, k0, hist);
        u64 v1 = v0;
        if ((n & 1) == 0) {  // even count: the next rank is v0 again when enough keys are <= v0, else the least key above it
            u64 le = 0, above = ~0ull;
            for (int i = t; i < n; i += BLOCK) {
                const u64 key = keys[i];
                if (key <= v0) ++le;
                else if (key < above) above = key;
            }
            le = vg_block_sum<BLOCK>(le, red);
            above = vg_block_min<BLOCK>(above, red);
            if (le < (u64)(k0 + 2)) v1 = above;
        }
        agg = 0.5 * (__longlong_as_double((long long)v0) + __longlong_as_double((long long)v1));
    }
    if (t == 0) {
        out_agg[e] = agg;
        out_n[e] = n;
        out_keep[e] = agg < thr_deg ? 1 : 0;
    }
}

// Every triplet is counted once by each of its three edges: grid-stride partial sums of n_triplets, one per workgroup
// into the workspace, then one workgroup adds them and divides by 3. Integer sums: any order gives the same total.
__device__ __forceinline__ u64 vg_sum_1024(u64 s, u64* part) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    u64 tot = 0;
    for (int w = 0; w < 16; ++w) tot += part[w];
    return tot;
}

__global__ __launch_bounds__(1024) void vg_partial_kernel(const int* __restrict__ n_trip, int n_edges,
                                                          u64* __restrict__ partial) {
    __shared__ u64 part[16];
    u64 s = 0;
    for (size_t i = (size_t)blockIdx.x * 1024 + threadIdx.x; i < (size_t)n_edges; i += (size_t)gridDim.x * 1024)
        s += (u64)n_trip[i];
    s = vg_sum_1024(s, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(1024) void vg_total_kernel(const u64* __restrict__ partial, int n_partial,
                                                        u64* __restrict__ total) {
    __shared__ u64 part[16];
    const u64 s = vg_sum_1024((int)threadIdx.x < n_partial ? partial[threadIdx.x] : 0, part);
    if (threadIdx.x == 0) total[0] = s / 3;
}

template <int BLOCK>
int vg_launch_edges(const int* d_edges, const double* d_R, const uint8_t* d_valid, int n_img, int n_edges, int criterion,
                    double thr, const uint32_t* bits, const int* tab, double* d_agg, int* d_n, uint8_t* d_keep,
                    hipStream_t stream) {
    const size_t lds = vg_lds_bytes(n_img);
    if (lds > 64 * 1024) GTSFM_CHECK_HIP(gtsfm_set_dynamic_lds((const void*)vg_edge_kernel<BLOCK>, (int)lds));
    hipLaunchKernelGGL(vg_edge_kernel<BLOCK>, dim3(n_edges), dim3(BLOCK), lds, stream, d_edges, d_R, d_valid, n_img,
                       criterion, thr, bits, tab, d_agg, d_n, d_keep);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // namespace

extern "C" {

size_t gtsfm_viewgraph_workspace_bytes(int n_img, int n_edges) {
    if (n_edges <= 0 || n_img <= 0 || n_img > GTSFM_VG_MAX_IMAGES) return 0;
    return vg_layout(n_img).total;
}

int gtsfm_viewgraph_cycle_filter(const int* d_edges, const double* d_R, const uint8_t* d_valid, int n_img, int n_edges,
                                 int criterion, double error_threshold_deg, void* d_workspace, size_t workspace_bytes,
                                 double* d_agg_error_deg, int* d_n_triplets, uint8_t* d_keep,
                                 unsigned long long* d_total_triplets, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_img < 0 || n_edges < 0 || n_img > GTSFM_VG_MAX_IMAGES) return GTSFM_ERR_ARG;
    if (criterion != GTSFM_VG_MIN_EDGE_ERROR && criterion != GTSFM_VG_MEDIAN_EDGE_ERROR) return GTSFM_ERR_ARG;
    if (n_edges == 0) return GTSFM_OK;
    if (n_img == 0 || !d_edges || !d_R || !d_workspace || !d_agg_error_deg || !d_n_triplets || !d_keep)
        return GTSFM_ERR_ARG;
    const VgLayout L = vg_layout(n_img);
    if (workspace_bytes < L.total) return GTSFM_ERR_ARG;

    uint32_t* bits = (uint32_t*)((char*)d_workspace + L.bits);
    int* tab = (int*)((char*)d_workspace + L.tab);
    GTSFM_CHECK_HIP(hipMemsetAsync(d_workspace, 0, L.total, stream));
    hipLaunchKernelGGL(vg_fill_kernel, dim3((n_edges + 255) / 256), dim3(256), 0, stream, d_edges, d_valid, n_img,
                       n_edges, bits, tab);
    GTSFM_CHECK_HIP(hipGetLastError());
    // one bitmap word per thread. Up to 512 images (at most 510 errors, 8 per lane) one wave per edge needs no
    // workgroup barrier; beyond that four waves, whose 256 words reach the ceiling
    int rc;
    if (vg_words(n_img) <= 16)
        rc = vg_launch_edges<64>(d_edges, d_R, d_valid, n_img, n_edges, criterion, error_threshold_deg, bits, tab,
                                 d_agg_error_deg, d_n_triplets, d_keep, stream);
    else
        rc = vg_launch_edges<256>(d_edges, d_R, d_valid, n_img, n_edges, criterion, error_threshold_deg, bits, tab,
                                  d_agg_error_deg, d_n_triplets, d_keep, stream);
    if (rc != GTSFM_OK) return rc;
    if (d_total_triplets) {
        u64* partial = (u64*)((char*)d_workspace + L.partial);
        const int nblk = (int)std::min<size_t>(VG_TOTAL_BLOCKS, ((size_t)n_edges + 1023) / 1024);
        hipLaunchKernelGGL(vg_partial_kernel, dim3(nblk), dim3(1024), 0, stream, d_n_triplets, n_edges, partial);
        GTSFM_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(vg_total_kernel, dim3(1), dim3(1024), 0, stream, partial, nblk, d_total_triplets);
        GTSFM_CHECK_HIP(hipGetLastError());
    }
    return GTSFM_OK;
}

}  // extern "C"
