// Dense multi-view-stereo geometry around a depth estimator: source views and depth ranges from the bundle-adjusted
// tracks, filtering and fusion of the depth maps into a coloured point cloud, and its voxel downsampling.
//
// Reference: gtsfm/densify/patchmatchnet_data.py:78-162 select_src_views_depth_ranges;
// gtsfm/densify/mvs_patchmatchnet.py:201-437 filter_depth and compute_filtered_reprojection_error with
// thirdparty/patchmatchnet/eval.py:11-125 reproject_with_depth and check_geometric_consistency;
// gtsfm/densify/mvs_base.py:75-92 with gtsfm/densify/mvs_utils.py:148-221 estimate_minimum_voxel_size and
// downsample_point_cloud (Open3D voxel_down_sample). The semantics are spelt out in include/gtsfm_hip.h.
//
// Mapping.
//   select views  one lane per measurement: its track by a binary search of the offsets, its depth into the camera's
//                 list (counted, scanned, then filled), and the Gaussian score of every later measurement of the track
//                 added to the pair matrix as a 2^-40 fixed-point integer atomic. One workgroup per camera takes the
//                 four order statistics of its depth list by an 8-bit radix select over order-preserving 64-bit keys
//                 (no sort, no length limit); one wave per row picks the sources.
//   fuse depth    one lane per reference pixel, 256 consecutive pixels of one view per workgroup: the reference-pixel
//                 loads and the three stores are coalesced, the four taps per source are gathers. The cameras of the
//                 view and of the source are uniform over the workgroup. Counts and the error sum (2^-24 fixed point)
//                 are integer atomics, one per wave and counter; the error minimum and maximum are integer atomics on
//                 the bit patterns of non-negative doubles.
//   gather        per-workgroup counts of the joint bits, a scan per view and over the views, then the same lanes
//                 write their points at view offset + workgroup offset + rank in the workgroup: row-major order.
//   voxels        mean, bounds and scatter by a fixed grid of workgroups and reduce.hpp's fixed-order sum; keys one lane
//                 per point; one lane per voxel adds its points in sorted order.
// Every result is a function of the input alone: integer atomics, fixed-order fp64 sums, no floating-point atomic.
#include <math.h>

#include <algorithm>

#include "common.hpp"

#pragma clang fp contract(off)

#include "reduce.hpp"  // block_sum

namespace {

typedef unsigned long long u64;
typedef long long i64;

#define MV_BLOCK 256
#define MV_SCAN_BLOCK 1024
#define MV_STAT_GRID 1024  // workgroups of the voxel statistics, at most

constexpr double kRadToDeg = 57.29577951308232;
constexpr double kScoreScale = 1099511627776.0;  // 2^40
constexpr double kErrScale = 16777216.0;         // 2^24
constexpr int kVoxelBits = 21;

enum { SV_NVALID, SV_NSRC, SV_EMPTY, SV_TERMS, SV_STATS };
enum { FU_GEO, FU_CONF, FU_JOINT, FU_ERR_COUNT, FU_COUNTS };
enum { MASK_GEO = 1, MASK_CONF = 2, MASK_JOINT = 4 };

// Exclusive scan of v over the workgroup (a multiple of 64 lanes, at most 1024); total is the sum, the same on every
// lane. sh holds 16 values.
__device__ __forceinline__ i64 block_scan(i64 v, i64* sh, i64& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    i64 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const i64 u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    if (lane == 63) sh[wave] = inc;
    __syncthreads();
    i64 base = 0, tot = 0;
    for (int w = 0; w < nw; ++w) {
        if (w < wave) base += sh[w];
        tot += sh[w];
    }
    __syncthreads();
    total = tot;
    return base + inc - v;
}

// Adds the number of lanes of the wave with `flag` set to *counter: one atomic per wave. Whole waves must call it.
__device__ __forceinline__ void wave_count(u64* counter, bool flag) {
    const u64 b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (u64)__popcll(b));
}

// ------------------------------------------------------------------------------------------------ select views
struct SvLayout {
    size_t cnt, off, cursor, depths, total;
};

inline SvLayout sv_layout(size_t n_meas, size_t n_img) {
    SvLayout L;
    WsCarver w;
    L.cnt = w.take(n_img * 4);
    L.off = w.take((n_img + 1) * 4);
    L.cursor = w.take(n_img * 4);
    L.depths = w.take(n_meas * 8);
    L.total = w.o;
    return L;
}

inline bool sv_sizes_ok(i64 n_tracks, i64 n_meas, int n_img) {
    const i64 lim = (1ll << 31) - 1;
    return n_tracks >= 0 && n_meas >= 0 && n_img >= 0 && n_tracks < lim && n_meas < lim && n_img <= 46340;
}

struct SvArgs {
    const int* offsets;
    const int* img;
    int n_tracks, n_meas, n_img;
    const double* point;
    const uint8_t* track_keep;
    const uint8_t* inlier;
    const double* wRc;
    const double* wtc;
    const uint8_t* cam_keep;
    int max_views, S;
    int *cnt, *off, *cursor;
    double* depths;
    int *img_to_pm, *pm_to_img;
    i64* scores;
    int* src;
    double* range;
    u64* stats;
};

// One workgroup: pm_i of every kept camera by a scan over the images in ascending order.
__global__ __launch_bounds__(MV_SCAN_BLOCK) void sv_map_kernel(SvArgs a) {
    __shared__ i64 sh[16];
    i64 base = 0;
    for (int i0 = 0; i0 < a.n_img; i0 += MV_SCAN_BLOCK) {
        const int i = i0 + threadIdx.x;
        const bool keep = i < a.n_img && (!a.cam_keep || a.cam_keep[i]);
        i64 total;
        const i64 pm = base + block_scan(keep ? 1 : 0, sh, total);
        if (i < a.n_img) a.img_to_pm[i] = keep ? (int)pm : -1;
        if (keep) a.pm_to_img[pm] = i;
        base += total;
    }
    for (int i = (int)base + threadIdx.x; i < a.n_img; i += MV_SCAN_BLOCK) a.pm_to_img[i] = -1;
    if (threadIdx.x == 0) {
        const i64 v = base < a.max_views ? base : a.max_views;
        a.stats[SV_NVALID] = (u64)base;
        a.stats[SV_NSRC] = (u64)(v > 0 ? v - 1 : 0);
        a.stats[SV_EMPTY] = 0;
        a.stats[SV_TERMS] = 0;
    }
}

__global__ __launch_bounds__(MV_BLOCK) void sv_init_kernel(SvArgs a) {
    const i64 i = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    const i64 n = a.n_img;
    if (i < n * n) a.scores[i] = 0;
    if (i < n * a.S) a.src[i] = -1;
    if (i < 2 * n) a.range[i] = 0.0;
    if (i < n) {
        a.cnt[i] = 0;
        a.cursor[i] = 0;
    }
}

// Largest t in [0, T) with offsets[t] <= m, given offsets[0] <= m.
__device__ __forceinline__ int sv_track_of(const int* __restrict__ offsets, int T, int m) {
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= m) lo = mid;
        else hi = mid;
    }
    return lo;
}

// pm_i of measurement m when it is an inlier in a valid camera, else -1. The track's own checks are the caller's.
__device__ __forceinline__ int sv_pm_of(const SvArgs& a, int m) {
    if (a.inlier && !a.inlier[m]) return -1;
    const int c = a.img[m];
    return (unsigned)c < (unsigned)a.n_img ? a.img_to_pm[c] : -1;
}

// The kept track that holds measurement m and its end, or false.
__device__ __forceinline__ bool sv_track(const SvArgs& a, int m, int& t, int& hi) {
    if (a.offsets[0] > m) return false;
    t = sv_track_of(a.offsets, a.n_tracks, m);
    const int lo = a.offsets[t];
    hi = a.offsets[t + 1];
    if (m >= hi || hi > a.n_meas || lo < 0) return false;
    return !a.track_keep || a.track_keep[t];
}

__global__ __launch_bounds__(MV_BLOCK) void sv_count_kernel(SvArgs a) {
    const i64 x = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    if (x >= a.n_meas) return;
    const int m = (int)x;
    int t, hi;
    if (!sv_track(a, m, t, hi)) return;
    const int pm = sv_pm_of(a, m);
    if (pm >= 0) atomicAdd(a.cnt + pm, 1);
}

// One workgroup: exclusive scan of the per-camera counts.
__global__ __launch_bounds__(MV_SCAN_BLOCK) void sv_scan_kernel(SvArgs a) {
    __shared__ i64 sh[16];
    i64 base = 0;
    for (int i0 = 0; i0 < a.n_img; i0 += MV_SCAN_BLOCK) {
        const int i = i0 + threadIdx.x;
        i64 total;
        const i64 e = base + block_scan(i < a.n_img ? a.cnt[i] : 0, sh, total);
        if (i < a.n_img) a.off[i] = (int)e;
        base += total;
    }
    if (threadIdx.x == 0) a.off[a.n_img] = (int)base;
}

__device__ __forceinline__ double sv_score(const double* X, const double* c1, const double* c2) {
    double r1[3], r2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r1[k] = X[k] - c1[k];
        r2[k] = X[k] - c2[k];
    }
    const double n1 = sqrt(r1[0] * r1[0] + r1[1] * r1[1] + r1[2] * r1[2]);
    const double n2 = sqrt(r2[0] * r2[0] + r2[1] * r2[1] + r2[2] * r2[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r1[k] /= n1;
        r2[k] /= n2;
    }
    double dot = r1[0] * r2[0] + r1[1] * r2[1] + r1[2] * r2[2];
    dot = dot < -1.0 ? -1.0 : (dot > 1.0 ? 1.0 : dot);
    const double theta = acos(dot) * kRadToDeg;
    const double sigma = theta <= 5.0 ? 1.0 : 10.0;
    const double d = theta - 5.0;
    return exp(-(d * d) / (2.0 * sigma * sigma));
}

__global__ __launch_bounds__(MV_BLOCK) void sv_fill_kernel(SvArgs a) {
    const i64 x = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    if (x >= a.n_meas) return;
    const int m = (int)x;
    int t, hi;
    if (!sv_track(a, m, t, hi)) return;
    const int pm = sv_pm_of(a, m);
    if (pm < 0) return;
    const int c = a.pm_to_img[pm];
    double X[3], c1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        X[k] = a.point[3 * (size_t)t + k];
        c1[k] = a.wtc[3 * (size_t)c + k];
    }
    const double* R = a.wRc + 9 * (size_t)c;
    const double z = R[2] * (X[0] - c1[0]) + R[5] * (X[1] - c1[1]) + R[8] * (X[2] - c1[2]);
    const int slot = a.off[pm] + atomicAdd(a.cursor + pm, 1);  // the list is sorted by value later: any order will do
    if (slot < a.off[pm + 1]) a.depths[slot] = z;
    const i64 n = a.n_img;
    u64 terms = 0;
    for (int k2 = m + 1; k2 < hi; ++k2) {
        const int pm2 = sv_pm_of(a, k2);
        if (pm2 < 0 || pm2 == pm) continue;
        const int cc = a.pm_to_img[pm2];
        double c2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c2[k] = a.wtc[3 * (size_t)cc + k];
        const double s = sv_score(X, c1, c2);
        if (!(s >= 0.0 && s <= 1.0)) continue;  // a point at a camera centre has no angle
        const u64 q = (u64)llround(s * kScoreScale);
        atomicAdd((u64*)a.scores + (pm * n + pm2), q);
        atomicAdd((u64*)a.scores + (pm2 * n + pm), q);
        ++terms;
    }
    if (terms) atomicAdd(a.stats + SV_TERMS, terms);
}

// Order-preserving 64-bit key of a double and back.
__device__ __forceinline__ u64 mv_key(double d) {
    const u64 b = (u64)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double mv_unkey(u64 k) {
    const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((i64)b);
}

// The rank-th smallest (0-based) of v[0..n) by the whole workgroup: eight passes of an 8-bit histogram over the keys
// that share the prefix found so far. The same value on every lane.
__device__ double mv_select(const double* __restrict__ v, int n, int rank, unsigned* hist, int* sh2) {
    u64 prefix = 0;
    int r = rank;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        const u64 himask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const u64 k = mv_key(v[i]);
            if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned c = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (c + hist[b] > (unsigned)r) break;
                c += hist[b];
            }
            sh2[0] = b;
            sh2[1] = r - (int)c;
        }
        __syncthreads();
        prefix |= (u64)sh2[0] << shift;
        r = sh2[1];
        __syncthreads();
    }
    return mv_unkey(prefix);
}

// np.percentile(v, 100 q), method "linear": the virtual index (n - 1) q and numpy's two-sided lerp.
__device__ double mv_percentile(const double* v, int n, double q, unsigned* hist, int* sh2) {
    const double pos = (double)(n - 1) * q;
    const double fl = floor(pos);
    const int lo = (int)fl;
    const int hi = lo + 1 < n ? lo + 1 : n - 1;
    const double t = pos - fl;
    const double x = mv_select(v, n, lo, hist, sh2);
    const double y = hi == lo ? x : mv_select(v, n, hi, hist, sh2);
    const double diff = y - x;
    return t >= 0.5 ? y - diff * (1.0 - t) : x + diff * t;
}

__global__ __launch_bounds__(MV_BLOCK) void sv_range_kernel(SvArgs a) {
    __shared__ unsigned hist[256];
    __shared__ int sh2[2];
    const int pm = blockIdx.x;
    if ((u64)pm >= a.stats[SV_NVALID]) return;
    const int lo = a.off[pm], n = a.off[pm + 1] - lo;
    double p1 = nan(""), p99 = nan("");
    if (n > 0) {
        p1 = mv_percentile(a.depths + lo, n, 0.01, hist, sh2);
        p99 = mv_percentile(a.depths + lo, n, 0.99, hist, sh2);
    }
    if (threadIdx.x == 0) {
        a.range[2 * pm] = p1;
        a.range[2 * pm + 1] = p99;
        if (n <= 0) atomicAdd(a.stats + SV_EMPTY, 1ull);
    }
}

// One wave per row: pick p is the best (score descending, pm_i ascending) view after pick p - 1 in that order.
__global__ __launch_bounds__(MV_BLOCK) void sv_src_kernel(SvArgs a) {
    const int lane = threadIdx.x & 63;
    const i64 r = (i64)blockIdx.x * (MV_BLOCK / 64) + (threadIdx.x >> 6);
    const i64 nv = (i64)a.stats[SV_NVALID];
    if (r >= nv) return;
    const int picks = (int)a.stats[SV_NSRC];
    const i64* row = a.scores + r * a.n_img;
    i64 ls = 0;
    int lc = -1;
    for (int p = 0; p < picks; ++p) {
        i64 bs = -1;
        int bc = 0x7fffffff;
        for (int c = lane; c < nv; c += 64) {
            if (c == r) continue;
            const i64 s = row[c];
            if (p > 0 && !(s < ls || (s == ls && c > lc))) continue;
            if (s > bs || (s == bs && c < bc)) {
                bs = s;
                bc = c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const i64 s2 = __shfl_xor(bs, o);
            const int c2 = __shfl_xor(bc, o);
            if (s2 > bs || (s2 == bs && c2 < bc)) {
                bs = s2;
                bc = c2;
            }
        }
        if (lane == 0) a.src[r * a.S + p] = bc;
        ls = bs;
        lc = bc;
    }
}

// ------------------------------------------------------------------------------------------------ fuse depth
struct FuArgs {
    const float* depth;
    const float* conf;
    int n_views, H, W;
    const double* wRc;
    const double* wtc;
    const double* intr;
    const int* src;
    int S;
    double pix_thr;
    float dep_thr, min_conf;
    int min_views;
    u64* raw;  // [n_views][3]: error sum in 2^-24, bits of the minimum, bits of the maximum
    float* fused;
    uint8_t* mask;
    u64* counts;  // [n_views][FU_COUNTS]
    double* err;  // [n_views][3]
};

struct MvCam {
    double R[9], t[3], f, u0, v0;
};

__device__ __forceinline__ void mv_load_cam(const double* wRc, const double* wtc, const double* intr, int i, MvCam& c) {
#pragma unroll
    for (int k = 0; k < 9; ++k) c.R[k] = wRc[9 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) c.t[k] = wtc[3 * (size_t)i + k];
    c.f = intr[3 * (size_t)i];
    c.u0 = intr[3 * (size_t)i + 1];
    c.v0 = intr[3 * (size_t)i + 2];
}

// Pixel (u, v) at depth d of camera a, in the frame of camera b.
__device__ __forceinline__ void mv_transfer(const MvCam& a, const MvCam& b, double u, double v, double d, double* out) {
    const double xc = (u - a.u0) / a.f * d, yc = (v - a.v0) / a.f * d;
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (a.R[3 * i] * xc + a.R[3 * i + 1] * yc + a.R[3 * i + 2] * d + a.t[i]) - b.t[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = b.R[j] * w[0] + b.R[3 + j] * w[1] + b.R[6 + j] * w[2];
}

// Bilinear sample at float coordinates with a constant-0 border, in float32.
__device__ __forceinline__ float mv_sample(const float* __restrict__ map, int H, int W, float x, float y) {
    if (!(x > -1.0f && x < (float)W && y > -1.0f && y < (float)H)) return 0.0f;
    const float fx = floorf(x), fy = floorf(y);
    const int x0 = (int)fx, y0 = (int)fy;
    const float ax = x - fx, ay = y - fy;
    const bool l = x0 >= 0, r = x0 + 1 < W, t = y0 >= 0, b = y0 + 1 < H;
    const float v00 = l && t ? map[(size_t)y0 * W + x0] : 0.0f;
    const float v10 = r && t ? map[(size_t)y0 * W + x0 + 1] : 0.0f;
    const float v01 = l && b ? map[(size_t)(y0 + 1) * W + x0] : 0.0f;
    const float v11 = r && b ? map[(size_t)(y0 + 1) * W + x0 + 1] : 0.0f;
    const float bx = 1.0f - ax, by = 1.0f - ay;
    return ((v00 * bx) * by + (v10 * ax) * by) + ((v01 * bx) * ay + (v11 * ax) * ay);
}

__global__ __launch_bounds__(MV_BLOCK) void fu_init_kernel(FuArgs a) {
    const int i = blockIdx.x * MV_BLOCK + threadIdx.x;
    if (i >= a.n_views) return;
    for (int k = 0; k < FU_COUNTS; ++k) a.counts[FU_COUNTS * (size_t)i + k] = 0;
    a.raw[3 * (size_t)i] = 0;
    a.raw[3 * (size_t)i + 1] = 0x7ff0000000000000ull;  // +inf
    a.raw[3 * (size_t)i + 2] = 0;
}

__global__ __launch_bounds__(MV_BLOCK) void fu_fuse_kernel(FuArgs a) {
    const int v = blockIdx.y;
    const i64 hw = (i64)a.H * a.W;
    const i64 p = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    const bool in = p < hw;
    MvCam ref;
    mv_load_cam(a.wRc, a.wtc, a.intr, v, ref);
    const size_t at = (size_t)v * hw + (in ? p : 0);
    const float d_ref = in ? a.depth[at] : 0.0f;
    const float cf = in ? a.conf[at] : 0.0f;
    const int px = (int)(p % a.W), py = (int)(p / a.W);
    const bool ok = in && isfinite(d_ref) && d_ref > 0.0f;
    int geo_sum = 0, n_err = 0;
    float dsum = 0.0f;
    double e_min = INFINITY, e_max = 0.0;
    u64 e_fixed = 0;
    for (int k = 0; k < a.S; ++k) {
        const int s = a.src[(size_t)v * a.S + k];
        if ((unsigned)s >= (unsigned)a.n_views) continue;  // uniform over the workgroup
        MvCam sc;
        mv_load_cam(a.wRc, a.wtc, a.intr, s, sc);
        if (!ok) continue;
        double xs[3];
        mv_transfer(ref, sc, (double)px, (double)py, (double)d_ref, xs);
        const double us = sc.f * xs[0] / xs[2] + sc.u0, vs = sc.f * xs[1] / xs[2] + sc.v0;
        const float sampled = mv_sample(a.depth + (size_t)s * hw, a.H, a.W, (float)us, (float)vs);
        double xr[3];
        mv_transfer(sc, ref, us, vs, (double)sampled, xr);
        const float d_rep = (float)xr[2];
        const float ur = (float)(ref.f * xr[0] / xr[2] + ref.u0), vr = (float)(ref.f * xr[1] / xr[2] + ref.v0);
        const double dx = (double)ur - (double)px, dy = (double)vr - (double)py;
        const double dist = sqrt(dx * dx + dy * dy);
        const float rel = fabsf(d_rep - d_ref) / d_ref;
        const bool near = dist < a.pix_thr;
        if (near && rel < a.dep_thr) {
            ++geo_sum;
            dsum += d_rep;
        }
        if (near) {
            ++n_err;
            e_fixed += (u64)llround(dist * kErrScale);
            e_min = dist < e_min ? dist : e_min;
            e_max = dist > e_max ? dist : e_max;
        }
    }
    // ok: with min_views <= 0 a pixel without a usable depth would pass with (0 + d_ref) / 1 as its fused depth, and a
    // NaN point would reach the cloud. With min_views >= 1 its geo_sum of 0 fails either way.
    const bool geo = ok && geo_sum >= a.min_views;
    const bool cok = in && cf > a.min_conf;
    const bool joint = geo && cok;
    if (in) {
        const float avg = (float)((double)(dsum + d_ref) / (double)(geo_sum + 1));
        a.fused[at] = joint ? avg : 0.0f;
        a.mask[at] = (uint8_t)((geo ? MASK_GEO : 0) | (cok ? MASK_CONF : 0) | (joint ? MASK_JOINT : 0));
    }
    u64* cnt = a.counts + FU_COUNTS * (size_t)v;
    wave_count(cnt + FU_GEO, geo);
    wave_count(cnt + FU_CONF, cok);
    wave_count(cnt + FU_JOINT, joint);
    // the error statistics of the joint pixels: one atomic per wave and quantity
    u64 ne = joint ? (u64)n_err : 0, ef = joint ? e_fixed : 0;
    double mn = joint && n_err ? e_min : INFINITY, mx = joint && n_err ? e_max : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ne += __shfl_xor(ne, o);
        ef += __shfl_xor(ef, o);
        const double mn2 = __shfl_xor(mn, o), mx2 = __shfl_xor(mx, o);
        mn = mn2 < mn ? mn2 : mn;
        mx = mx2 > mx ? mx2 : mx;
    }
    if ((threadIdx.x & 63) == 0 && ne) {
        atomicAdd(cnt + FU_ERR_COUNT, ne);
        atomicAdd(a.raw + 3 * (size_t)v, ef);
        atomicMin(a.raw + 3 * (size_t)v + 1, (u64)__double_as_longlong(mn));  // non-negative doubles order as integers
        atomicMax(a.raw + 3 * (size_t)v + 2, (u64)__double_as_longlong(mx));
    }
}

__global__ __launch_bounds__(MV_BLOCK) void fu_finish_kernel(FuArgs a) {
    const int i = blockIdx.x * MV_BLOCK + threadIdx.x;
    if (i >= a.n_views) return;
    const bool any = a.counts[FU_COUNTS * (size_t)i + FU_ERR_COUNT] != 0;
    a.err[3 * (size_t)i] = (double)a.raw[3 * (size_t)i] / kErrScale;
    a.err[3 * (size_t)i + 1] = any ? __longlong_as_double((i64)a.raw[3 * (size_t)i + 1]) : 0.0;
    a.err[3 * (size_t)i + 2] = any ? __longlong_as_double((i64)a.raw[3 * (size_t)i + 2]) : 0.0;
}

// ------------------------------------------------------------------------------------------------ gather points
struct GaLayout {
    size_t blk_cnt, blk_off, view_total, total;
};

inline GaLayout ga_layout(size_t n_views, size_t bpv) {
    GaLayout L;
    WsCarver w;
    L.blk_cnt = w.take(n_views * bpv * 4);
    L.blk_off = w.take(n_views * bpv * 8);
    L.view_total = w.take(n_views * 8);
    L.total = w.o;
    return L;
}

struct GaArgs {
    const float* fused;
    const uint8_t* mask;
    int n_views, H, W;
    const double* wRc;
    const double* wtc;
    const double* intr;
    const uint8_t* images;
    const int* view_image;
    int n_images, img_h, img_w;
    i64 capacity;
    int bpv;
    int* blk_cnt;
    i64* blk_off;
    i64* view_total;
    double* points;
    uint8_t* colors;
    i64* view_offset;
};

__global__ __launch_bounds__(MV_BLOCK) void ga_count_kernel(GaArgs a) {
    __shared__ int sh[MV_BLOCK / 64];
    const int v = blockIdx.y;
    const i64 hw = (i64)a.H * a.W;
    const i64 p = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    const bool on = p < hw && (a.mask[(size_t)v * hw + p] & MASK_JOINT);
    const u64 b = __ballot(on);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < MV_BLOCK / 64; ++w) n += sh[w];
        a.blk_cnt[(size_t)v * a.bpv + blockIdx.x] = n;
    }
}

// One workgroup per view: exclusive scan of its workgroup counts.
__global__ __launch_bounds__(MV_SCAN_BLOCK) void ga_scan_view_kernel(GaArgs a) {
    __shared__ i64 sh[16];
    const int v = blockIdx.x;
    i64 base = 0;
    for (int i0 = 0; i0 < a.bpv; i0 += MV_SCAN_BLOCK) {
        const int i = i0 + threadIdx.x;
        i64 total;
        const i64 e = base + block_scan(i < a.bpv ? a.blk_cnt[(size_t)v * a.bpv + i] : 0, sh, total);
        if (i < a.bpv) a.blk_off[(size_t)v * a.bpv + i] = e;
        base += total;
    }
    if (threadIdx.x == 0) a.view_total[v] = base;
}

// One workgroup: exclusive scan of the per-view counts.
__global__ __launch_bounds__(MV_SCAN_BLOCK) void ga_scan_kernel(GaArgs a) {
    __shared__ i64 sh[16];
    i64 base = 0;
    for (int i0 = 0; i0 < a.n_views; i0 += MV_SCAN_BLOCK) {
        const int i = i0 + threadIdx.x;
        i64 total;
        const i64 e = base + block_scan(i < a.n_views ? a.view_total[i] : 0, sh, total);
        if (i < a.n_views) a.view_offset[i] = e;
        base += total;
    }
    if (threadIdx.x == 0) a.view_offset[a.n_views] = base;
}

__global__ __launch_bounds__(MV_BLOCK) void ga_write_kernel(GaArgs a) {
    __shared__ int sh[MV_BLOCK / 64];
    const int v = blockIdx.y;
    const i64 hw = (i64)a.H * a.W;
    const i64 p = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    const bool on = p < hw && (a.mask[(size_t)v * hw + p] & MASK_JOINT);
    const u64 b = __ballot(on);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = __popcll(b);
    __syncthreads();
    if (!on) return;
    int rank = __popcll(b & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w) rank += sh[w];
    const i64 o = a.view_offset[v] + a.blk_off[(size_t)v * a.bpv + blockIdx.x] + rank;
    if (o >= a.capacity) return;
    MvCam c;
    mv_load_cam(a.wRc, a.wtc, a.intr, v, c);
    const int px = (int)(p % a.W), py = (int)(p / a.W);
    const double d = (double)a.fused[(size_t)v * hw + p];
    const double xc = ((double)px - c.u0) / c.f * d, yc = ((double)py - c.v0) / c.f * d;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        a.points[3 * (size_t)o + i] = c.R[3 * i] * xc + c.R[3 * i + 1] * yc + c.R[3 * i + 2] * d + c.t[i];
    const int im = a.view_image ? a.view_image[v] : v;
    const bool have = (unsigned)im < (unsigned)a.n_images;  // a view without an image is black
    const uint8_t* src = a.images + (((size_t)(have ? im : 0) * a.img_h + py) * a.img_w + px) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) a.colors[3 * (size_t)o + k] = have ? (uint8_t)(((float)src[k] / 255.0f) * 255.0f) : 0;
}

// ------------------------------------------------------------------------------------------------ voxels
enum { VS_MEAN = 0, VS_SCATTER = 3, VS_MIN = 12, VS_MAX = 15, VS_STATS = 18 };

__device__ __forceinline__ void block_minmax3(double* mn, double* mx, double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double a = __shfl_xor(mn[k], o), b = __shfl_xor(mx[k], o);
            mn[k] = a < mn[k] ? a : mn[k];
            mx[k] = b > mx[k] ? b : mx[k];
        }
    }
    if (lane == 0)
        for (int k = 0; k < 3; ++k) {
            sh[wave * 6 + k] = mn[k];
            sh[wave * 6 + 3 + k] = mx[k];
        }
    __syncthreads();
    for (int k = 0; k < 3; ++k) {
        double a = sh[k], b = sh[3 + k];
        for (int w = 1; w < nw; ++w) {
            a = sh[w * 6 + k] < a ? sh[w * 6 + k] : a;
            b = sh[w * 6 + 3 + k] > b ? sh[w * 6 + 3 + k] : b;
        }
        mn[k] = a;
        mx[k] = b;
    }
    __syncthreads();
}

// part[g][9]: sum, min, max of the points of workgroup g (a grid-stride share fixed by n and the grid alone).
__global__ __launch_bounds__(MV_BLOCK) void vs_mean_kernel(const double* __restrict__ pts, i64 n, double* part) {
    __shared__ double sh[16 * 6];
    double s[3] = {0.0, 0.0, 0.0}, mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (i64 i = (i64)blockIdx.x * MV_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * MV_BLOCK) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double x = pts[3 * i + k];
            s[k] += x;
            mn[k] = x < mn[k] ? x : mn[k];
            mx[k] = x > mx[k] ? x : mx[k];
        }
    }
    block_sum<3>(s, sh);
    block_minmax3(mn, mx, sh);
    if (threadIdx.x < 3) {
        part[9 * (size_t)blockIdx.x + threadIdx.x] = s[threadIdx.x];
        part[9 * (size_t)blockIdx.x + 3 + threadIdx.x] = mn[threadIdx.x];
        part[9 * (size_t)blockIdx.x + 6 + threadIdx.x] = mx[threadIdx.x];
    }
}

__global__ __launch_bounds__(MV_BLOCK) void vs_mean_finish_kernel(const double* part, int grid, i64 n, double* stats) {
    __shared__ double sh[16 * 6];
    double s[3] = {0.0, 0.0, 0.0}, mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int g = threadIdx.x; g < grid; g += MV_BLOCK) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[k] += part[9 * (size_t)g + k];
            const double a = part[9 * (size_t)g + 3 + k], b = part[9 * (size_t)g + 6 + k];
            mn[k] = a < mn[k] ? a : mn[k];
            mx[k] = b > mx[k] ? b : mx[k];
        }
    }
    block_sum<3>(s, sh);
    block_minmax3(mn, mx, sh);
    if (threadIdx.x < 3) {
        stats[VS_MEAN + threadIdx.x] = s[threadIdx.x] / (double)n;
        stats[VS_MIN + threadIdx.x] = mn[threadIdx.x];
        stats[VS_MAX + threadIdx.x] = mx[threadIdx.x];
    }
}

// part[g][6]: xx, xy, xz, yy, yz, zz of the centred points of workgroup g.
__global__ __launch_bounds__(MV_BLOCK) void vs_scatter_kernel(const double* __restrict__ pts, i64 n, const double* stats,
                                                              double* part) {
    __shared__ double sh[16 * 6];
    const double m0 = stats[VS_MEAN], m1 = stats[VS_MEAN + 1], m2 = stats[VS_MEAN + 2];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (i64 i = (i64)blockIdx.x * MV_BLOCK + threadIdx.x; i < n; i += (i64)gridDim.x * MV_BLOCK) {
        const double x = pts[3 * i] - m0, y = pts[3 * i + 1] - m1, z = pts[3 * i + 2] - m2;
        s[0] += x * x;
        s[1] += x * y;
        s[2] += x * z;
        s[3] += y * y;
        s[4] += y * z;
        s[5] += z * z;
    }
    block_sum<6>(s, sh);
    if (threadIdx.x < 6) part[6 * (size_t)blockIdx.x + threadIdx.x] = s[threadIdx.x];
}

__global__ __launch_bounds__(MV_BLOCK) void vs_scatter_finish_kernel(const double* part, int grid, i64 n, double* stats) {
    __shared__ double sh[16 * 6];
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = threadIdx.x; g < grid; g += MV_BLOCK) {
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += part[6 * (size_t)g + k];
    }
    block_sum<6>(s, sh);
    if (threadIdx.x == 0) {
        const double d = n >= 2 ? (double)(n - 1) : 1.0;
        const int at[9] = {0, 1, 2, 1, 3, 4, 2, 4, 5};
        for (int k = 0; k < 9; ++k) stats[VS_SCATTER + k] = n >= 2 ? s[at[k]] / d : 0.0;
    }
}

__global__ __launch_bounds__(MV_BLOCK) void vx_keys_kernel(const double* __restrict__ pts, i64 n, const double* stats,
                                                           double voxel, i64* keys) {
    const i64 i = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    if (i >= n) return;
    u64 key = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double origin = stats[VS_MIN + k] - voxel / 2.0;
        const double q = floor((pts[3 * i + k] - origin) / voxel);
        const double top = (double)((1 << kVoxelBits) - 1);
        const u64 idx = q >= 0.0 ? (u64)(q < top ? q : top) : 0ull;  // NaN falls to 0
        key = (key << kVoxelBits) | idx;
    }
    keys[i] = (i64)key;
}

struct VxLayout {
    size_t blk_cnt, blk_off, start, total;
};

inline VxLayout vx_layout(size_t n) {
    VxLayout L;
    WsCarver w;
    const size_t blocks = (n + MV_BLOCK - 1) / MV_BLOCK;
    L.blk_cnt = w.take(blocks * 4);
    L.blk_off = w.take(blocks * 8);
    L.start = w.take((n + 1) * 8);
    L.total = w.o;
    return L;
}

struct VxArgs {
    const double* pts;
    const uint8_t* colors;
    const i64* keys;  // sorted
    const i64* perm;
    i64 n;
    int blocks;
    int* blk_cnt;
    i64* blk_off;
    i64* start;
    double* out_pts;
    uint8_t* out_colors;
    i64* out_keys;
    int* out_count;
    i64* n_voxels;
};

__device__ __forceinline__ bool vx_head(const VxArgs& a, i64 i) { return i < a.n && (i == 0 || a.keys[i] != a.keys[i - 1]); }

__global__ __launch_bounds__(MV_BLOCK) void vx_count_kernel(VxArgs a) {
    __shared__ int sh[MV_BLOCK / 64];
    const i64 i = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    const u64 b = __ballot(vx_head(a, i));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
        for (int w = 0; w < MV_BLOCK / 64; ++w) n += sh[w];
        a.blk_cnt[blockIdx.x] = n;
    }
}

__global__ __launch_bounds__(MV_SCAN_BLOCK) void vx_scan_kernel(VxArgs a) {
    __shared__ i64 sh[16];
    i64 base = 0;
    for (int i0 = 0; i0 < a.blocks; i0 += MV_SCAN_BLOCK) {
        const int i = i0 + threadIdx.x;
        i64 total;
        const i64 e = base + block_scan(i < a.blocks ? a.blk_cnt[i] : 0, sh, total);
        if (i < a.blocks) a.blk_off[i] = e;
        base += total;
    }
    if (threadIdx.x == 0) {
        a.n_voxels[0] = base;
        a.start[base] = a.n;
    }
}

__global__ __launch_bounds__(MV_BLOCK) void vx_start_kernel(VxArgs a) {
    __shared__ int sh[MV_BLOCK / 64];
    const i64 i = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    const bool head = vx_head(a, i);
    const u64 b = __ballot(head);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) sh[wave] = __popcll(b);
    __syncthreads();
    if (!head) return;
    int rank = __popcll(b & ((1ull << lane) - 1));
    for (int w = 0; w < wave; ++w) rank += sh[w];
    a.start[a.blk_off[blockIdx.x] + rank] = i;
}

// One lane per voxel: its points in sorted order (ascending input index among equal keys, the sort being stable).
__global__ __launch_bounds__(MV_BLOCK) void vx_mean_kernel(VxArgs a) {
    const i64 j = (i64)blockIdx.x * MV_BLOCK + threadIdx.x;
    if (j >= a.n) return;
    if (j >= a.n_voxels[0]) {  // rows past the voxel count are zero
        for (int k = 0; k < 3; ++k) {
            a.out_pts[3 * j + k] = 0.0;
            a.out_colors[3 * j + k] = 0;
        }
        a.out_keys[j] = 0;
        a.out_count[j] = 0;
        return;
    }
    const i64 lo = a.start[j], hi = a.start[j + 1];
    double s[3] = {0.0, 0.0, 0.0};
    u64 c[3] = {0, 0, 0};
    for (i64 i = lo; i < hi; ++i) {
        const i64 q = a.perm[i];
        if ((u64)q >= (u64)a.n) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s[k] += a.pts[3 * q + k];
            c[k] += a.colors[3 * q + k];
        }
    }
    const u64 m = (u64)(hi - lo);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.out_pts[3 * j + k] = s[k] / (double)m;
        a.out_colors[3 * j + k] = (uint8_t)(c[k] / m);
    }
    a.out_keys[j] = a.keys[lo];
    a.out_count[j] = (int)m;
}

inline int vs_grid(i64 n) {
    const i64 b = (n + MV_BLOCK - 1) / MV_BLOCK;
    return (int)(b < MV_STAT_GRID ? b : MV_STAT_GRID);
}

inline bool fu_shape_ok(int n_views, int H, int W) {
    return n_views >= 0 && H >= 0 && W >= 0 && n_views <= 65535 && (i64)H * W < (1ll << 31) - MV_BLOCK;
}

}  // namespace

extern "C" {

size_t gtsfm_mvs_select_views_workspace_bytes(long long n_tracks, long long n_meas, int n_img) {
    if (n_tracks <= 0 || n_meas <= 0 || n_img <= 0 || !sv_sizes_ok(n_tracks, n_meas, n_img)) return 0;
    return sv_layout((size_t)n_meas, (size_t)n_img).total;
}

int gtsfm_mvs_select_views(const int* d_track_offsets, const int* d_track_img, long long n_tracks, long long n_meas,
                           const double* d_point, const uint8_t* d_track_keep, const uint8_t* d_meas_inlier,
                           const double* d_wRc, const double* d_wtc, const uint8_t* d_cam_keep, int n_img,
                           int max_num_views, void* d_workspace, size_t workspace_bytes, int* d_img_to_pm,
                           int* d_pm_to_img, long long* d_scores, int* d_src_views, double* d_depth_range,
                           long long* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!sv_sizes_ok(n_tracks, n_meas, n_img) || max_num_views < 1 || max_num_views > 65536) return GTSFM_ERR_ARG;
    const int S = max_num_views - 1;
    if (!d_stats) return GTSFM_ERR_ARG;
    if (n_img > 0 && (!d_img_to_pm || !d_pm_to_img || !d_scores || !d_depth_range || (S > 0 && !d_src_views)))
        return GTSFM_ERR_ARG;
    if (n_tracks == 0 || n_meas == 0 || n_img == 0) {  // no depth for any camera. Nothing below indexes an input.
        GTSFM_CHECK_HIP(hipMemsetAsync(d_stats, 0, SV_STATS * sizeof(long long), stream));
        if (n_img > 0) {
            const size_t n = (size_t)n_img;
            GTSFM_CHECK_HIP(hipMemsetAsync(d_img_to_pm, 0, n * sizeof(int), stream));
            GTSFM_CHECK_HIP(hipMemsetAsync(d_pm_to_img, 0, n * sizeof(int), stream));
            GTSFM_CHECK_HIP(hipMemsetAsync(d_scores, 0, n * n * sizeof(long long), stream));
            GTSFM_CHECK_HIP(hipMemsetAsync(d_depth_range, 0, n * 2 * sizeof(double), stream));
            if (S > 0) GTSFM_CHECK_HIP(hipMemsetAsync(d_src_views, 0, n * (size_t)S * sizeof(int), stream));
        }
        return GTSFM_OK;
    }
    if (!d_track_offsets || !d_track_img || !d_point || !d_wRc || !d_wtc || !d_workspace) return GTSFM_ERR_ARG;
    const SvLayout U = sv_layout((size_t)n_meas, (size_t)n_img);
    if (workspace_bytes < U.total) return GTSFM_ERR_CAPACITY;
    char* ws = (char*)d_workspace;
    SvArgs a;
    a.offsets = d_track_offsets;
    a.img = d_track_img;
    a.n_tracks = (int)n_tracks;
    a.n_meas = (int)n_meas;
    a.n_img = n_img;
    a.point = d_point;
    a.track_keep = d_track_keep;
    a.inlier = d_meas_inlier;
    a.wRc = d_wRc;
    a.wtc = d_wtc;
    a.cam_keep = d_cam_keep;
    a.max_views = max_num_views;
    a.S = S;
    a.cnt = (int*)(ws + U.cnt);
    a.off = (int*)(ws + U.off);
    a.cursor = (int*)(ws + U.cursor);
    a.depths = (double*)(ws + U.depths);
    a.img_to_pm = d_img_to_pm;
    a.pm_to_img = d_pm_to_img;
    a.scores = d_scores;
    a.src = d_src_views;
    a.range = d_depth_range;
    a.stats = (u64*)d_stats;

    const size_t cells = (size_t)n_img * (size_t)std::max(std::max(n_img, S), 2);
    hipLaunchKernelGGL(sv_map_kernel, dim3(1), dim3(MV_SCAN_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(sv_init_kernel, dim3(blocks_for(cells, MV_BLOCK)), dim3(MV_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sv_count_kernel, dim3(blocks_for((size_t)n_meas, MV_BLOCK)), dim3(MV_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(sv_scan_kernel, dim3(1), dim3(MV_SCAN_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(sv_fill_kernel, dim3(blocks_for((size_t)n_meas, MV_BLOCK)), dim3(MV_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(sv_range_kernel, dim3(n_img), dim3(MV_BLOCK), 0, stream, a);
    if (S > 0) hipLaunchKernelGGL(sv_src_kernel, dim3(blocks_for((size_t)n_img, MV_BLOCK / 64)), dim3(MV_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

size_t gtsfm_mvs_fuse_depth_workspace_bytes(int n_views, int height, int width) {
    if (n_views <= 0 || height <= 0 || width <= 0 || !fu_shape_ok(n_views, height, width)) return 0;
    return gtsfm_align_up((size_t)n_views * 3 * 8, 256);
}

int gtsfm_mvs_fuse_depth(const float* d_depth, const float* d_confidence, int n_views, int height, int width,
                         const double* d_wRc, const double* d_wtc, const double* d_intrinsics, const int* d_src_views,
                         int n_src, double pixel_thresh, double depth_thresh, double min_confidence,
                         int min_consistent_views, void* d_workspace, size_t workspace_bytes, float* d_fused,
                         uint8_t* d_mask, long long* d_counts, double* d_err, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!fu_shape_ok(n_views, height, width) || n_src < 0) return GTSFM_ERR_ARG;
    if (!(pixel_thresh >= 0.0 && pixel_thresh <= 1024.0) || depth_thresh != depth_thresh ||
        min_confidence != min_confidence)
        return GTSFM_ERR_ARG;
    if (n_views > 0 && (!d_counts || !d_err)) return GTSFM_ERR_ARG;
    if (n_views == 0) return GTSFM_OK;
    if (height == 0 || width == 0) {
        GTSFM_CHECK_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_views * FU_COUNTS * sizeof(long long), stream));
        GTSFM_CHECK_HIP(hipMemsetAsync(d_err, 0, (size_t)n_views * 3 * sizeof(double), stream));
        return GTSFM_OK;
    }
    if (!d_depth || !d_confidence || !d_wRc || !d_wtc || !d_intrinsics || (n_src > 0 && !d_src_views) || !d_fused ||
        !d_mask || !d_workspace)
        return GTSFM_ERR_ARG;
    if (workspace_bytes < gtsfm_mvs_fuse_depth_workspace_bytes(n_views, height, width)) return GTSFM_ERR_CAPACITY;
    FuArgs a;
    a.depth = d_depth;
    a.conf = d_confidence;
    a.n_views = n_views;
    a.H = height;
    a.W = width;
    a.wRc = d_wRc;
    a.wtc = d_wtc;
    a.intr = d_intrinsics;
    a.src = d_src_views;
    a.S = n_src;
    a.pix_thr = pixel_thresh;
    a.dep_thr = (float)depth_thresh;
    a.min_conf = (float)min_confidence;
    a.min_views = min_consistent_views;
    a.raw = (u64*)d_workspace;
    a.fused = d_fused;
    a.mask = d_mask;
    a.counts = (u64*)d_counts;
    a.err = d_err;
    const unsigned vb = blocks_for((size_t)n_views, MV_BLOCK);
    hipLaunchKernelGGL(fu_init_kernel, dim3(vb), dim3(MV_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(fu_fuse_kernel, dim3(blocks_for((size_t)height * width, MV_BLOCK), n_views), dim3(MV_BLOCK), 0,
                       stream, a);
    hipLaunchKernelGGL(fu_finish_kernel, dim3(vb), dim3(MV_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

size_t gtsfm_mvs_gather_points_workspace_bytes(int n_views, int height, int width) {
    if (n_views <= 0 || height <= 0 || width <= 0 || !fu_shape_ok(n_views, height, width)) return 0;
    return ga_layout((size_t)n_views, blocks_for((size_t)height * width, MV_BLOCK)).total;
}

int gtsfm_mvs_gather_points(const float* d_fused, const uint8_t* d_mask, int n_views, int height, int width,
                            const double* d_wRc, const double* d_wtc, const double* d_intrinsics,
                            const uint8_t* d_images, const int* d_view_image, int n_images, int image_height,
                            int image_width,
                            long long capacity, void* d_workspace, size_t workspace_bytes, double* d_points,
                            uint8_t* d_colors, long long* d_view_offset, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!fu_shape_ok(n_views, height, width) || capacity < 0 || !d_view_offset) return GTSFM_ERR_ARG;
    if (n_views == 0 || height == 0 || width == 0) {
        GTSFM_CHECK_HIP(hipMemsetAsync(d_view_offset, 0, ((size_t)n_views + 1) * sizeof(long long), stream));
        return GTSFM_OK;
    }
    if (image_height < height || image_width < width || n_images <= 0) return GTSFM_ERR_ARG;
    if (!d_fused || !d_mask || !d_wRc || !d_wtc || !d_intrinsics || !d_images || !d_workspace ||
        (capacity > 0 && (!d_points || !d_colors)))
        return GTSFM_ERR_ARG;
    const int bpv = (int)blocks_for((size_t)height * width, MV_BLOCK);
    const GaLayout L = ga_layout((size_t)n_views, (size_t)bpv);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    char* ws = (char*)d_workspace;
    GaArgs a;
    a.fused = d_fused;
    a.mask = d_mask;
    a.n_views = n_views;
    a.H = height;
    a.W = width;
    a.wRc = d_wRc;
    a.wtc = d_wtc;
    a.intr = d_intrinsics;
    a.images = d_images;
    a.view_image = d_view_image;
    a.n_images = n_images;
    a.img_h = image_height;
    a.img_w = image_width;
    a.capacity = capacity;
    a.bpv = bpv;
    a.blk_cnt = (int*)(ws + L.blk_cnt);
    a.blk_off = (i64*)(ws + L.blk_off);
    a.view_total = (i64*)(ws + L.view_total);
    a.points = d_points;
    a.colors = d_colors;
    a.view_offset = d_view_offset;
    hipLaunchKernelGGL(ga_count_kernel, dim3(bpv, n_views), dim3(MV_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(ga_scan_view_kernel, dim3(n_views), dim3(MV_SCAN_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(ga_scan_kernel, dim3(1), dim3(MV_SCAN_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    if (capacity > 0) hipLaunchKernelGGL(ga_write_kernel, dim3(bpv, n_views), dim3(MV_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

size_t gtsfm_mvs_voxel_stats_workspace_bytes(long long n_points) {
    if (n_points <= 0) return 0;
    return gtsfm_align_up((size_t)vs_grid(n_points) * 9 * 8, 256);
}

int gtsfm_mvs_voxel_stats(const double* d_points, long long n_points, void* d_workspace, size_t workspace_bytes,
                          double* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_points < 0 || !d_stats) return GTSFM_ERR_ARG;
    if (n_points == 0) {
        GTSFM_CHECK_HIP(hipMemsetAsync(d_stats, 0, VS_STATS * sizeof(double), stream));
        return GTSFM_OK;
    }
    if (!d_points || !d_workspace) return GTSFM_ERR_ARG;
    if (workspace_bytes < gtsfm_mvs_voxel_stats_workspace_bytes(n_points)) return GTSFM_ERR_CAPACITY;
    const int grid = vs_grid(n_points);
    double* part = (double*)d_workspace;
    hipLaunchKernelGGL(vs_mean_kernel, dim3(grid), dim3(MV_BLOCK), 0, stream, d_points, (i64)n_points, part);
    hipLaunchKernelGGL(vs_mean_finish_kernel, dim3(1), dim3(MV_BLOCK), 0, stream, part, grid, (i64)n_points, d_stats);
    hipLaunchKernelGGL(vs_scatter_kernel, dim3(grid), dim3(MV_BLOCK), 0, stream, d_points, (i64)n_points, d_stats, part);
    hipLaunchKernelGGL(vs_scatter_finish_kernel, dim3(1), dim3(MV_BLOCK), 0, stream, part, grid, (i64)n_points, d_stats);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

int gtsfm_mvs_voxel_keys(const double* d_points, long long n_points, const double* d_stats, double voxel_size,
                         long long* d_keys, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_points < 0 || !(voxel_size > 0.0) || voxel_size > 1.7e308) return GTSFM_ERR_ARG;
    if (n_points == 0) return GTSFM_OK;
    if (!d_points || !d_stats || !d_keys) return GTSFM_ERR_ARG;
    hipLaunchKernelGGL(vx_keys_kernel, dim3(blocks_for((size_t)n_points, MV_BLOCK)), dim3(MV_BLOCK), 0, stream, d_points,
                       (i64)n_points, d_stats, voxel_size, (i64*)d_keys);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

size_t gtsfm_mvs_voxel_downsample_workspace_bytes(long long n_points) {
    if (n_points <= 0 || n_points >= (1ll << 31) * MV_BLOCK) return 0;
    return vx_layout((size_t)n_points).total;
}

int gtsfm_mvs_voxel_downsample(const double* d_points, const uint8_t* d_colors, const long long* d_sorted_keys,
                               const long long* d_perm, long long n_points, void* d_workspace, size_t workspace_bytes,
                               double* d_out_points, uint8_t* d_out_colors, long long* d_out_keys, int* d_out_count,
                               long long* d_n_voxels, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_points < 0 || n_points >= (1ll << 31) * MV_BLOCK || !d_n_voxels) return GTSFM_ERR_ARG;
    if (n_points == 0) {
        GTSFM_CHECK_HIP(hipMemsetAsync(d_n_voxels, 0, sizeof(long long), stream));
        return GTSFM_OK;
    }
    if (!d_points || !d_colors || !d_sorted_keys || !d_perm || !d_workspace || !d_out_points || !d_out_colors ||
        !d_out_keys || !d_out_count)
        return GTSFM_ERR_ARG;
    const VxLayout L = vx_layout((size_t)n_points);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    char* ws = (char*)d_workspace;
    VxArgs a;
    a.pts = d_points;
    a.colors = d_colors;
    a.keys = (const i64*)d_sorted_keys;
    a.perm = (const i64*)d_perm;
    a.n = n_points;
    a.blocks = (int)blocks_for((size_t)n_points, MV_BLOCK);
    a.blk_cnt = (int*)(ws + L.blk_cnt);
    a.blk_off = (i64*)(ws + L.blk_off);
    a.start = (i64*)(ws + L.start);
    a.out_pts = d_out_points;
    a.out_colors = d_out_colors;
    a.out_keys = (i64*)d_out_keys;
    a.out_count = d_out_count;
    a.n_voxels = (i64*)d_n_voxels;
    hipLaunchKernelGGL(vx_count_kernel, dim3(a.blocks), dim3(MV_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(vx_scan_kernel, dim3(1), dim3(MV_SCAN_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(vx_start_kernel, dim3(a.blocks), dim3(MV_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(vx_mean_kernel, dim3(a.blocks), dim3(MV_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // extern "C"
