// Triangulation of 2D tracks to 3D landmarks, with or without the two-view RANSAC over a track's measurement pairs.
//
// Reference: gtsfm/data_association/point3d_initializer.py:117-380 Point3dInitializer (execute_ransac_variant,
// triangulate, sample_ransac_hypotheses, extract_measurements), called once per track by
// gtsfm/data_association/data_assoc.py:211-273 DataAssociation.run_triangulation; gtsfm/utils/reprojection.py:48-83
// compute_point_reprojection_errors; gtsfm/utils/tracks.py:82-102 get_max_triangulation_angle with
// gtsfm/densify/mvs_utils.py:43-50; on GTSAM 4.2's triangulatePoint3(rank_tol = 1e-9, optimize = true): DLT null vector
// (rank >= 3), Levenberg-Marquardt on the unit-noise reprojection factors (lambda 1, factor 10, <= 100 iterations,
// absoluteErrorTol 1), cheirality in every camera used. The arithmetic of the two-view solve is ba2.hip's triangulate2
// generalised to n views; the semantics are spelt out in include/gtsfm_hip.h.
//
// Mapping. A (track, hypothesis) item is one independent fp64 solve, a track is a reduction over its items:
//   1. count     m_t = min(n_hyp, n (n - 1) / 2) per track (0 without RANSAC), exclusive int64 scan over tracks by one
//                workgroup: hyp_off[t]. hyp_off[n_tracks] is the "hypotheses evaluated" counter.
//   then, per chunk of tracks whose items fit the hypothesis buffer (chunk size fixed on the host from the workspace):
//   2. select    one wave per track with m_t < n_pairs: an 8-bit radix select over the 64-bit keys finds the m_t-th
//                smallest (key, j); keys are recomputed in every pass and never stored. The chosen j are written in
//                ascending order. Tracks that enumerate all their pairs skip this.
//   3. score     one lane per item: the item's track by a binary search of hyp_off bracketed by the wave's first and
//                last item (tracks.hip's row search), pair j -> (k1, k2), two-view solve, votes and mean inlier error
//                of all n measurements into the hypothesis buffer.
//   4. finish    one lane per track: minimum of (-votes, avg_err, j) over its items, that hypothesis solved again for
//                its inlier mask, then the n-view solve over the inliers and the exit-code ladder.
// One lane walks one track's measurements sequentially, in CSR order, and reads nothing another lane wrote in the same
// kernel: a track's result does not depend on which tracks share its wave, its chunk or its launch. The counters are
// integer atomics (one add per wave and counter); no floating-point atomic anywhere.
#include <math.h>

#include "common.hpp"
#include "twoview.hpp"  // sm_mix

#pragma clang fp contract(off)

#include "lm.hpp"   // the LM constants
#include "se3.hpp"  // chol3_solve

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr double kRankTol = 1e-9;
constexpr double kRadToDeg = 57.29577951308232;

#define TG_BLOCK 128
#define TG_SCAN_BLOCK 1024
#define TG_HYP_CAP_BYTES (64ull << 20)  // the hypothesis buffer the workspace query asks for, at most
#define TG_ITEM_BYTES 20                // j (int64), avg_err (double), votes (int32)

enum { kNoRansac = 0, kUniform = 1, kBiased = 2, kTopK = 3 };
enum { kSuccess = 0, kCheirality = 1, kInliersUnder = 2, kPosesUnder = 3, kExceeds = 4, kLowAngle = 5 };

struct TgArgs {
    const int* offsets;
    const int* img;
    const void* uv;
    int uv_f64;
    const int* track_id;
    i64 n_tracks_cap;
    const i64* d_n_tracks;
    i64 n_meas;
    const double* wRc;
    const double* wtc;
    const double* intr;
    const uint8_t* cam_valid;
    int n_img;
    int mode;
    double thresh, min_angle;
    int n_hyp;
    u64 seed;
    // workspace
    i64* hyp_off;    // [n_tracks_cap + 1]
    i64* item_j;     // [items_cap]
    double* item_avg;
    int* item_votes;
    // outputs
    int* exit_code;
    double* point;
    double* avg_err;
    uint8_t* inlier;
    i64* stats;
    int* track_n_hyp;
    i64* hyp_pair;
    i64 hyp_cap;
};

__device__ __forceinline__ i64 tg_n_tracks(const TgArgs& a) {
    i64 n = a.n_tracks_cap;
    if (a.d_n_tracks) {
        const i64 d = a.d_n_tracks[0];
        n = d < 0 ? 0 : (d < n ? d : n);
    }
    return n;
}

// [lo, hi) of track t in the measurement arrays, and whether they are usable
__device__ __forceinline__ bool tg_range(const TgArgs& a, i64 t, int& lo, int& n) {
    lo = a.offsets[t];
    const int hi = a.offsets[t + 1];
    n = hi - lo;
    return lo >= 0 && hi >= lo && (i64)hi <= a.n_meas;
}

__device__ __forceinline__ i64 tg_pairs(int n) { return (i64)n * (n - 1) / 2; }

__device__ __forceinline__ int tg_m(const TgArgs& a, int n) {
    if (a.mode == kNoRansac || n < 2) return 0;
    const i64 p = tg_pairs(n);
    return p < (i64)a.n_hyp ? (int)p : a.n_hyp;
}

// pair j of itertools.combinations(range(n), 2): row k1 starts at S(k1) = k1 n - k1 (k1 + 1) / 2
__device__ __forceinline__ i64 tg_row_start(i64 k1, i64 n) { return k1 * n - k1 * (k1 + 1) / 2; }

__device__ __forceinline__ void tg_pair_of(i64 j, int n, int& k1, int& k2) {
    const double b = 2.0 * n - 1.0;
    const double disc = b * b - 8.0 * (double)j;
    i64 r = (i64)((b - sqrt(disc > 0.0 ? disc : 0.0)) * 0.5);
    if (r < 0) r = 0;
    if (r > n - 2) r = n - 2;
    while (r + 1 <= n - 2 && tg_row_start(r + 1, n) <= j) ++r;
    while (r > 0 && tg_row_start(r, n) > j) --r;
    k1 = (int)r;
    k2 = (int)(j - tg_row_start(r, n) + r + 1);
}

struct Cam {
    double R[9];  // wRc row-major
    double t[3];  // wtc
    double K[3];  // f, u0, v0
};

__device__ __forceinline__ bool tg_cam_ok(const TgArgs& a, int i) {
    return (unsigned)i < (unsigned)a.n_img && (!a.cam_valid || a.cam_valid[i] != 0);
}

__device__ __forceinline__ void tg_load_cam(const TgArgs& a, int i, Cam& c) {
#pragma unroll
    for (int k = 0; k < 9; ++k) c.R[k] = a.wRc[9 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c.t[k] = a.wtc[3 * (size_t)i + k];
        c.K[k] = a.intr[3 * (size_t)i + k];
    }
}

__device__ __forceinline__ void tg_load_uv(const TgArgs& a, int pos, double* uv) {
    if (a.uv_f64) {
        const double* p = (const double*)a.uv + 2 * (size_t)pos;
        uv[0] = p[0];
        uv[1] = p[1];
    } else {
        const float* p = (const float*)a.uv + 2 * (size_t)pos;
        uv[0] = (double)p[0];
        uv[1] = (double)p[1];
    }
}

// point in the camera frame; false when z <= 0 (projectSafe)
__device__ __forceinline__ bool tg_project(const Cam& c, const double* p, double* pc, double* uv) {
    const double d[3] = {p[0] - c.t[0], p[1] - c.t[1], p[2] - c.t[2]};
#pragma unroll
    for (int j = 0; j < 3; ++j) pc[j] = c.R[j] * d[0] + c.R[3 + j] * d[1] + c.R[6 + j] * d[2];
    if (!(pc[2] > 0.0)) return false;
    uv[0] = c.K[1] + c.K[0] * (pc[0] / pc[2]);
    uv[1] = c.K[2] + c.K[0] * (pc[1] / pc[2]);
    return true;
}

// unit-noise reprojection factor: error e (2), d e / d p (2 x 3), returns 0.5 |e|^2. Behind the camera: GTSAM's
// cheirality branch (error 2 f per component, zero Jacobian).
__device__ __forceinline__ double tg_factor(const Cam& c, const double* p, const double* uv, double* e, double* Jp) {
    double pc[3], pr[2];
    if (!tg_project(c, p, pc, pr)) {
        e[0] = e[1] = 2.0 * c.K[0];
#pragma unroll
        for (int k = 0; k < 6; ++k) Jp[k] = 0.0;
    } else {
        e[0] = pr[0] - uv[0];
        e[1] = pr[1] - uv[1];
        const double iz = 1.0 / pc[2], xn = pc[0] * iz, yn = pc[1] * iz, f = c.K[0];
        const double D[6] = {f * iz, 0.0, -f * xn * iz, 0.0, f * iz, -f * yn * iz};
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Jp[3 * r + j] = D[3 * r] * c.R[3 * j] + D[3 * r + 1] * c.R[3 * j + 1] + D[3 * r + 2] * c.R[3 * j + 2];
    }
    return 0.5 * (e[0] * e[0] + e[1] * e[1]);
}

// The measurements a solve uses: the pair (ka, kb) when mask is null, else every k of the track with mask[k] set and a
// valid camera, in CSR order.
struct Sel {
    int lo, n;
    int ka, kb;
    const uint8_t* mask;  // at the track's first measurement
};

__device__ __forceinline__ int tg_sel_count(const Sel& s) { return s.mask ? s.n : 2; }

__device__ __forceinline__ bool tg_sel_at(const TgArgs& a, const Sel& s, int it, int& pos, int& img) {
    const int k = s.mask ? it : (it ? s.kb : s.ka);
    pos = s.lo + k;
    img = a.img[pos];
    if (!s.mask) return true;  // the caller checked both cameras
    return s.mask[k] != 0 && tg_cam_ok(a, img);
}

// one DLT row folded into the 4 x 4 upper-triangular factor T by four Givens rotations
__device__ __forceinline__ void tg_fold_row(double* T, double* row) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double x = T[5 * i], y = row[i];
        if (y == 0.0) continue;
        const double r = sqrt(x * x + y * y);
        const double c = x / r, s = y / r;
#pragma unroll
        for (int j = i; j < 4; ++j) {
            const double tj = T[4 * i + j], rj = row[j];
            T[4 * i + j] = c * tj + s * rj;
            row[j] = c * rj - s * tj;
        }
    }
}

// sum of the factors' 0.5 |e|^2 at p over the selection
__device__ __forceinline__ double tg_total_error(const TgArgs& a, const Sel& s, const double* p) {
    double err = 0.0;
    const int cnt = tg_sel_count(s);
    for (int it = 0; it < cnt; ++it) {
        int pos, img;
        if (!tg_sel_at(a, s, it, pos, img)) continue;
        Cam c;
        tg_load_cam(a, img, c);
        double uv[2], e[2], J[6];
        tg_load_uv(a, pos, uv);
        err += tg_factor(c, p, uv, e, J);
    }
    return err;
}

// triangulatePoint3 over the selection. false: rank < 3 or a point behind one of the cameras used.
__device__ __attribute__((noinline)) bool tg_triangulate(const TgArgs& a, const Sel& s, double* p_out) {
    const int cnt = tg_sel_count(s);
    double U[16], V[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) U[k] = 0.0;
    for (int it = 0; it < cnt; ++it) {
        int pos, img;
        if (!tg_sel_at(a, s, it, pos, img)) continue;
        Cam c;
        tg_load_cam(a, img, c);
        double uv[2];
        tg_load_uv(a, pos, uv);
        double P[12];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double row[3] = {c.R[r], c.R[3 + r], c.R[6 + r]};
            P[4 * r] = row[0];
            P[4 * r + 1] = row[1];
            P[4 * r + 2] = row[2];
            P[4 * r + 3] = -(row[0] * c.t[0] + row[1] * c.t[1] + row[2] * c.t[2]);
        }
        double r0[4], r1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double kp0 = c.K[0] * P[j] + c.K[1] * P[8 + j];
            const double kp1 = c.K[0] * P[4 + j] + c.K[2] * P[8 + j];
            r0[j] = uv[0] * P[8 + j] - kp0;
            r1[j] = uv[1] * P[8 + j] - kp1;
        }
        tg_fold_row(U, r0);
        tg_fold_row(U, r1);
    }
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool rotated = false;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double al = 0, be = 0, ga = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    al += U[4 * i + p] * U[4 * i + p];
                    be += U[4 * i + q] * U[4 * i + q];
                    ga += U[4 * i + p] * U[4 * i + q];
                }
                if (fabs(ga) <= 1e-15 * sqrt(al * be) || ga == 0.0) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double up = U[4 * i + p], uq = U[4 * i + q];
                    U[4 * i + p] = cs * up - sn * uq;
                    U[4 * i + q] = sn * up + cs * uq;
                    const double vp = V[4 * i + p], vq = V[4 * i + q];
                    V[4 * i + p] = cs * vp - sn * vq;
                    V[4 * i + q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    int rank = 0;
    double smin = INFINITY, vmin[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double sv = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) sv += U[4 * i + j] * U[4 * i + j];
        sv = sqrt(sv);
        if (sv > kRankTol) ++rank;
        if (sv < smin) {
            smin = sv;
#pragma unroll
            for (int i = 0; i < 4; ++i) vmin[i] = V[4 * i + j];
        }
    }
    if (rank < 3) return false;
    double p[3] = {vmin[0] / vmin[3], vmin[1] / vmin[3], vmin[2] / vmin[3]};
    double err = tg_total_error(a, s, p);
    double lambda = 1.0;
    int iters = 0;
    if (isfinite(err) && err > 0.0) {
        for (int outer = 0; outer < 200; ++outer) {
            const double cur = err;
            double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, bb = 0;
            for (int it = 0; it < cnt; ++it) {
                int pos, img;
                if (!tg_sel_at(a, s, it, pos, img)) continue;
                Cam c;
                tg_load_cam(a, img, c);
                double uv[2], e[2], J[6];
                tg_load_uv(a, pos, uv);
                tg_factor(c, p, uv, e, J);
#pragma unroll
                for (int r = 0; r < 2; ++r) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) {
                        g[i] += J[3 * r + i] * (-e[r]);
#pragma unroll
                        for (int j = 0; j < 3; ++j) H[3 * i + j] += J[3 * r + i] * J[3 * r + j];
                    }
                    bb += e[r] * e[r];
                }
            }
            for (int inner = 0; inner < kInnerMax; ++inner) {
                double Hd[9], d[3] = {g[0], g[1], g[2]};
#pragma unroll
                for (int k = 0; k < 9; ++k) Hd[k] = H[k];
#pragma unroll
                for (int i = 0; i < 3; ++i) Hd[4 * i] += lambda;
                bool success = false, stop = false;
                double newp[3], newErr = INFINITY;
                if (chol3_solve(Hd, d)) {
                    // linearised decrease of the undamped system at d: |e|^2 / 2 - |J d + e|^2 / 2 = d.g - d.H d / 2
                    double dHd = 0.0;
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        dHd += d[i] * (H[3 * i] * d[0] + H[3 * i + 1] * d[1] + H[3 * i + 2] * d[2]);
                    const double oldLin = 0.5 * bb;
                    const double linChange = (d[0] * g[0] + d[1] * g[1] + d[2] * g[2]) - 0.5 * dHd;
                    if (linChange >= 0) {
#pragma unroll
                        for (int i = 0; i < 3; ++i) newp[i] = p[i] + d[i];
                        newErr = tg_total_error(a, s, newp);
                        const double costChange = err - newErr;
                        if (linChange > kDblEps * oldLin) success = costChange / linChange > kMinFidelity;
                        else success = true;
                        if (fabs(costChange) < 1e-5 * err) stop = true;
                    }
                }
                if (success) {
#pragma unroll
                    for (int i = 0; i < 3; ++i) p[i] = newp[i];
                    err = newErr;
                    lambda /= 10.0;
                    ++iters;
                    break;
                }
                if (stop) break;
                lambda *= 10.0;
                if (lambda >= kLambdaUpper) break;
            }
            const double dec = cur - err;
            if (iters >= 100 || dec / cur <= 1e-5 || dec <= 1.0 || !isfinite(cur)) break;
        }
    }
    for (int it = 0; it < cnt; ++it) {
        int pos, img;
        if (!tg_sel_at(a, s, it, pos, img)) continue;
        Cam c;
        tg_load_cam(a, img, c);
        double pc[3], pr[2];
        if (!tg_project(c, p, pc, pr)) return false;
    }
    p_out[0] = p[0];
    p_out[1] = p[1];
    p_out[2] = p[2];
    return true;
}

// reprojection error of measurement `pos` against p: NaN for an invalid camera or z <= 0
__device__ __forceinline__ double tg_reproj(const TgArgs& a, int pos, const double* p) {
    const int img = a.img[pos];
    if (!tg_cam_ok(a, img)) return NAN;
    Cam c;
    tg_load_cam(a, img, c);
    double pc[3], pr[2], uv[2];
    if (!tg_project(c, p, pc, pr)) return NAN;
    tg_load_uv(a, pos, uv);
    const double dx = uv[0] - pr[0], dy = uv[1] - pr[1];
    return sqrt(dx * dx + dy * dy);
}

// the two-view hypothesis on measurements (k1, k2) of a track; false = skipped
__device__ __forceinline__ bool tg_hypothesis(const TgArgs& a, int lo, int n, int k1, int k2, double* p) {
    if (!tg_cam_ok(a, a.img[lo + k1]) || !tg_cam_ok(a, a.img[lo + k2])) return false;
    Sel s;
    s.lo = lo;
    s.n = n;
    s.ka = k1;
    s.kb = k2;
    s.mask = nullptr;
    return tg_triangulate(a, s, p);
}

// ---- selection keys -------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 tg_track_key(const TgArgs& a, i64 t) {
    const u64 id = a.track_id ? (u64)(uint32_t)a.track_id[t] : (u64)t;
    return sm_mix(a.seed ^ sm_mix(id));
}

__device__ __forceinline__ u64 tg_key(const TgArgs& a, u64 tkey, int lo, int n, i64 j) {
    if (a.mode == kUniform) return sm_mix(tkey + (u64)j);
    int k1, k2;
    tg_pair_of(j, n, k1, k2);
    const int i1 = a.img[lo + k1], i2 = a.img[lo + k2];
    if (!tg_cam_ok(a, i1) || !tg_cam_ok(a, i2)) return ~0ull;  // ranks with a zero baseline
    const double dx = a.wtc[3 * (size_t)i1] - a.wtc[3 * (size_t)i2];
    const double dy = a.wtc[3 * (size_t)i1 + 1] - a.wtc[3 * (size_t)i2 + 1];
    const double dz = a.wtc[3 * (size_t)i1 + 2] - a.wtc[3 * (size_t)i2 + 2];
    const double d2 = dx * dx + dy * dy + dz * dz;
    return ~(u64)__double_as_longlong(d2);  // d2 >= 0: its bits ascend with it; complemented for descending order
}

// ---- 1. count + scan ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TG_SCAN_BLOCK) void tg_scan_kernel(TgArgs a) {
    __shared__ i64 wsum[TG_SCAN_BLOCK / 64];
    const i64 n_tracks = tg_n_tracks(a);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    i64 carry = 0;
    for (i64 t0 = 0; t0 < n_tracks; t0 += TG_SCAN_BLOCK) {  // block-uniform trip count
        const i64 t = t0 + threadIdx.x;
        i64 m = 0;
        if (t < n_tracks) {
            int lo, n;
            if (tg_range(a, t, lo, n)) m = tg_m(a, n);
            if (a.track_n_hyp) a.track_n_hyp[t] = (int)m;
        }
        i64 incl = m;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const i64 up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        __syncthreads();  // wsum is reused between rounds
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        i64 before = 0, sum = 0;
#pragma unroll
        for (int i = 0; i < TG_SCAN_BLOCK / 64; ++i) {
            const i64 v = wsum[i];
            if (i < w) before += v;
            sum += v;
        }
        if (t < n_tracks) a.hyp_off[t] = carry + before + incl - m;
        carry += sum;
    }
    if (threadIdx.x == 0) {
        a.hyp_off[n_tracks] = carry;
        a.stats[7] = carry;
    }
}

// ---- 2. select ------------------------------------------------------------------------------------------------
// One wave per track of the chunk. Finds the m-th smallest (key, j) over the track's pairs by an 8-bit radix select on
// the key (ties on the key go to the smaller j) and writes the chosen j ascending into item_j.
__global__ __launch_bounds__(64) void tg_select_kernel(TgArgs a, i64 t_begin, i64 t_end) {
    __shared__ u64 hist[256];
    const i64 t = t_begin + blockIdx.x;
    const i64 n_tracks = tg_n_tracks(a);
    if (t >= t_end || t >= n_tracks) return;
    int lo, n;
    if (!tg_range(a, t, lo, n)) return;
    const int m = tg_m(a, n);
    const i64 n_pairs = tg_pairs(n);
    if (m == 0 || (i64)m == n_pairs) return;  // block-uniform
    const int lane = threadIdx.x;
    const u64 tkey = tg_track_key(a, t);
    u64 prefix = 0;   // the digits of the m-th smallest key found so far
    u64 below = 0;    // keys smaller than every key with that prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int b = lane; b < 256; b += 64) hist[b] = 0;
        __syncthreads();
        const u64 hi_mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
        for (i64 j = lane; j < n_pairs; j += 64) {
            const u64 k = tg_key(a, tkey, lo, n, j);
            if ((k & hi_mask) == prefix) atomicAdd(&hist[(unsigned)(k >> shift) & 255u], 1ull);
        }
        __syncthreads();
        // every lane walks the histogram: the digit at which the running count passes m - below
        u64 run = below;
        int digit = 255;
        for (int b = 0; b < 256; ++b) {
            const u64 c = hist[b];
            if (run + c >= (u64)m) {
                digit = b;
                break;
            }
            run += c;
        }
        below = run;
        prefix |= (u64)digit << shift;
        __syncthreads();
    }
    // prefix is the m-th smallest key; `below` keys are smaller; the first m - below of its equals (by j) are taken
    const i64 base = a.hyp_off[t] - a.hyp_off[t_begin];
    const i64 take_equal = (i64)m - (i64)below;
    i64 written = 0, equal_seen = 0;
    const u64 lt = (1ull << lane) - 1;
    for (i64 j0 = 0; j0 < n_pairs; j0 += 64) {  // wave-uniform trip count
        const i64 j = j0 + lane;
        bool less = false, equal = false;
        if (j < n_pairs) {
            const u64 k = tg_key(a, tkey, lo, n, j);
            less = k < prefix;
            equal = k == prefix;
        }
        const u64 eq_b = __ballot(equal);
        const bool take = less || (equal && equal_seen + (i64)__popcll(eq_b & lt) < take_equal);
        const u64 tk_b = __ballot(take);
        if (take) a.item_j[base + written + (i64)__popcll(tk_b & lt)] = j;
        written += __popcll(tk_b);
        equal_seen += __popcll(eq_b);
    }
}

// Largest t in [lo, hi) with hyp_off[t] <= g, given hyp_off[lo] <= g.
__device__ __forceinline__ i64 tg_track_of(const i64* __restrict__ off, i64 lo, i64 hi, i64 g) {
    while (hi - lo > 1) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- 3. score -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TG_BLOCK) void tg_score_kernel(TgArgs a, i64 t_begin, i64 t_end) {
    const i64 n_tracks = tg_n_tracks(a);
    if (t_begin >= n_tracks) return;
    if (t_end > n_tracks) t_end = n_tracks;
    const i64 g_begin = a.hyp_off[t_begin], g_end = a.hyp_off[t_end];
    const int lane = threadIdx.x & 63;
    const i64 wave_first = g_begin + (i64)blockIdx.x * TG_BLOCK + (threadIdx.x & ~63);
    if (wave_first >= g_end) return;
    const i64 g = wave_first + lane;
    if (g >= g_end) return;
    const i64 wave_last = wave_first + 63 < g_end - 1 ? wave_first + 63 : g_end - 1;
    const i64 t_lo = tg_track_of(a.hyp_off, t_begin, t_end, wave_first);
    const i64 t_hi = tg_track_of(a.hyp_off, t_lo, t_end, wave_last);
    const i64 t = tg_track_of(a.hyp_off, t_lo, t_hi + 1, g);
    const i64 slot = g - g_begin;  // < items_cap: the host sized the chunk
    int lo, n;
    tg_range(a, t, lo, n);  // m_t > 0, so the range was usable in the scan
    const i64 h = g - a.hyp_off[t];
    const bool all = (i64)tg_m(a, n) == tg_pairs(n);
    const i64 j = all ? h : a.item_j[slot];
    if (all) a.item_j[slot] = j;
    if (a.hyp_pair && g < a.hyp_cap) a.hyp_pair[g] = j;
    int k1, k2;
    tg_pair_of(j, n, k1, k2);
    double p[3];
    int votes = 0;
    double sum = 0.0;
    if (tg_hypothesis(a, lo, n, k1, k2, p)) {
        for (int k = 0; k < n; ++k) {
            const double e = tg_reproj(a, lo + k, p);
            if (e < a.thresh) {
                ++votes;
                sum += e;
            }
        }
    }
    a.item_votes[slot] = votes;
    a.item_avg[slot] = votes > 0 ? sum / (double)votes : NAN;
}

// ---- 4. finish ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TG_BLOCK) void tg_finish_kernel(TgArgs a, i64 t_begin, i64 t_end) {
    const i64 n_tracks = tg_n_tracks(a);
    if (t_end > n_tracks) t_end = n_tracks;
    const i64 t = t_begin + (i64)blockIdx.x * TG_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int code = -1;
    int n_inl_success = 0;
    if (t < t_end) {
        int lo, n;
        const bool usable = tg_range(a, t, lo, n);
        double pt[3] = {NAN, NAN, NAN}, avg = NAN;
        bool have_pt = false;
        if (!usable) {
            code = kInliersUnder;
        } else {
            uint8_t* mask = a.inlier + lo;
            int n_inl = 0;
            if (a.mode == kNoRansac) {
                for (int k = 0; k < n; ++k) mask[k] = 1;
                n_inl = n;
            } else {
                const i64 g0 = a.hyp_off[t], g1 = a.hyp_off[t + 1], base = a.hyp_off[t_begin];
                int best_votes = 0;
                double best_avg = INFINITY;
                i64 best_j = -1;
                for (i64 g = g0; g < g1; ++g) {
                    const int v = a.item_votes[g - base];
                    if (v <= 0) continue;
                    const double e = a.item_avg[g - base];
                    const i64 j = a.item_j[g - base];
                    if (v > best_votes || (v == best_votes && (e < best_avg || (e == best_avg && j < best_j)))) {
                        best_votes = v;
                        best_avg = e;
                        best_j = j;
                    }
                }
                double p[3];
                int k1 = 0, k2 = 0;
                bool ok = false;
                if (best_j >= 0) {
                    tg_pair_of(best_j, n, k1, k2);
                    ok = tg_hypothesis(a, lo, n, k1, k2, p);  // the same solve as the score pass: the same point
                }
                for (int k = 0; k < n; ++k) {
                    const bool in = ok && tg_reproj(a, lo + k, p) < a.thresh;
                    mask[k] = in ? 1 : 0;
                    n_inl += in ? 1 : 0;
                }
            }
            int n_posed = 0;
            for (int k = 0; k < n; ++k) n_posed += (mask[k] && tg_cam_ok(a, a.img[lo + k])) ? 1 : 0;
            if (n_inl < 2) {
                code = kInliersUnder;
            } else if (n_posed < 2) {
                code = kPosesUnder;
            } else {
                Sel s;
                s.lo = lo;
                s.n = n;
                s.ka = s.kb = 0;
                s.mask = mask;
                if (!tg_triangulate(a, s, pt)) {
                    code = kCheirality;
                } else {
                    have_pt = true;
                    bool all_in = true;
                    int n_fin = 0;
                    double sum = 0.0;
                    for (int k = 0; k < n; ++k) {
                        if (!mask[k]) continue;
                        const double e = tg_reproj(a, lo + k, pt);
                        if (!(e < a.thresh)) all_in = false;
                        if (e == e) {
                            sum += e;
                            ++n_fin;
                        }
                    }
                    avg = n_fin > 0 ? sum / (double)n_fin : NAN;
                    if (!all_in) {
                        code = kExceeds;
                    } else {
                        code = kSuccess;
                        if (a.min_angle > 0.0) {
                            // every inlier has a valid camera here: an invalid one gave a NaN error above
                            double min_dot = INFINITY;
                            for (int ka = 0; ka < n; ++ka) {
                                if (!mask[ka]) continue;
                                const int ia = a.img[lo + ka];
                                double ra[3];
                                double na = 0.0;
                                for (int c = 0; c < 3; ++c) {
                                    ra[c] = pt[c] - a.wtc[3 * (size_t)ia + c];
                                    na += ra[c] * ra[c];
                                }
                                na = sqrt(na);
                                for (int c = 0; c < 3; ++c) ra[c] = ra[c] / na;
                                for (int kb = ka + 1; kb < n; ++kb) {
                                    if (!mask[kb]) continue;
                                    const int ib = a.img[lo + kb];
                                    double rb[3];
                                    double nb = 0.0;
                                    for (int c = 0; c < 3; ++c) {
                                        rb[c] = pt[c] - a.wtc[3 * (size_t)ib + c];
                                        nb += rb[c] * rb[c];
                                    }
                                    nb = sqrt(nb);
                                    double dot = 0.0;
                                    for (int c = 0; c < 3; ++c) dot += ra[c] * (rb[c] / nb);
                                    dot = fmin(1.0, fmax(-1.0, dot));
                                    if (dot < min_dot) min_dot = dot;
                                }
                            }
                            const double angle = acos(min_dot) * kRadToDeg;
                            if (angle < a.min_angle) code = kLowAngle;
                        }
                        if (code == kSuccess) n_inl_success = n_inl;
                    }
                }
            }
        }
        a.exit_code[t] = code;
        a.avg_err[t] = avg;
        if (have_pt) {
            a.point[3 * t] = pt[0];
            a.point[3 * t + 1] = pt[1];
            a.point[3 * t + 2] = pt[2];
        }
    }
    // counters: one integer add per wave and counter
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int cnt = __popcll(__ballot(code == c));
        if (lane == 0 && cnt) atomicAdd((u64*)a.stats + c, (u64)cnt);
    }
    int s = n_inl_success;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0 && s) atomicAdd((u64*)a.stats + 6, (u64)s);
}

struct TgLayout {
    size_t hyp_off, item_j, item_avg, item_votes, total;
    i64 items_cap;
};

// fixed part: the scan; then a hypothesis buffer of items_cap items
inline size_t tg_fixed_bytes(i64 n_tracks) { return gtsfm_align_up((size_t)(n_tracks + 1) * 8, 256); }

inline TgLayout tg_layout(i64 n_tracks, size_t workspace_bytes) {
    TgLayout L;
    L.hyp_off = 0;
    const size_t fixed = tg_fixed_bytes(n_tracks);
    L.items_cap = 0;
    L.item_j = L.item_avg = L.item_votes = L.total = fixed;
    if (workspace_bytes <= fixed + 3 * 256) return L;
    const size_t rest = workspace_bytes - fixed - 3 * 256;
    i64 cap = (i64)(rest / TG_ITEM_BYTES);
    cap = cap / 64 * 64;  // keeps the three arrays aligned
    L.items_cap = cap;
    L.item_j = fixed;
    L.item_avg = gtsfm_align_up(L.item_j + (size_t)cap * 8, 256);
    L.item_votes = gtsfm_align_up(L.item_avg + (size_t)cap * 8, 256);
    L.total = gtsfm_align_up(L.item_votes + (size_t)cap * 4, 256);
    return L;
}

}  // namespace

extern "C" {

size_t gtsfm_triangulate_workspace_bytes(long long n_tracks, long long n_meas, int n_hyp) {
    if (n_tracks <= 0 || n_meas <= 0 || n_hyp < 0) return 0;
    if (n_tracks >= (1ll << 31) || n_meas >= (1ll << 31)) return 0;
    // a track has at most per_track = min(n_hyp, n_meas (n_meas - 1) / 2) items. The buffer holds all tracks' items
    // up to the cap, and one track's whatever the cap.
    const unsigned long long by_meas = (unsigned long long)n_meas * (unsigned long long)(n_meas - 1) / 2;
    const unsigned long long per_track = by_meas < (unsigned long long)n_hyp ? by_meas : (unsigned long long)n_hyp;
    unsigned long long bytes = (unsigned long long)n_tracks * per_track * TG_ITEM_BYTES;
    if (bytes > TG_HYP_CAP_BYTES) bytes = TG_HYP_CAP_BYTES;
    if (bytes < per_track * TG_ITEM_BYTES) bytes = per_track * TG_ITEM_BYTES;
    return tg_fixed_bytes(n_tracks) + gtsfm_align_up((size_t)bytes + 64 * TG_ITEM_BYTES, 256) + 3 * 256;
}

int gtsfm_triangulate_tracks(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                             const int* d_track_id, long long n_tracks, const long long* d_n_tracks, long long n_meas,
                             const double* d_wRc, const double* d_wtc, const double* d_intrinsics,
                             const uint8_t* d_cam_valid, int n_img, int mode, double reproj_error_threshold,
                             double min_triangulation_angle, int n_hyp, uint64_t seed, void* d_workspace,
                             size_t workspace_bytes, int* d_exit_code, double* d_point, double* d_avg_err,
                             uint8_t* d_inlier, long long* d_stats, int* d_track_n_hyp, long long* d_hyp_pair,
                             long long hyp_cap, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_tracks < 0 || n_meas < 0 || n_img < 0 || n_hyp < 0 || hyp_cap < 0) return GTSFM_ERR_ARG;
    if (n_tracks >= (1ll << 31) || n_meas >= (1ll << 31)) return GTSFM_ERR_ARG;
    if (mode != kNoRansac && mode != kUniform && mode != kTopK) return GTSFM_ERR_ARG;  // BIASED_BASELINE: not built
    if (!(reproj_error_threshold > 0.0) || min_triangulation_angle != min_triangulation_angle) return GTSFM_ERR_ARG;
    if (!d_stats) return GTSFM_ERR_ARG;
    GTSFM_CHECK_HIP(hipMemsetAsync(d_stats, 0, 8 * sizeof(long long), stream));
    if (n_tracks == 0) return GTSFM_OK;
    if (!d_track_offsets || !d_wRc || !d_wtc || !d_intrinsics || !d_workspace || !d_exit_code || !d_point ||
        !d_avg_err || n_img == 0)
        return GTSFM_ERR_ARG;
    if (n_meas > 0 && (!d_track_img || !d_track_uv || !d_inlier)) return GTSFM_ERR_ARG;
    if (mode != kNoRansac && n_hyp == 0) return GTSFM_ERR_ARG;
    if (d_hyp_pair == nullptr) hyp_cap = 0;

    // a track has at most min(n_hyp, n_meas (n_meas - 1) / 2) items (nothing here relies on a track naming an image
    // once, so n_img does not bound its length)
    i64 per_track = 0;
    if (mode != kNoRansac) {
        const i64 pairs_max = n_meas * (n_meas - 1) / 2;
        per_track = pairs_max < (i64)n_hyp ? pairs_max : (i64)n_hyp;
    }
    const TgLayout L = tg_layout(n_tracks, workspace_bytes);
    if (workspace_bytes < tg_fixed_bytes(n_tracks)) return GTSFM_ERR_CAPACITY;
    if (per_track > 0 && L.items_cap < per_track) return GTSFM_ERR_CAPACITY;
    if (L.total > workspace_bytes) return GTSFM_ERR_CAPACITY;

    char* ws = (char*)d_workspace;
    TgArgs a;
    a.offsets = d_track_offsets;
    a.img = d_track_img;
    a.uv = d_track_uv;
    a.uv_f64 = uv_is_f64;
    a.track_id = d_track_id;
    a.n_tracks_cap = n_tracks;
    a.d_n_tracks = d_n_tracks;
    a.n_meas = n_meas;
    a.wRc = d_wRc;
    a.wtc = d_wtc;
    a.intr = d_intrinsics;
    a.cam_valid = d_cam_valid;
    a.n_img = n_img;
    a.mode = mode;
    a.thresh = reproj_error_threshold;
    a.min_angle = min_triangulation_angle;
    a.n_hyp = n_hyp;
    a.seed = seed;
    a.hyp_off = (i64*)(ws + L.hyp_off);
    a.item_j = (i64*)(ws + L.item_j);
    a.item_avg = (double*)(ws + L.item_avg);
    a.item_votes = (int*)(ws + L.item_votes);
    a.exit_code = d_exit_code;
    a.point = d_point;
    a.avg_err = d_avg_err;
    a.inlier = d_inlier;
    a.stats = d_stats;
    a.track_n_hyp = d_track_n_hyp;
    a.hyp_pair = d_hyp_pair;
    a.hyp_cap = hyp_cap;

    hipLaunchKernelGGL(tg_scan_kernel, dim3(1), dim3(TG_SCAN_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    // chunks of tracks whose items fit the hypothesis buffer whatever their lengths
    i64 chunk = n_tracks;
    if (per_track > 0) {
        chunk = L.items_cap / per_track;
        if (chunk > n_tracks) chunk = n_tracks;
    }
    const i64 finish_cap = 1ll << 22;  // tracks per finish launch
    if (chunk > finish_cap) chunk = finish_cap;
    for (i64 t0 = 0; t0 < n_tracks; t0 += chunk) {
        const i64 t1 = t0 + chunk < n_tracks ? t0 + chunk : n_tracks;
        if (per_track > 0) {
            if ((i64)n_hyp < n_meas * (n_meas - 1) / 2) {  // some track may have to choose among its pairs
                hipLaunchKernelGGL(tg_select_kernel, dim3((unsigned)(t1 - t0)), dim3(64), 0, stream, a, t0, t1);
                GTSFM_CHECK_HIP(hipGetLastError());
            }
            const i64 items = (t1 - t0) * per_track;  // <= items_cap
            const unsigned blocks = (unsigned)((items + TG_BLOCK - 1) / TG_BLOCK);
            hipLaunchKernelGGL(tg_score_kernel, dim3(blocks), dim3(TG_BLOCK), 0, stream, a, t0, t1);
            GTSFM_CHECK_HIP(hipGetLastError());
        }
        const unsigned blocks = (unsigned)((t1 - t0 + TG_BLOCK - 1) / TG_BLOCK);
        hipLaunchKernelGGL(tg_finish_kernel, dim3(blocks), dim3(TG_BLOCK), 0, stream, a, t0, t1);
        GTSFM_CHECK_HIP(hipGetLastError());
    }
    return GTSFM_OK;
}

}  // extern "C"
