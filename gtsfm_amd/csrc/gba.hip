// Global bundle adjustment: one Levenberg-Marquardt over every camera pose and every landmark of a track CSR.
//
// Reference: gtsfm/bundle/bundle_adjustment.py:58-397 (BundleAdjustmentOptimizer.run_ba_stage_with_filtering, run_ba),
// gtsfm/bundle/global_ba.py and gtsfm/common/gtsfm_data.py:389-427 (filter_landmarks), on GTSAM 4.2's
// LevenbergMarquardtOptimizer. The factors, the priors, the retraction, the cheirality treatment and the LM schedule
// are ba2.hip's, generalised from two cameras (camera 0 = identity) to N cameras with an arbitrary first camera; the
// SO(3) / SE(3) helpers are se3.hpp's for both. This entry point holds calibration fixed (k1 = k2 = 0), as
// ba2.hip:19-22 states; gba_calib.hip is the same solver with Cal3Bundler (f, k1, k2) refined, per camera or shared, and
// gba_shared.hpp holds what the two files have in common.
//
// What differs from ba2.hip is the linear solve. The 6C x 6C reduced camera system is never formed: each LM trial
// eliminates the points (3 x 3 blocks, damped) and solves S dc = b by preconditioned conjugate gradients from a zero
// start, the preconditioner being the inverse of the 6 x 6 diagonal blocks of the damped Schur complement. One product
// q = S p is two passes over the per-measurement blocks stored at linearisation (Jx 2 x 6, Jp 2 x 3, b 2: 160 bytes
// per measurement, array of structs):
//   gba_prod_tracks  one lane per track, CSR order:   y_t = Hpp_t^-1 sum_m Jp_m^T (Jx_m p_cam(m))
//   gba_prod_cams    one 256-lane workgroup per camera, walking the camera-major index built once per call by a stable
//                    counting sort:                   q_c = (Hcc_c + lambda I) p_c - sum_m Jx_m^T (Jp_m y_track(m))
//   gba_pcg_step     one workgroup: the dot products, x, r, z = M^-1 r, p.
// Every sum has a fixed order (a lane's strided partial, a 64-lane butterfly, the waves in order: reduce.hpp), there is
// no floating-point atomic, so two calls return the same bytes. The LM and PCG control flow is host code (its decisions
// are lm.hpp's): one small device-to-host read per PCG iteration and per LM trial, so this entry point synchronises its
// stream.
#include <limits.h>
#include <math.h>

#include "common.hpp"

#pragma clang fp contract(off)

#include "csr.hpp"
#include "gba_shared.hpp"
#include "lm.hpp"
#include "reduce.hpp"
#include "se3.hpp"

namespace {

constexpr int kLin = 20;       // doubles per measurement: Jx[12], Jp[6], b[2]
constexpr int kCamBlock = 256;  // lanes of a camera-grouped workgroup
constexpr int kVecBlock = 1024; // lanes of the single-workgroup vector kernels
constexpr int kSortChunksMax = 1024;

// scal[] slots (doubles, device)
enum { S_RR = 0, S_RZ = 1, S_BB = 2, S_OLDLIN = 3, S_NEWLIN = 4, S_NEWERR = 5, S_XI0 = 8, S_COUNT = 16 };
// icnt[] slots (ints, device)
enum { I_NPART = 0, I_NMOD = 1, I_T0 = 2, I_C0 = 3, I_NFAC = 4, I_NKEPT = 5, I_BAD = 6, I_COUNT = 8 };

struct GbaArgs {
    // inputs
    const int* off;
    const int* img;
    const void* uv;
    int uv64;
    const long long* d_nt;
    int T, M, C;
    const double* point_in;
    const uint8_t* tvalid;
    const uint8_t* mvalid;
    const double* wRc;
    const double* wtc;
    const double* intr;
    const uint8_t* cvalid;
    int robust;
    double isig;     // 1 / measurement_sigma
    double prior_w;  // 1 / cam_pose3_prior_sigma^2
    // workspace
    uint8_t* part;      // [T]
    uint8_t* modelled;  // [C]
    int* mtrack;        // [M] track of a factor measurement, -1 otherwise
    int* cam_off;       // [C + 1]
    int* perm;          // [M] camera-major factor measurements
    int* hist;          // [chunks][C]
    int* icnt;          // [I_COUNT]
    double* XA;         // [C][12]
    double* XB;
    double* PA;         // [T][3]
    double* PB;
    double* lin;        // [M][kLin]
    double* Hcc;        // [C][36]
    double* gc;         // [C][6]
    double* Pinv;       // [C][36]
    double* Hpp;        // [T][9] undamped
    double* Minv;       // [T][9]
    double* rp;         // [T][3]
    double* y;          // [T][3]
    double* tl;         // [T]
    double* te;         // [T]
    double* bvec;       // [6C] each
    double* x;
    double* r;
    double* z;
    double* p;
    double* q;
    double* scal;       // [S_COUNT]
    CsrChunks chunks;   // of the sort by camera
};

__device__ __forceinline__ int n_tracks_eff(const GbaArgs& a) {
    if (!a.d_nt) return a.T;
    const long long n = a.d_nt[0];
    return n < 0 ? 0 : (n < (long long)a.T ? (int)n : a.T);
}

__device__ __forceinline__ void load_uv(const GbaArgs& a, int m, double* uv) {
    if (a.uv64) {
        uv[0] = ((const double*)a.uv)[2 * (size_t)m];
        uv[1] = ((const double*)a.uv)[2 * (size_t)m + 1];
    } else {
        uv[0] = ((const float*)a.uv)[2 * (size_t)m];
        uv[1] = ((const float*)a.uv)[2 * (size_t)m + 1];
    }
}

__device__ __forceinline__ bool meas_flag(const GbaArgs& a, int m) { return !a.mvalid || a.mvalid[m] != 0; }
__device__ __forceinline__ bool cam_ok(const GbaArgs& a, int c) {
    return c >= 0 && c < a.C && (!a.cvalid || a.cvalid[c] != 0);
}
__device__ __forceinline__ bool track_range(const GbaArgs& a, int t, int& b, int& e) {
    b = a.off[t];
    e = a.off[t + 1];
    return b >= 0 && e >= b && e <= a.M;
}
__device__ __forceinline__ void load_pose(const double* X, int c, Pose& P) {
    const double* s = X + 12 * (size_t)c;
    for (int k = 0; k < 9; ++k) P.R[k] = s[k];
    for (int k = 0; k < 3; ++k) P.t[k] = s[9 + k];
}

// ------------------------------------------------------------------ setup
__global__ void gba_init(GbaArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        for (int k = 0; k < I_COUNT; ++k) a.icnt[k] = 0;
        a.icnt[I_T0] = INT_MAX;
        a.icnt[I_C0] = INT_MAX;
        for (int k = 0; k < S_COUNT; ++k) a.scal[k] = 0.0;
    }
    if (i < (size_t)a.C) {
        a.modelled[i] = 0;
        for (int k = 0; k < 9; ++k) a.XA[12 * i + k] = a.XB[12 * i + k] = a.wRc[9 * i + k];
        for (int k = 0; k < 3; ++k) a.XA[12 * i + 9 + k] = a.XB[12 * i + 9 + k] = a.wtc[3 * i + k];
    }
    if (i < (size_t)a.T) {
        a.part[i] = 0;
        a.tl[i] = 0.0;
        a.te[i] = 0.0;
        for (int k = 0; k < 3; ++k) a.PA[3 * i + k] = a.PB[3 * i + k] = a.point_in[3 * i + k];
    }
    if (i < (size_t)a.M) a.mtrack[i] = -1;
}

__global__ void gba_setup_tracks(GbaArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tracks_eff(a)) return;
    if (a.tvalid && a.tvalid[t] == 0) return;
    int b, e;
    if (!track_range(a, t, b, e)) return;
    int cnt = 0;
    for (int m = b; m < e; ++m) cnt += meas_flag(a, m) && cam_ok(a, a.img[m]);
    if (cnt < 2) return;
    a.part[t] = 1;
    for (int m = b; m < e; ++m)
        if (meas_flag(a, m) && cam_ok(a, a.img[m])) {
            a.mtrack[m] = t;
            a.modelled[a.img[m]] = 1;
        }
    atomicAdd(&a.icnt[I_NPART], 1);
    atomicMin(&a.icnt[I_T0], t);
    atomicAdd(&a.icnt[I_NFAC], cnt);
}

__global__ void gba_setup_cams(GbaArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    atomicAdd(&a.icnt[I_NMOD], 1);
    atomicMin(&a.icnt[I_C0], c);
}

// ------------------------------------------------------------------ nonlinear error of (X, P): per-track partials
__device__ double track_error(const GbaArgs& a, const double* X, const double* p, int t, int b, int e) {
    double s = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const int c = a.img[m];
        Pose Xc;
        load_pose(X, c, Xc);
        double pc[3], pr[2], uv[2];
        if (!project(Xc, a.intr + 3 * c, p, pc, pr)) continue;
        load_uv(a, m, uv);
        const double dx = pr[0] - uv[0], dy = pr[1] - uv[1];
        const double d = sqrt(dx * dx + dy * dy) * a.isig;
        s += a.robust ? huber_loss(d) : 0.5 * d * d;
    }
    return s;
}

__global__ void gba_eval(GbaArgs a, const double* X, const double* P) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    const double* p = P + 3 * (size_t)t;
    double s = track_error(a, X, p, t, b, e);
    if (t == a.icnt[I_T0])
        for (int k = 0; k < 3; ++k) {
            const double d = p[k] - a.point_in[3 * (size_t)t + k];
            s += 0.5 * d * d * kPointPriorW;
        }
    a.te[t] = s;
}

// scal[S_NEWERR] = sum te + pose prior(Xerr); with_lin: scal[S_NEWLIN] = 0.5 (sum tl + prior row of the step)
__global__ __launch_bounds__(kVecBlock) void gba_reduce(GbaArgs a, const double* Xerr, int with_lin) {
    __shared__ double sh[32];
    double v[2] = {0.0, 0.0};
    for (int t = threadIdx.x; t < a.T; t += kVecBlock) {
        v[0] += a.te[t];
        v[1] += a.tl[t];
    }
    block_sum<2>(v, sh);
    if (threadIdx.x == 0) {
        const int c0 = a.icnt[I_C0];
        Pose A, B;
        for (int k = 0; k < 9; ++k) A.R[k] = a.wRc[9 * (size_t)c0 + k];
        for (int k = 0; k < 3; ++k) A.t[k] = a.wtc[3 * (size_t)c0 + k];
        load_pose(Xerr, c0, B);
        double xi[6], s = 0.0;
        pose_local(A, B, xi);
        for (int k = 0; k < 6; ++k) s += xi[k] * xi[k];
        a.scal[S_NEWERR] = v[0] + 0.5 * s * a.prior_w;
        if (with_lin) {
            double nl = v[1];
            for (int k = 0; k < 6; ++k) {
                const double d = a.x[6 * (size_t)c0 + k] + a.scal[S_XI0 + k];
                nl += d * d * a.prior_w;
            }
            a.scal[S_NEWLIN] = 0.5 * nl;
        }
    }
}

// ------------------------------------------------------------------ linearisation
__global__ void gba_linearize(GbaArgs a, const double* X, const double* P) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.M) return;
    const int t = a.mtrack[m];
    if (t < 0) return;
    const int c = a.img[m];
    Pose Xc;
    load_pose(X, c, Xc);
    double* L = a.lin + (size_t)m * kLin;
    double pc[3], pr[2], uv[2], Jx[12], Jp[6];
    if (!project(Xc, a.intr + 3 * c, P + 3 * (size_t)t, pc, pr)) {
        for (int k = 0; k < kLin; ++k) L[k] = 0.0;
        return;
    }
    project_jac(Xc, a.intr + 3 * c, pc, Jp, Jx);
    load_uv(a, m, uv);
    const double e0 = (pr[0] - uv[0]) * a.isig, e1 = (pr[1] - uv[1]) * a.isig;
    const double sw = a.robust ? sqrt(huber_weight(sqrt(e0 * e0 + e1 * e1))) : 1.0;
    const double s = sw * a.isig;
    for (int k = 0; k < 12; ++k) L[k] = Jx[k] * s;
    for (int k = 0; k < 6; ++k) L[12 + k] = Jp[k] * s;
    L[18] = -sw * e0;
    L[19] = -sw * e1;
}

// per track: undamped Hpp (with the first track's prior), the point right-hand side, the track's share of oldLin
__global__ void gba_track_lin(GbaArgs a, const double* P) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, rp[3] = {0, 0, 0}, ol = 0.0;
    if (t == a.icnt[I_T0])
        for (int k = 0; k < 3; ++k) {
            const double d = P[3 * (size_t)t + k] - a.point_in[3 * (size_t)t + k];
            H[4 * k] += kPointPriorW;
            rp[k] += -d * kPointPriorW;
            ol += d * d * kPointPriorW;
        }
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const double* L = a.lin + (size_t)m * kLin;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double* jp = L + 12 + 3 * r;
            const double br = L[18 + r];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                rp[k] += jp[k] * br;
#pragma unroll
                for (int l = 0; l < 3; ++l) H[3 * k + l] += jp[k] * jp[l];
            }
            ol += br * br;
        }
    }
    for (int k = 0; k < 9; ++k) a.Hpp[9 * (size_t)t + k] = H[k];
    for (int k = 0; k < 3; ++k) a.rp[3 * (size_t)t + k] = rp[k];
    a.tl[t] = ol;
}

// per camera: Hcc = sum Jx^T Jx (+ the pose prior on the first camera), gc = sum Jx^T b (- prior); block c0 also
// stores the prior's residual xi0 = Logmap(X0^-1 X)
__global__ __launch_bounds__(kCamBlock) void gba_cam_lin(GbaArgs a, const double* X) {
    __shared__ double sh[16 * 27];
    const int c = blockIdx.x;
    if (!a.modelled[c]) return;
    double v[27];
    for (int k = 0; k < 27; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const double* L = a.lin + (size_t)a.perm[i] * kLin;
        int n = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int s = r; s < 6; ++s, ++n) v[n] += L[r] * L[s] + L[6 + r] * L[6 + s];
            v[21 + r] += L[r] * L[18] + L[6 + r] * L[19];
        }
    }
    block_sum<27>(v, sh);
    if (threadIdx.x == 0) {
        double* H = a.Hcc + 36 * (size_t)c;
        double* g = a.gc + 6 * (size_t)c;
        int n = 0;
        for (int r = 0; r < 6; ++r)
            for (int s = r; s < 6; ++s, ++n) H[6 * r + s] = H[6 * s + r] = v[n];
        for (int r = 0; r < 6; ++r) g[r] = v[21 + r];
        if (c == a.icnt[I_C0]) {
            Pose A, B;
            for (int k = 0; k < 9; ++k) A.R[k] = a.wRc[9 * (size_t)c + k];
            for (int k = 0; k < 3; ++k) A.t[k] = a.wtc[3 * (size_t)c + k];
            load_pose(X, c, B);
            double xi[6];
            pose_local(A, B, xi);
            for (int k = 0; k < 6; ++k) {
                a.scal[S_XI0 + k] = xi[k];
                H[7 * k] += a.prior_w;
                g[k] += -xi[k] * a.prior_w;
            }
        }
    }
}

// scal[S_OLDLIN] = 0.5 (sum tl + |xi0|^2 / sigma^2); runs after gba_track_lin and gba_cam_lin
__global__ __launch_bounds__(kVecBlock) void gba_oldlin(GbaArgs a) {
    __shared__ double sh[16];
    double v[1] = {0.0};
    for (int t = threadIdx.x; t < a.T; t += kVecBlock) v[0] += a.tl[t];
    block_sum<1>(v, sh);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += a.scal[S_XI0 + k] * a.scal[S_XI0 + k];
        a.scal[S_OLDLIN] = 0.5 * (v[0] + s * a.prior_w);
    }
}

// ------------------------------------------------------------------ one LM trial: damping, preconditioner, rhs
__global__ void gba_track_damp(GbaArgs a, double lambda) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    double H[9];
    for (int k = 0; k < 9; ++k) H[k] = a.Hpp[9 * (size_t)t + k];
    for (int k = 0; k < 3; ++k) H[4 * k] += lambda;
    double Mi[9];
    if (!inv3(H, Mi)) {
        for (int k = 0; k < 9; ++k) Mi[k] = 0.0;
        a.icnt[I_BAD] = 1;
    }
    for (int k = 0; k < 9; ++k) a.Minv[9 * (size_t)t + k] = Mi[k];
}

// per camera: the 6 x 6 diagonal block of the damped Schur complement, inverted (the preconditioner), and the reduced
// right-hand side b_c = gc - sum W Hpp^-1 rp, W = Jx^T Jp
__global__ __launch_bounds__(kCamBlock) void gba_cam_build(GbaArgs a, double lambda) {
    __shared__ double sh[16 * 27];
    const int c = blockIdx.x;
    if (!a.modelled[c]) {
        if (threadIdx.x < 36) a.Pinv[36 * (size_t)c + threadIdx.x] = 0.0;
        if (threadIdx.x < 6) a.bvec[6 * (size_t)c + threadIdx.x] = 0.0;
        return;
    }
    double v[27];
    for (int k = 0; k < 27; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const int m = a.perm[i];
        const double* L = a.lin + (size_t)m * kLin;
        const size_t t = (size_t)a.mtrack[m];
        const double* Mi = a.Minv + 9 * t;
        const double* rp = a.rp + 3 * t;
        double W[18], WM[18], Mr[3];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) W[3 * r + k] = L[r] * L[12 + k] + L[6 + r] * L[15 + k];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                WM[3 * r + k] = W[3 * r] * Mi[k] + W[3 * r + 1] * Mi[3 + k] + W[3 * r + 2] * Mi[6 + k];
        mv3(Mi, rp, Mr);
        int n = 0;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int s = r; s < 6; ++s, ++n)
                v[n] += WM[3 * r] * W[3 * s] + WM[3 * r + 1] * W[3 * s + 1] + WM[3 * r + 2] * W[3 * s + 2];
            v[21 + r] += W[3 * r] * Mr[0] + W[3 * r + 1] * Mr[1] + W[3 * r + 2] * Mr[2];
        }
    }
    block_sum<27>(v, sh);
    if (threadIdx.x == 0) {
        const double* H = a.Hcc + 36 * (size_t)c;
        double S[36], Inv[36];
        int n = 0;
        for (int r = 0; r < 6; ++r)
            for (int s = r; s < 6; ++s, ++n) S[6 * r + s] = S[6 * s + r] = H[6 * r + s] - v[n];
        for (int k = 0; k < 6; ++k) S[7 * k] += lambda;
        if (!spd_inverse<6>(S, Inv)) {
            for (int k = 0; k < 36; ++k) Inv[k] = 0.0;
            a.icnt[I_BAD] = 1;
        }
        for (int k = 0; k < 36; ++k) a.Pinv[36 * (size_t)c + k] = Inv[k];
        for (int r = 0; r < 6; ++r) a.bvec[6 * (size_t)c + r] = a.gc[6 * (size_t)c + r] - v[21 + r];
    }
}

// ------------------------------------------------------------------ PCG
__device__ __forceinline__ double precond_row(const GbaArgs& a, int i) {
    const int c = i / 6, k = i - 6 * c;
    const double* Pm = a.Pinv + 36 * (size_t)c + 6 * k;
    const double* rc = a.r + 6 * (size_t)c;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j) s += Pm[j] * rc[j];
    return s;
}

__global__ __launch_bounds__(kVecBlock) void gba_pcg_init(GbaArgs a) {
    __shared__ double sh[32];
    const int n = 6 * a.C;
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        a.x[i] = 0.0;
        a.r[i] = a.bvec[i];
    }
    __syncthreads();
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        const double zi = precond_row(a, i), ri = a.r[i];
        a.z[i] = zi;
        a.p[i] = zi;
        v[0] += ri * ri;
        v[1] += ri * zi;
    }
    block_sum<2>(v, sh);
    if (threadIdx.x == 0) {
        a.scal[S_RR] = v[0];
        a.scal[S_RZ] = v[1];
        a.scal[S_BB] = v[0];
    }
}

// y_t = Hpp_t^-1 sum_m Jp_m^T (Jx_m p_cam(m)): one lane per track, CSR order. vec is p (a product) or the solved step
// x (back-substitution reuses the inner sum).
__device__ __forceinline__ void track_wtx(const GbaArgs& a, const double* vec, int t, int b, int e, double* s) {
    s[0] = s[1] = s[2] = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const double* L = a.lin + (size_t)m * kLin;
        const double* pc = vec + 6 * (size_t)a.img[m];
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            u0 += L[k] * pc[k];
            u1 += L[6 + k] * pc[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += L[12 + k] * u0 + L[15 + k] * u1;
    }
}

__global__ void gba_prod_tracks(GbaArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    double s[3], y[3];
    track_wtx(a, a.p, t, b, e, s);
    mv3(a.Minv + 9 * (size_t)t, s, y);
    for (int k = 0; k < 3; ++k) a.y[3 * (size_t)t + k] = y[k];
}

// q_c = (Hcc_c + lambda I) p_c - sum_m Jx_m^T (Jp_m y_track(m)): one workgroup per camera over the camera-major index
__global__ __launch_bounds__(kCamBlock) void gba_prod_cams(GbaArgs a, double lambda) {
    __shared__ double sh[16 * 6];
    const int c = blockIdx.x;
    if (!a.modelled[c]) {
        if (threadIdx.x < 6) a.q[6 * (size_t)c + threadIdx.x] = 0.0;
        return;
    }
    double v[6] = {0, 0, 0, 0, 0, 0};
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const int m = a.perm[i];
        const double* L = a.lin + (size_t)m * kLin;
        const double* y = a.y + 3 * (size_t)a.mtrack[m];
        const double u0 = L[12] * y[0] + L[13] * y[1] + L[14] * y[2];
        const double u1 = L[15] * y[0] + L[16] * y[1] + L[17] * y[2];
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += L[k] * u0 + L[6 + k] * u1;
    }
    block_sum<6>(v, sh);
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        const double* H = a.Hcc + 36 * (size_t)c + 6 * k;
        const double* pc = a.p + 6 * (size_t)c;
        double s = 0.0;
        for (int j = 0; j < 6; ++j) s += H[j] * pc[j];
        s += lambda * pc[k];
        a.q[6 * (size_t)c + k] = s - v[k];
    }
}

__global__ __launch_bounds__(kVecBlock) void gba_pcg_step(GbaArgs a) {
    __shared__ double sh[32];
    const int n = 6 * a.C;
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += kVecBlock) v[0] += a.p[i] * a.q[i];
    block_sum<1>(v, sh);
    const double rz = a.scal[S_RZ];
    const double alpha = rz / v[0];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        a.x[i] = a.x[i] + alpha * a.p[i];
        a.r[i] = a.r[i] - alpha * a.q[i];
    }
    __syncthreads();
    v[0] = v[1] = 0.0;
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        const double zi = precond_row(a, i), ri = a.r[i];
        a.z[i] = zi;
        v[0] += ri * ri;
        v[1] += ri * zi;
    }
    block_sum<2>(v, sh);
    const double beta = v[1] / rz;
    for (int i = threadIdx.x; i < n; i += kVecBlock) a.p[i] = a.z[i] + beta * a.p[i];
    if (threadIdx.x == 0) {
        a.scal[S_RR] = v[0];
        a.scal[S_RZ] = v[1];
    }
}

// ------------------------------------------------------------------ the step: retraction, back-substitution, costs
__global__ void gba_retract(GbaArgs a, const double* X, double* Xn) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    Pose A, B;
    load_pose(X, c, A);
    pose_retract(A, a.x + 6 * (size_t)c, B);
    for (int k = 0; k < 9; ++k) Xn[12 * (size_t)c + k] = B.R[k];
    for (int k = 0; k < 3; ++k) Xn[12 * (size_t)c + 9 + k] = B.t[k];
}

__global__ void gba_backsub(GbaArgs a, const double* Xn, const double* P, double* Pn) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    double s[3], q[3], dp[3], pn[3];
    track_wtx(a, a.x, t, b, e, s);
    for (int k = 0; k < 3; ++k) q[k] = a.rp[3 * (size_t)t + k] - s[k];
    mv3(a.Minv + 9 * (size_t)t, q, dp);
    for (int k = 0; k < 3; ++k) {
        pn[k] = P[3 * (size_t)t + k] + dp[k];
        Pn[3 * (size_t)t + k] = pn[k];
    }
    double nl = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const double* L = a.lin + (size_t)m * kLin;
        const double* dc = a.x + 6 * (size_t)a.img[m];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double v = -L[18 + r];
#pragma unroll
            for (int k = 0; k < 6; ++k) v += L[6 * r + k] * dc[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) v += L[12 + 3 * r + k] * dp[k];
            nl += v * v;
        }
    }
    double ne = track_error(a, Xn, pn, t, b, e);
    if (t == a.icnt[I_T0])
        for (int k = 0; k < 3; ++k) {
            const double d0 = P[3 * (size_t)t + k] - a.point_in[3 * (size_t)t + k];
            const double v = dp[k] + d0, d1 = pn[k] - a.point_in[3 * (size_t)t + k];
            nl += v * v * kPointPriorW;
            ne += 0.5 * d1 * d1 * kPointPriorW;
        }
    a.tl[t] = nl;
    a.te[t] = ne;
}

// ------------------------------------------------------------------ outputs
__global__ void gba_filter(GbaArgs a, const double* X, const double* P, double thresh, uint8_t* track_keep,
                           uint8_t* cam_keep) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    bool good = true;
    // an infinite threshold is the reference's reproj_error_thresh None: no filter, every optimised track is valid
    // (bundle_adjustment.py:346-355), without the cheirality test of filter_landmarks
    for (int m = b; m < e && good && isfinite(thresh); ++m) {
        if (!meas_flag(a, m)) continue;
        const int c = a.img[m];
        if (!cam_ok(a, c)) { good = false; break; }
        Pose Xc;
        load_pose(X, c, Xc);
        double pc[3], pr[2], uv[2];
        if (!project(Xc, a.intr + 3 * c, P + 3 * (size_t)t, pc, pr)) { good = false; break; }
        load_uv(a, m, uv);
        const double dx = pr[0] - uv[0], dy = pr[1] - uv[1];
        if (!(sqrt(dx * dx + dy * dy) < thresh)) good = false;
    }
    if (!good) return;
    track_keep[t] = 1;
    atomicAdd(&a.icnt[I_NKEPT], 1);
    for (int m = b; m < e; ++m)
        if (meas_flag(a, m) && cam_ok(a, a.img[m])) cam_keep[a.img[m]] = 1;
}

__global__ void gba_output(GbaArgs a, const double* X, const double* P, double* wRc_out, double* wtc_out,
                           double* point_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)a.C) {
        for (int k = 0; k < 9; ++k) wRc_out[9 * i + k] = X[12 * i + k];
        for (int k = 0; k < 3; ++k) wtc_out[3 * i + k] = X[12 * i + 9 + k];
    }
    if (i < (size_t)a.T)
        for (int k = 0; k < 3; ++k) point_out[3 * i + k] = P[3 * i + k];
}

__global__ void gba_stats(GbaArgs a, double* stats, double err0, double err, double iters, double trials,
                          double pcg_iters, double cap_hits, double status) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    stats[0] = err0;
    stats[1] = err;
    stats[2] = iters;
    stats[3] = trials;
    stats[4] = pcg_iters;
    stats[5] = cap_hits;
    stats[6] = (double)a.icnt[I_NMOD];
    stats[7] = (double)a.icnt[I_NPART];
    stats[8] = (double)a.icnt[I_NKEPT];
    stats[9] = status;
}

// ------------------------------------------------------------------ workspace
struct GbaLayout {
    size_t part, modelled, mtrack, cam_off, perm, hist, icnt, XA, XB, PA, PB, lin, Hcc, gc, Pinv, Hpp, Minv, rp, y, tl,
        te, vec, scal, total;
    CsrChunks chunks;
};

bool gba_sizes_ok(long long n_tracks, long long n_meas, int n_img) {
    return n_tracks > 0 && n_meas > 0 && n_img > 0 && n_tracks < (1ll << 31) - 1 && n_meas < (1ll << 31) - 1 &&
           n_img <= (1 << 20);
}

GbaLayout gba_layout(long long T, long long M, int C) {
    GbaLayout L;
    L.chunks = csr_chunks(M, kSortChunksMax);
    WsCarver w;
    const size_t t = (size_t)T, m = (size_t)M, c = (size_t)C, d = sizeof(double);
    L.part = w.take(t);
    L.modelled = w.take(c);
    L.mtrack = w.take(m * 4);
    L.cam_off = w.take((c + 1) * 4);
    L.perm = w.take(m * 4);
    L.hist = w.take(csr_hist_bytes(L.chunks, c));
    L.icnt = w.take(I_COUNT * 4);
    L.XA = w.take(c * 12 * d);
    L.XB = w.take(c * 12 * d);
    L.PA = w.take(t * 3 * d);
    L.PB = w.take(t * 3 * d);
    L.lin = w.take(m * kLin * d);
    L.Hcc = w.take(c * 36 * d);
    L.gc = w.take(c * 6 * d);
    L.Pinv = w.take(c * 36 * d);
    L.Hpp = w.take(t * 9 * d);
    L.Minv = w.take(t * 9 * d);
    L.rp = w.take(t * 3 * d);
    L.y = w.take(t * 3 * d);
    L.tl = w.take(t * d);
    L.te = w.take(t * d);
    L.vec = w.take(6 * c * 6 * d);
    L.scal = w.take(S_COUNT * d);
    L.total = w.o;
    return L;
}

}  // namespace

extern "C" {

size_t gtsfm_global_ba_workspace_bytes(long long n_tracks, long long n_meas, int n_img) {
    if (!gba_sizes_ok(n_tracks, n_meas, n_img)) return 0;
    return gba_layout(n_tracks, n_meas, n_img).total;
}

int gtsfm_global_ba(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                    long long n_tracks, const long long* d_n_tracks, long long n_meas, const double* d_point,
                    const uint8_t* d_track_valid, const uint8_t* d_meas_valid, const double* d_wRc,
                    const double* d_wtc, const double* d_intrinsics, const uint8_t* d_cam_valid, int n_img, int robust,
                    double measurement_sigma, double cam_pose3_prior_sigma, int max_iterations, double pcg_rel_tol,
                    int pcg_max_iter, double reproj_error_thresh, void* d_workspace, size_t workspace_bytes,
                    double* d_wRc_out, double* d_wtc_out, double* d_point_out, uint8_t* d_track_keep,
                    uint8_t* d_cam_keep, double* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_tracks < 0 || n_meas < 0 || n_img < 0 || n_tracks >= (1ll << 31) - 1 || n_meas >= (1ll << 31) - 1 ||
        n_img > (1 << 20) || !d_wRc_out || !d_wtc_out || !d_point_out || !d_track_keep || !d_cam_keep || !d_stats ||
        !(measurement_sigma > 0) || !(cam_pose3_prior_sigma > 0) || max_iterations < 0 || !(pcg_rel_tol > 0) ||
        pcg_max_iter <= 0 || !(reproj_error_thresh > 0) || (uv_is_f64 != 0 && uv_is_f64 != 1))
        return GTSFM_ERR_ARG;
    if ((n_img > 0 && (!d_wRc || !d_wtc || !d_intrinsics)) || (n_tracks > 0 && (!d_track_offsets || !d_point)) ||
        (n_meas > 0 && (!d_track_img || !d_track_uv)))
        return GTSFM_ERR_ARG;
    const int T = (int)n_tracks, M = (int)n_meas, C = n_img;
    const double nothing[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    // the reference's early return (bundle_adjustment.py:319-324): inputs copied through, keep all zero, error 0
    auto copy_through = [&]() -> int {
        if (C > 0) {
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_wRc_out, d_wRc, (size_t)C * 9 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_wtc_out, d_wtc, (size_t)C * 3 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            GTSFM_CHECK_HIP(hipMemsetAsync(d_cam_keep, 0, (size_t)C, stream));
        }
        if (T > 0) {
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_point_out, d_point, (size_t)T * 3 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            GTSFM_CHECK_HIP(hipMemsetAsync(d_track_keep, 0, (size_t)T, stream));
        }
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_stats, nothing, sizeof(nothing), hipMemcpyHostToDevice, stream));
        GTSFM_CHECK_HIP(hipStreamSynchronize(stream));  // `nothing` lives on this stack frame
        return GTSFM_OK;
    };
    if (T == 0 || M == 0 || C == 0) return copy_through();
    if (!d_workspace) return GTSFM_ERR_ARG;
    const GbaLayout L = gba_layout(T, M, C);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    GbaArgs a;
    a.off = d_track_offsets; a.img = d_track_img; a.uv = d_track_uv; a.uv64 = uv_is_f64; a.d_nt = d_n_tracks;
    a.T = T; a.M = M; a.C = C;
    a.point_in = d_point; a.tvalid = d_track_valid; a.mvalid = d_meas_valid;
    a.wRc = d_wRc; a.wtc = d_wtc; a.intr = d_intrinsics; a.cvalid = d_cam_valid;
    a.robust = robust != 0;
    a.isig = 1.0 / measurement_sigma;
    a.prior_w = 1.0 / (cam_pose3_prior_sigma * cam_pose3_prior_sigma);
    a.part = ws + L.part; a.modelled = ws + L.modelled;
    a.mtrack = (int*)(ws + L.mtrack); a.cam_off = (int*)(ws + L.cam_off); a.perm = (int*)(ws + L.perm);
    a.hist = (int*)(ws + L.hist); a.icnt = (int*)(ws + L.icnt);
    a.XA = (double*)(ws + L.XA); a.XB = (double*)(ws + L.XB);
    a.PA = (double*)(ws + L.PA); a.PB = (double*)(ws + L.PB);
    a.lin = (double*)(ws + L.lin); a.Hcc = (double*)(ws + L.Hcc); a.gc = (double*)(ws + L.gc);
    a.Pinv = (double*)(ws + L.Pinv); a.Hpp = (double*)(ws + L.Hpp); a.Minv = (double*)(ws + L.Minv);
    a.rp = (double*)(ws + L.rp); a.y = (double*)(ws + L.y); a.tl = (double*)(ws + L.tl);
    a.te = (double*)(ws + L.te);
    double* vec = (double*)(ws + L.vec);
    const size_t n6 = 6 * (size_t)C;
    a.bvec = vec; a.x = vec + n6; a.r = vec + 2 * n6; a.z = vec + 3 * n6; a.p = vec + 4 * n6; a.q = vec + 5 * n6;
    a.scal = (double*)(ws + L.scal);
    a.chunks = L.chunks;

    const unsigned B = 256;
    const unsigned gT = blocks_for(T, B), gM = blocks_for(M, B), gC = blocks_for(C, B);
    const size_t nmax = (size_t)(T > M ? T : M) > (size_t)C ? (size_t)(T > M ? T : M) : (size_t)C;
    int icnt[I_COUNT];
    double scal[6];
    auto read_icnt = [&]() { return read_back(icnt, a.icnt, I_COUNT, stream); };
    auto read_scal = [&]() { return read_back(scal, a.scal, 6, stream); };

    hipLaunchKernelGGL(gba_init, dim3(blocks_for(nmax, B)), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(gba_setup_tracks, dim3(gT), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(gba_setup_cams, dim3(gC), dim3(B), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    int rc = read_icnt();
    if (rc != GTSFM_OK) return rc;
    if (icnt[I_NPART] == 0 || icnt[I_NMOD] == 0) return copy_through();

    if ((rc = csr_build(GbaByCamera{a.mtrack, a.img, a.perm}, M, C, a.chunks, a.hist, a.cam_off, stream)) != GTSFM_OK)
        return rc;

    double* X = a.XA;
    double* Xn = a.XB;
    double* P = a.PA;
    double* Pn = a.PB;
    hipLaunchKernelGGL(gba_eval, dim3(gT), dim3(B), 0, stream, a, X, P);
    hipLaunchKernelGGL(gba_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, X, 0);
    GTSFM_CHECK_HIP(hipGetLastError());
    if ((rc = read_scal()) != GTSFM_OK) return rc;
    const double err0 = scal[S_NEWERR];
    double err = err0, lambda = 1e-5;
    const int max_iters = max_iterations > 0 ? max_iterations : 100;
    long long iters = 0, trials = 0, pcg_total = 0, cap_hits = 0;
    if (err > 0.0) {
        for (;;) {  // ends: every outer step either accepts (iters <= max_iters) or leaves err unchanged (dec = 0)
            const double cur = err;
            hipLaunchKernelGGL(gba_linearize, dim3(gM), dim3(B), 0, stream, a, X, P);
            hipLaunchKernelGGL(gba_track_lin, dim3(gT), dim3(B), 0, stream, a, P);
            hipLaunchKernelGGL(gba_cam_lin, dim3(C), dim3(kCamBlock), 0, stream, a, X);
            hipLaunchKernelGGL(gba_oldlin, dim3(1), dim3(kVecBlock), 0, stream, a);
            double oldLin = 0.0;
            bool have_oldlin = false;
            for (int inner = 0; inner < kInnerMax; ++inner) {
                ++trials;
                GTSFM_CHECK_HIP(hipMemsetAsync(a.icnt + I_BAD, 0, sizeof(int), stream));
                hipLaunchKernelGGL(gba_track_damp, dim3(gT), dim3(B), 0, stream, a, lambda);
                hipLaunchKernelGGL(gba_cam_build, dim3(C), dim3(kCamBlock), 0, stream, a, lambda);
                hipLaunchKernelGGL(gba_pcg_init, dim3(1), dim3(kVecBlock), 0, stream, a);
                GTSFM_CHECK_HIP(hipGetLastError());
                if ((rc = read_icnt()) != GTSFM_OK) return rc;
                LmTrial trial;
                if (!icnt[I_BAD]) {
                    if ((rc = read_scal()) != GTSFM_OK) return rc;
                    if (!have_oldlin) {
                        oldLin = scal[S_OLDLIN];
                        have_oldlin = true;
                    }
                    rc = pcg_iterate(scal[S_BB], scal[S_RR], pcg_rel_tol, pcg_max_iter, pcg_total, cap_hits,
                                     [&](double& rr) -> int {
                        hipLaunchKernelGGL(gba_prod_tracks, dim3(gT), dim3(B), 0, stream, a);
                        hipLaunchKernelGGL(gba_prod_cams, dim3(C), dim3(kCamBlock), 0, stream, a, lambda);
                        hipLaunchKernelGGL(gba_pcg_step, dim3(1), dim3(kVecBlock), 0, stream, a);
                        GTSFM_CHECK_HIP(hipGetLastError());
                        const int rc2 = read_scal();
                        rr = scal[S_RR];
                        return rc2;
                    });
                    if (rc != GTSFM_OK) return rc;
                    hipLaunchKernelGGL(gba_retract, dim3(gC), dim3(B), 0, stream, a, X, Xn);
                    hipLaunchKernelGGL(gba_backsub, dim3(gT), dim3(B), 0, stream, a, Xn, P, Pn);
                    hipLaunchKernelGGL(gba_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, Xn, 1);
                    GTSFM_CHECK_HIP(hipGetLastError());
                    if ((rc = read_scal()) != GTSFM_OK) return rc;
                    trial = lm_judge(err, oldLin, scal[S_NEWLIN], scal[S_NEWERR]);
                }
                if (trial.success) {
                    double* s = X; X = Xn; Xn = s;
                    s = P; P = Pn; Pn = s;
                    err = trial.newErr;
                    ++iters;
                }
                if (lm_trials_done(trial, lambda)) break;
            }
            if (lm_done(cur, err, iters, max_iters)) break;
        }
    }
    GTSFM_CHECK_HIP(hipMemsetAsync(d_track_keep, 0, (size_t)T, stream));
    GTSFM_CHECK_HIP(hipMemsetAsync(d_cam_keep, 0, (size_t)C, stream));
    hipLaunchKernelGGL(gba_filter, dim3(gT), dim3(B), 0, stream, a, X, P, reproj_error_thresh, d_track_keep,
                       d_cam_keep);
    hipLaunchKernelGGL(gba_output, dim3(blocks_for(T > C ? T : C, B)), dim3(B), 0, stream, a, X, P, d_wRc_out,
                       d_wtc_out, d_point_out);
    hipLaunchKernelGGL(gba_stats, dim3(1), dim3(64), 0, stream, a, d_stats, err0, err, (double)iters, (double)trials,
                       (double)pcg_total, (double)cap_hits, 0.0);
    GTSFM_CHECK_HIP(hipGetLastError());
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    return GTSFM_OK;
}

}  // extern "C"
