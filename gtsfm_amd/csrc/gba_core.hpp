// The global bundle adjustment solver, written once for both entry points: gba.hip (calibration fixed) and gba_calib.hip
// (Cal3Bundler f, k1, k2 refined, per camera or shared). Every kernel, the workspace layout, the argument checks and the
// host LM / PCG driver are templates on a camera model, chosen at compile time; there is no runtime flag. The includer's
// file comment describes its algorithm; this one describes what a model is.
//
// A model Mdl provides
//   kCal            calibration columns of a camera's block, 0 or 3; a block is N = 6 + kCal wide
//   kCamStride      doubles per camera of the parameter array the projection reads (3 for intr, 5 for calib)
//   kStats          doubles of the stats output
//   struct Extra    the arguments only this model has; GbaArgs<Mdl> inherits them. Empty for the fixed model, which so
//                   has no calibration variable, no shared mode, no wider reduction and no larger workspace
//   project(X, K, p, pc, uv), project_jac(X, K, pc, Jp, Jx, Jk)
// and, when kCal > 0, the hooks that the kernels below call inside `if constexpr (kCal > 0)`: the calibration prior, the
// shared mode's border, the retraction of K, its workspace and its extra stats (gba_calib.hip lists them).
//
// A measurement's record is Jx[12] | Jk[2 kCal] | Jp[6] | b[2] doubles: 160 bytes with kCal = 0, 208 with kCal = 3.
//
// Summation order is part of the contract: the includers compile with fp contract(off) and there is no floating-point
// atomic, so the order written here fixes the output bytes. Sets no fp-contract pragma itself: include it after the
// includer's own, and after nothing that sets one (see se3.hpp).
#pragma once
#include <limits.h>
#include <math.h>

#include "common.hpp"
#include "csr.hpp"
#include "lm.hpp"
#include "reduce.hpp"
#include "se3.hpp"

namespace {

constexpr double kPointPriorW = 100.0;  // PriorFactorPoint3 sigma 0.1
constexpr int kCamBlock = 256;          // lanes of a camera-grouped workgroup
constexpr int kVecBlock = 1024;         // lanes of the single-workgroup vector kernels
constexpr int kSortChunksMax = 1024;

// scal[] slots (doubles, device)
enum { S_RR = 0, S_RZ = 1, S_BB = 2, S_OLDLIN = 3, S_NEWLIN = 4, S_NEWERR = 5, S_XI0 = 8, S_COUNT = 16 };
// icnt[] slots (ints, device)
enum { I_NPART = 0, I_NMOD = 1, I_T0 = 2, I_C0 = 3, I_NFAC = 4, I_NKEPT = 5, I_BAD = 6, I_COUNT = 8 };

// the widths that follow from a model's kCal
template <class Mdl>
struct GbaDims {
    static constexpr int kCal = Mdl::kCal;
    static constexpr int N = 6 + kCal;           // columns of a camera's block
    static constexpr int kSym = N * (N + 1) / 2;  // upper triangle of an N x N
    static constexpr int kJk = 12, kJp = 12 + 2 * kCal, kB = kJp + 6;
    static constexpr int kLin = kB + 2;          // doubles per measurement
};

template <class Mdl>
struct GbaArgs : Mdl::Extra {
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
    const double* cam;  // [C][kCamStride] as passed in: intr (f, u0, v0) or calib (f, k1, k2, u0, v0)
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
    double* H;          // [C][N * N] sum J^T J of the camera's block, J = [Jx | Jk]
    double* g;          // [C][N]
    double* Pinv;       // [C][N * N]; shared mode: the 6 x 6 in the first 36
    double* Hpp;        // [T][9] undamped
    double* Minv;       // [T][9]
    double* rp;         // [T][3]
    double* y;          // [T][3]
    double* tl;         // [T]
    double* te;         // [T]
    double* bvec;       // [gba_vec_len] each
    double* x;
    double* r;
    double* z;
    double* p;
    double* q;
    double* scal;       // [S_COUNT]
    CsrChunks chunks;   // of the sort by camera
};

// ------------------------------------------------------------------ accessors
// the refined model's shared mode: the unknown is [6C poses | 3], not [C][N]
template <class Mdl>
__device__ __forceinline__ bool is_shared(const GbaArgs<Mdl>& a) {
    if constexpr (Mdl::kCal > 0) return a.shared != 0;
    else return false;
}
template <class Mdl>
__device__ __forceinline__ int nvec(const GbaArgs<Mdl>& a) {
    return is_shared(a) ? 6 * a.C + Mdl::kCal : GbaDims<Mdl>::N * a.C;
}
// the pose and the calibration entries of camera c in an unknown-sized vector
template <class Mdl>
__device__ __forceinline__ const double* vec_pose(const GbaArgs<Mdl>& a, const double* v, int c) {
    return v + (size_t)(is_shared(a) ? 6 : GbaDims<Mdl>::N) * c;
}
template <class Mdl>
__device__ __forceinline__ const double* vec_calib(const GbaArgs<Mdl>& a, const double* v, int c) {
    return is_shared(a) ? v + 6 * (size_t)a.C : v + (size_t)GbaDims<Mdl>::N * c + 6;
}

template <class Mdl>
__device__ __forceinline__ int n_tracks_eff(const GbaArgs<Mdl>& a) {
    if (!a.d_nt) return a.T;
    const long long n = a.d_nt[0];
    return n < 0 ? 0 : (n < (long long)a.T ? (int)n : a.T);
}

template <class Mdl>
__device__ __forceinline__ void load_uv(const GbaArgs<Mdl>& a, int m, double* uv) {
    if (a.uv64) {
        uv[0] = ((const double*)a.uv)[2 * (size_t)m];
        uv[1] = ((const double*)a.uv)[2 * (size_t)m + 1];
    } else {
        uv[0] = ((const float*)a.uv)[2 * (size_t)m];
        uv[1] = ((const float*)a.uv)[2 * (size_t)m + 1];
    }
}

template <class Mdl>
__device__ __forceinline__ bool meas_flag(const GbaArgs<Mdl>& a, int m) {
    return !a.mvalid || a.mvalid[m] != 0;
}
template <class Mdl>
__device__ __forceinline__ bool cam_ok(const GbaArgs<Mdl>& a, int c) {
    return c >= 0 && c < a.C && (!a.cvalid || a.cvalid[c] != 0);
}
template <class Mdl>
__device__ __forceinline__ bool track_range(const GbaArgs<Mdl>& a, int t, int& b, int& e) {
    b = a.off[t];
    e = a.off[t + 1];
    return b >= 0 && e >= b && e <= a.M;
}
__device__ __forceinline__ void load_pose(const double* X, int c, Pose& P) {
    const double* s = X + 12 * (size_t)c;
    for (int k = 0; k < 9; ++k) P.R[k] = s[k];
    for (int k = 0; k < 3; ++k) P.t[k] = s[9 + k];
}

// entry a of row r of J = [Jx | Jk] in a measurement's record; with kCal = 0 it is L[6 r + a]
template <class Mdl>
__device__ __forceinline__ double jn(const double* L, int r, int a) {
    return a < 6 ? L[6 * r + a] : L[GbaDims<Mdl>::kJk + Mdl::kCal * r + (a - 6)];
}

// Logmap(A^-1 B): the pose prior's residual at B for a prior at A (ba2.hip has A = identity)
__device__ void pose_local(const Pose& A, const Pose& B, double* xi) {
    Pose T;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            T.R[3 * i + j] = A.R[i] * B.R[j] + A.R[3 + i] * B.R[3 + j] + A.R[6 + i] * B.R[6 + j];
    const double d[3] = {B.t[0] - A.t[0], B.t[1] - A.t[1], B.t[2] - A.t[2]};
    mtv3(A.R, d, T.t);
    pose_log(T, xi);
}

// the pose prior's residual at X: the first modelled camera c0 is held at its input pose
template <class Mdl>
__device__ __forceinline__ void pose_prior_residual(const GbaArgs<Mdl>& a, const double* X, int c0, double* xi) {
    Pose A, B;
    for (int k = 0; k < 9; ++k) A.R[k] = a.wRc[9 * (size_t)c0 + k];
    for (int k = 0; k < 3; ++k) A.t[k] = a.wtc[3 * (size_t)c0 + k];
    load_pose(X, c0, B);
    pose_local(A, B, xi);
}

// inverse of a symmetric positive definite N x N (full storage, row stride N) by Cholesky; false when it is not
// positive definite
template <int N>
__device__ bool spd_inverse(const double* S, double* Inv) {
    double L[N * N];
    for (int k = 0; k < N * N; ++k) L[k] = S[k];
    for (int j = 0; j < N; ++j) {
        double v = L[(N + 1) * j];
        for (int k = 0; k < j; ++k) v -= L[N * j + k] * L[N * j + k];
        if (!(v > 0.0) || !isfinite(v)) return false;
        const double d = sqrt(v);
        L[(N + 1) * j] = d;
        for (int i = j + 1; i < N; ++i) {
            double w = L[N * i + j];
            for (int k = 0; k < j; ++k) w -= L[N * i + k] * L[N * j + k];
            L[N * i + j] = w / d;
        }
    }
    for (int c = 0; c < N; ++c) {
        double s[N];
        for (int i = 0; i < N; ++i) {
            double v = (i == c) ? 1.0 : 0.0;
            for (int k = 0; k < i; ++k) v -= L[N * i + k] * s[k];
            s[i] = v / L[(N + 1) * i];
        }
        for (int i = N - 1; i >= 0; --i) {
            double v = s[i];
            for (int k = i + 1; k < N; ++k) v -= L[N * k + i] * s[k];
            s[i] = v / L[(N + 1) * i];
        }
        for (int i = 0; i < N; ++i) Inv[N * i + c] = s[i];
    }
    return true;
}

// csr.hpp source: the factor measurements grouped by camera, perm[] their camera-major order
struct GbaByCamera {
    static constexpr int kKeys = 1;
    const int* mtrack;
    const int* img;
    int* perm;
    __device__ bool keys(long long m, int* k) const {
        if (mtrack[m] < 0) return false;
        k[0] = img[m];
        return true;
    }
    __device__ void put(long long m, const int*, const size_t* slot) const { perm[slot[0]] = (int)m; }
};

// ------------------------------------------------------------------ setup
template <class Mdl>
__global__ void gba_init(GbaArgs<Mdl> a) {
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
        if constexpr (Mdl::kCal > 0) Mdl::init_cam(a, i);
    }
    if (i < (size_t)a.T) {
        a.part[i] = 0;
        a.tl[i] = 0.0;
        a.te[i] = 0.0;
        for (int k = 0; k < 3; ++k) a.PA[3 * i + k] = a.PB[3 * i + k] = a.point_in[3 * i + k];
    }
    if (i < (size_t)a.M) a.mtrack[i] = -1;
}

template <class Mdl>
__global__ void gba_setup_tracks(GbaArgs<Mdl> a) {
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

template <class Mdl>
__global__ void gba_setup_cams(GbaArgs<Mdl> a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    atomicAdd(&a.icnt[I_NMOD], 1);
    atomicMin(&a.icnt[I_C0], c);
}

// ------------------------------------------------------------------ nonlinear error of (X, K, P): per-track partials
// K is the cameras' parameters [C][kCamStride]: the input intrinsics (fixed model) or the calibration variable
template <class Mdl>
__device__ double track_error(const GbaArgs<Mdl>& a, const double* X, const double* K, const double* p, int t, int b,
                              int e) {
    double s = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const int c = a.img[m];
        Pose Xc;
        load_pose(X, c, Xc);
        double pc[3], pr[2], uv[2];
        if (!Mdl::project(Xc, K + Mdl::kCamStride * (size_t)c, p, pc, pr)) continue;
        load_uv(a, m, uv);
        const double dx = pr[0] - uv[0], dy = pr[1] - uv[1];
        const double d = sqrt(dx * dx + dy * dy) * a.isig;
        s += a.robust ? huber_loss(d) : 0.5 * d * d;
    }
    return s;
}

template <class Mdl>
__global__ void gba_eval(GbaArgs<Mdl> a, const double* X, const double* K, const double* P) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    const double* p = P + 3 * (size_t)t;
    double s = track_error(a, X, K, p, t, b, e);
    if (t == a.icnt[I_T0])
        for (int k = 0; k < 3; ++k) {
            const double d = p[k] - a.point_in[3 * (size_t)t + k];
            s += 0.5 * d * d * kPointPriorW;
        }
    a.te[t] = s;
}

// scal[S_NEWERR] = sum te + pose prior(Xerr) (+ calibration priors(Kerr)); with_lin: scal[S_NEWLIN] = 0.5 (sum tl + the
// prior rows of the step)
template <class Mdl>
__global__ __launch_bounds__(kVecBlock) void gba_reduce(GbaArgs<Mdl> a, const double* Xerr, const double* Kerr,
                                                        int with_lin) {
    constexpr int W = Mdl::kCal > 0 ? 4 : 2;  // v[2], v[3]: the calibration priors' error and linear row
    __shared__ double sh[16 * W];
    double v[W];
    for (int k = 0; k < W; ++k) v[k] = 0.0;
    for (int t = threadIdx.x; t < a.T; t += kVecBlock) {
        v[0] += a.te[t];
        v[1] += a.tl[t];
    }
    if constexpr (Mdl::kCal > 0) Mdl::reduce_calib_prior(a, Kerr, with_lin, v);
    block_sum<W>(v, sh);
    if (threadIdx.x == 0) {
        const int c0 = a.icnt[I_C0];
        double xi[6], s = 0.0;
        pose_prior_residual(a, Xerr, c0, xi);
        for (int k = 0; k < 6; ++k) s += xi[k] * xi[k];
        double ne = v[0] + 0.5 * s * a.prior_w;
        if constexpr (Mdl::kCal > 0) ne += 0.5 * v[2] * a.kprior_w;
        a.scal[S_NEWERR] = ne;
        if (with_lin) {
            double nl = v[1];
            const double* dx = vec_pose(a, a.x, c0);
            for (int k = 0; k < 6; ++k) {
                const double d = dx[k] + a.scal[S_XI0 + k];
                nl += d * d * a.prior_w;
            }
            if constexpr (Mdl::kCal > 0) nl += v[3] * a.kprior_w;
            a.scal[S_NEWLIN] = 0.5 * nl;
        }
    }
}

// ------------------------------------------------------------------ linearisation
template <class Mdl>
__global__ void gba_linearize(GbaArgs<Mdl> a, const double* X, const double* K, const double* P) {
    using D = GbaDims<Mdl>;
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.M) return;
    const int t = a.mtrack[m];
    if (t < 0) return;
    const int c = a.img[m];
    Pose Xc;
    load_pose(X, c, Xc);
    const double* Kc = K + Mdl::kCamStride * (size_t)c;
    double* L = a.lin + (size_t)m * D::kLin;
    double pc[3], pr[2], uv[2], Jx[12], Jp[6], Jk[D::kCal > 0 ? 2 * D::kCal : 1];
    if (!Mdl::project(Xc, Kc, P + 3 * (size_t)t, pc, pr)) {
        for (int k = 0; k < D::kLin; ++k) L[k] = 0.0;
        return;
    }
    Mdl::project_jac(Xc, Kc, pc, Jp, Jx, Jk);
    load_uv(a, m, uv);
    const double e0 = (pr[0] - uv[0]) * a.isig, e1 = (pr[1] - uv[1]) * a.isig;
    const double sw = a.robust ? sqrt(huber_weight(sqrt(e0 * e0 + e1 * e1))) : 1.0;
    const double s = sw * a.isig;
    for (int k = 0; k < 12; ++k) L[k] = Jx[k] * s;
    for (int k = 0; k < 2 * D::kCal; ++k) L[D::kJk + k] = Jk[k] * s;
    for (int k = 0; k < 6; ++k) L[D::kJp + k] = Jp[k] * s;
    L[D::kB] = -sw * e0;
    L[D::kB + 1] = -sw * e1;
}

// per track: undamped Hpp (with the first track's prior), the point right-hand side, the track's share of oldLin
template <class Mdl>
__global__ void gba_track_lin(GbaArgs<Mdl> a, const double* P) {
    using D = GbaDims<Mdl>;
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
        const double* L = a.lin + (size_t)m * D::kLin;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double* jp = L + D::kJp + 3 * r;
            const double br = L[D::kB + r];
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

// per camera: H = sum J^T J (+ the pose prior on the first camera), g = sum J^T b (- prior); block c0 also stores the
// prior's residual xi0 = Logmap(X0^-1 X). The refined model adds its calibration prior.
template <class Mdl>
__global__ __launch_bounds__(kCamBlock) void gba_cam_lin(GbaArgs<Mdl> a, const double* X, const double* K) {
    using D = GbaDims<Mdl>;
    constexpr int N = D::N, NS = D::kSym + N;
    __shared__ double sh[16 * NS];
    const int c = blockIdx.x;
    if (!a.modelled[c]) return;
    double v[NS];
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const double* L = a.lin + (size_t)a.perm[i] * D::kLin;
        int n = 0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int s = r; s < N; ++s, ++n)
                v[n] += jn<Mdl>(L, 0, r) * jn<Mdl>(L, 0, s) + jn<Mdl>(L, 1, r) * jn<Mdl>(L, 1, s);
            v[D::kSym + r] += jn<Mdl>(L, 0, r) * L[D::kB] + jn<Mdl>(L, 1, r) * L[D::kB + 1];
        }
    }
    block_sum<NS>(v, sh);
    if (threadIdx.x == 0) {
        double* H = a.H + N * N * (size_t)c;
        double* g = a.g + N * (size_t)c;
        int n = 0;
        for (int r = 0; r < N; ++r)
            for (int s = r; s < N; ++s, ++n) H[N * r + s] = H[N * s + r] = v[n];
        for (int r = 0; r < N; ++r) g[r] = v[D::kSym + r];
        if (c == a.icnt[I_C0]) {
            double xi[6];
            pose_prior_residual(a, X, c, xi);
            for (int k = 0; k < 6; ++k) {
                a.scal[S_XI0 + k] = xi[k];
                H[(N + 1) * k] += a.prior_w;
                g[k] += -xi[k] * a.prior_w;
            }
        }
        if constexpr (Mdl::kCal > 0) Mdl::cam_lin_calib_prior(a, c, K, H, g);
    }
}

// scal[S_OLDLIN] = 0.5 (sum tl + |xi0|^2 / sigma^2 (+ sum |dk|^2 / sigma_k^2)); runs after gba_track_lin and gba_cam_lin
template <class Mdl>
__global__ __launch_bounds__(kVecBlock) void gba_oldlin(GbaArgs<Mdl> a) {
    constexpr int W = Mdl::kCal > 0 ? 2 : 1;  // v[1]: the calibration priors
    __shared__ double sh[16 * W];
    double v[W];
    for (int k = 0; k < W; ++k) v[k] = 0.0;
    for (int t = threadIdx.x; t < a.T; t += kVecBlock) v[0] += a.tl[t];
    if constexpr (Mdl::kCal > 0) Mdl::oldlin_calib_prior(a, v);
    block_sum<W>(v, sh);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += a.scal[S_XI0 + k] * a.scal[S_XI0 + k];
        double ol = v[0] + s * a.prior_w;
        if constexpr (Mdl::kCal > 0) ol += v[1] * a.kprior_w;
        a.scal[S_OLDLIN] = 0.5 * ol;
    }
}

// ------------------------------------------------------------------ one LM trial: damping, preconditioner, rhs
template <class Mdl>
__global__ void gba_track_damp(GbaArgs<Mdl> a, double lambda) {
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

// per camera: the N x N block S = H - sum W Hpp^-1 W^T of the Schur complement, W = J^T Jp, damped and inverted (the
// preconditioner), and the reduced right-hand side b_c = g - sum W Hpp^-1 rp. Shared mode keeps the 6 x 6 pose block and
// hands the calibration rows and columns to the model's border.
template <class Mdl>
__global__ __launch_bounds__(kCamBlock) void gba_cam_build(GbaArgs<Mdl> a, double lambda) {
    using D = GbaDims<Mdl>;
    constexpr int N = D::N, NS = D::kSym + N, kJp = D::kJp;
    __shared__ double sh[16 * NS];
    const int c = blockIdx.x;
    const int nb = is_shared(a) ? 6 : N;
    if (!a.modelled[c]) {
        if (threadIdx.x < N * N) a.Pinv[N * N * (size_t)c + threadIdx.x] = 0.0;
        if (threadIdx.x < nb) a.bvec[(size_t)nb * c + threadIdx.x] = 0.0;
        if constexpr (Mdl::kCal > 0)
            if (a.shared && threadIdx.x < 9) a.bslot[9 * (size_t)c + threadIdx.x] = 0.0;
        return;
    }
    double v[NS];
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const int m = a.perm[i];
        const double* L = a.lin + (size_t)m * D::kLin;
        const size_t t = (size_t)a.mtrack[m];
        const double* Mi = a.Minv + 9 * t;
        const double* rp = a.rp + 3 * t;
        double W[3 * N], WM[3 * N], Mr[3];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) W[3 * r + k] = jn<Mdl>(L, 0, r) * L[kJp + k] + jn<Mdl>(L, 1, r) * L[kJp + 3 + k];
#pragma unroll
        for (int r = 0; r < N; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                WM[3 * r + k] = W[3 * r] * Mi[k] + W[3 * r + 1] * Mi[3 + k] + W[3 * r + 2] * Mi[6 + k];
        mv3(Mi, rp, Mr);
        int n = 0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
            for (int s = r; s < N; ++s, ++n)
                v[n] += WM[3 * r] * W[3 * s] + WM[3 * r + 1] * W[3 * s + 1] + WM[3 * r + 2] * W[3 * s + 2];
            v[D::kSym + r] += W[3 * r] * Mr[0] + W[3 * r + 1] * Mr[1] + W[3 * r + 2] * Mr[2];
        }
    }
    block_sum<NS>(v, sh);
    if (threadIdx.x == 0) {
        const double* H = a.H + N * N * (size_t)c;
        const double* g = a.g + N * (size_t)c;
        double S[N * N], Inv[N * N];
        int n = 0;
        for (int r = 0; r < N; ++r)
            for (int s = r; s < N; ++s, ++n) S[N * r + s] = S[N * s + r] = H[N * r + s] - v[n];
        if constexpr (Mdl::kCal > 0)
            if (a.shared) {
                Mdl::build_border(a, c, lambda, S, g, v, Inv);
                return;
            }
        for (int k = 0; k < N; ++k) S[(N + 1) * k] += lambda;
        if (!spd_inverse<N>(S, Inv)) {
            for (int k = 0; k < N * N; ++k) Inv[k] = 0.0;
            a.icnt[I_BAD] = 1;
        }
        for (int k = 0; k < N * N; ++k) a.Pinv[N * N * (size_t)c + k] = Inv[k];
        for (int r = 0; r < N; ++r) a.bvec[N * (size_t)c + r] = g[r] - v[D::kSym + r];
    }
}

// ------------------------------------------------------------------ PCG
template <class Mdl>
__device__ __forceinline__ double precond_row(const GbaArgs<Mdl>& a, int i) {
    constexpr int N = GbaDims<Mdl>::N;
    if constexpr (Mdl::kCal > 0)
        if (a.shared) return Mdl::precond_row_shared(a, i);
    const int c = i / N, k = i - N * c;
    const double* Pm = a.Pinv + N * N * (size_t)c + N * k;
    const double* rc = a.r + N * (size_t)c;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) s += Pm[j] * rc[j];
    return s;
}

template <class Mdl>
__global__ __launch_bounds__(kVecBlock) void gba_pcg_init(GbaArgs<Mdl> a, double lambda) {
    __shared__ double sh[16 * (Mdl::kCal > 0 ? 9 : 2)];  // the refined model's border sum is 9 wide
    const int n = nvec(a);
    if constexpr (Mdl::kCal > 0)
        if (a.shared) Mdl::border_init(a, lambda, sh);
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

// s = sum_m Jp_m^T (J_m vec_cam(m)): one lane per track, CSR order. vec is p (a product) or the solved step x
// (back-substitution reuses the inner sum). u0 / u1 take the pose columns first, then the calibration columns.
template <class Mdl>
__device__ __forceinline__ void track_wtx(const GbaArgs<Mdl>& a, const double* vec, int t, int b, int e, double* s) {
    using D = GbaDims<Mdl>;
    s[0] = s[1] = s[2] = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const double* L = a.lin + (size_t)m * D::kLin;
        const int c = a.img[m];
        const double* pc = vec_pose(a, vec, c);
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            u0 += L[k] * pc[k];
            u1 += L[6 + k] * pc[k];
        }
        if constexpr (D::kCal > 0) {
            const double* pk = vec_calib(a, vec, c);
#pragma unroll
            for (int k = 0; k < D::kCal; ++k) {
                u0 += L[D::kJk + k] * pk[k];
                u1 += L[D::kJk + D::kCal + k] * pk[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += L[D::kJp + k] * u0 + L[D::kJp + 3 + k] * u1;
    }
}

// y_t = Hpp_t^-1 sum_m Jp_m^T (J_m p_cam(m))
template <class Mdl>
__global__ void gba_prod_tracks(GbaArgs<Mdl> a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    double s[3], y[3];
    track_wtx(a, a.p, t, b, e, s);
    mv3(a.Minv + 9 * (size_t)t, s, y);
    for (int k = 0; k < 3; ++k) a.y[3 * (size_t)t + k] = y[k];
}

// one workgroup per camera over the camera-major index: w = H_c p_c - sum_m J_m^T (Jp_m y_track(m)), q_c = w + lambda p_c.
// Shared mode: q_c = w[0:6] + lambda p_c, and w[6:9] is the camera's share of the border row, written to its slot.
template <class Mdl>
__global__ __launch_bounds__(kCamBlock) void gba_prod_cams(GbaArgs<Mdl> a, double lambda) {
    using D = GbaDims<Mdl>;
    constexpr int N = D::N, kJp = D::kJp;
    __shared__ double sh[16 * N];
    const int c = blockIdx.x;
    const int nb = is_shared(a) ? 6 : N;
    if (!a.modelled[c]) {
        if (threadIdx.x < nb) a.q[(size_t)nb * c + threadIdx.x] = 0.0;
        if constexpr (D::kCal > 0)
            if (a.shared && threadIdx.x < D::kCal) a.pslot[D::kCal * (size_t)c + threadIdx.x] = 0.0;
        return;
    }
    double v[N];
    for (int k = 0; k < N; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const int m = a.perm[i];
        const double* L = a.lin + (size_t)m * D::kLin;
        const double* y = a.y + 3 * (size_t)a.mtrack[m];
        const double u0 = L[kJp] * y[0] + L[kJp + 1] * y[1] + L[kJp + 2] * y[2];
        const double u1 = L[kJp + 3] * y[0] + L[kJp + 4] * y[1] + L[kJp + 5] * y[2];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += jn<Mdl>(L, 0, k) * u0 + jn<Mdl>(L, 1, k) * u1;
    }
    block_sum<N>(v, sh);
    if (threadIdx.x < N) {
        const int k = threadIdx.x;
        const double* H = a.H + N * N * (size_t)c + N * k;
        const double* pc = vec_pose(a, a.p, c);
        double s = 0.0;
        for (int j = 0; j < 6; ++j) s += H[j] * pc[j];
        if constexpr (D::kCal > 0) {
            const double* pk = vec_calib(a, a.p, c);
            for (int j = 0; j < D::kCal; ++j) s += H[6 + j] * pk[j];
            if (k >= nb) {
                a.pslot[D::kCal * (size_t)c + (k - 6)] = s - v[k];
                return;
            }
        }
        s += lambda * pc[k];  // k < nb: entry k of the camera's own block (per camera mode: its calibration follows pc)
        a.q[(size_t)nb * c + k] = s - v[k];
    }
}

template <class Mdl>
__global__ __launch_bounds__(kVecBlock) void gba_pcg_step(GbaArgs<Mdl> a, double lambda) {
    __shared__ double sh[16 * (Mdl::kCal > 0 ? 3 : 2)];  // the refined model's border row is 3 wide
    const int n = nvec(a);
    if constexpr (Mdl::kCal > 0)
        if (a.shared) Mdl::border_q(a, lambda, sh);
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
template <class Mdl>
__global__ void gba_retract(GbaArgs<Mdl> a, const double* X, double* Xn) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    Pose A, B;
    load_pose(X, c, A);
    pose_retract(A, vec_pose(a, a.x, c), B);
    for (int k = 0; k < 9; ++k) Xn[12 * (size_t)c + k] = B.R[k];
    for (int k = 0; k < 3; ++k) Xn[12 * (size_t)c + 9 + k] = B.t[k];
    if constexpr (Mdl::kCal > 0) Mdl::retract_calib(a, c);
}

template <class Mdl>
__global__ void gba_backsub(GbaArgs<Mdl> a, const double* Xn, const double* Kn, const double* P, double* Pn) {
    using D = GbaDims<Mdl>;
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
        const double* L = a.lin + (size_t)m * D::kLin;
        const double* dc = vec_pose(a, a.x, a.img[m]);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double v = -L[D::kB + r];
#pragma unroll
            for (int k = 0; k < 6; ++k) v += L[6 * r + k] * dc[k];
            if constexpr (D::kCal > 0) {
                const double* dk = vec_calib(a, a.x, a.img[m]);
#pragma unroll
                for (int k = 0; k < D::kCal; ++k) v += L[D::kJk + D::kCal * r + k] * dk[k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) v += L[D::kJp + 3 * r + k] * dp[k];
            nl += v * v;
        }
    }
    double ne = track_error(a, Xn, Kn, pn, t, b, e);
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
template <class Mdl>
__global__ void gba_filter(GbaArgs<Mdl> a, const double* X, const double* K, const double* P, double thresh,
                           uint8_t* track_keep, uint8_t* cam_keep) {
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
        if (!Mdl::project(Xc, K + Mdl::kCamStride * (size_t)c, P + 3 * (size_t)t, pc, pr)) { good = false; break; }
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

template <class Mdl>
__global__ void gba_output(GbaArgs<Mdl> a, const double* X, const double* K, const double* P, double* wRc_out,
                           double* wtc_out, double* calib_out, double* point_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)a.C) {
        for (int k = 0; k < 9; ++k) wRc_out[9 * i + k] = X[12 * i + k];
        for (int k = 0; k < 3; ++k) wtc_out[3 * i + k] = X[12 * i + 9 + k];
        if constexpr (Mdl::kCal > 0)
            for (int k = 0; k < Mdl::kCamStride; ++k) calib_out[Mdl::kCamStride * i + k] = K[Mdl::kCamStride * i + k];
    }
    if (i < (size_t)a.T)
        for (int k = 0; k < 3; ++k) point_out[3 * i + k] = P[3 * i + k];
}

// one workgroup, of 64 lanes (fixed model) or kVecBlock (refined: its extra stats are a reduction over the cameras)
template <class Mdl>
__global__ __launch_bounds__(kVecBlock) void gba_stats(GbaArgs<Mdl> a, const double* K, double* stats, double err0,
                                                       double err, double iters, double trials, double pcg_iters,
                                                       double cap_hits, double status) {
    if constexpr (Mdl::kCal > 0) Mdl::extra_stats(a, K, stats);
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
bool gba_sizes_ok(long long n_tracks, long long n_meas, int n_img) {
    return n_tracks > 0 && n_meas > 0 && n_img > 0 && n_tracks < (1ll << 31) - 1 && n_meas < (1ll << 31) - 1 &&
           n_img <= (1 << 20);
}

// hands out the pieces of a workspace at `base`: piece(p, count) points p at count elements of its type
struct GbaCarver {
    uintptr_t base;
    WsCarver w;
    template <class T>
    void piece(T*& p, size_t count) {
        p = (T*)(base + w.take(count * sizeof(T)));
    }
};

// an unknown-sized vector: [C][N], or the shared mode's [6C | kCal], whichever is longer
template <class Mdl>
constexpr size_t gba_vec_len(size_t c) {
    return GbaDims<Mdl>::N * c + Mdl::kCal;
}

// Points a's workspace fields into the workspace at `base` and returns the bytes it needs; base = 0 only sizes it.
template <class Mdl>
size_t gba_carve(GbaArgs<Mdl>& a, uintptr_t base, long long T, long long M, int C) {
    using D = GbaDims<Mdl>;
    a.chunks = csr_chunks(M, kSortChunksMax);
    GbaCarver cv{base};
    const size_t t = (size_t)T, m = (size_t)M, c = (size_t)C, nv = gba_vec_len<Mdl>(c);
    cv.piece(a.part, t);
    cv.piece(a.modelled, c);
    cv.piece(a.mtrack, m);
    cv.piece(a.cam_off, c + 1);
    cv.piece(a.perm, m);
    cv.piece(a.hist, csr_hist_bytes(a.chunks, c) / sizeof(int));
    cv.piece(a.icnt, I_COUNT);
    cv.piece(a.XA, c * 12);
    cv.piece(a.XB, c * 12);
    cv.piece(a.PA, t * 3);
    cv.piece(a.PB, t * 3);
    cv.piece(a.lin, m * D::kLin);
    cv.piece(a.H, c * D::N * D::N);
    cv.piece(a.g, c * D::N);
    cv.piece(a.Pinv, c * D::N * D::N);
    if constexpr (Mdl::kCal > 0) Mdl::carve(a, cv, c);
    cv.piece(a.Hpp, t * 9);
    cv.piece(a.Minv, t * 9);
    cv.piece(a.rp, t * 3);
    cv.piece(a.y, t * 3);
    cv.piece(a.tl, t);
    cv.piece(a.te, t);
    cv.piece(a.bvec, 6 * nv);
    a.x = a.bvec + nv; a.r = a.bvec + 2 * nv; a.z = a.bvec + 3 * nv; a.p = a.bvec + 4 * nv; a.q = a.bvec + 5 * nv;
    cv.piece(a.scal, S_COUNT);
    return cv.w.o;
}

template <class Mdl>
size_t gba_workspace_bytes(long long n_tracks, long long n_meas, int n_img) {
    if (!gba_sizes_ok(n_tracks, n_meas, n_img)) return 0;
    GbaArgs<Mdl> a;
    return gba_carve(a, 0, n_tracks, n_meas, n_img);
}

// ------------------------------------------------------------------ the entry point behind both extern "C" wrappers
// The parameters are the C ABI's (include/gtsfm_hip.h); d_cam is d_intrinsics or d_calib, d_calib_out is null for the
// fixed model, and `extra` carries the model's own checked arguments. Synchronises the stream; allocates nothing.
template <class Mdl>
int gba_run(typename Mdl::Extra extra, const int* d_track_offsets, const int* d_track_img, const void* d_track_uv,
            int uv_is_f64, long long n_tracks, const long long* d_n_tracks, long long n_meas, const double* d_point,
            const uint8_t* d_track_valid, const uint8_t* d_meas_valid, const double* d_wRc, const double* d_wtc,
            const double* d_cam, const uint8_t* d_cam_valid, int n_img, int robust, double measurement_sigma,
            double cam_pose3_prior_sigma, int max_iterations, double pcg_rel_tol, int pcg_max_iter,
            double reproj_error_thresh, void* d_workspace, size_t workspace_bytes, double* d_wRc_out, double* d_wtc_out,
            double* d_calib_out, double* d_point_out, uint8_t* d_track_keep, uint8_t* d_cam_keep, double* d_stats,
            hipStream_t stream) {
    if (n_tracks < 0 || n_meas < 0 || n_img < 0 || n_tracks >= (1ll << 31) - 1 || n_meas >= (1ll << 31) - 1 ||
        n_img > (1 << 20) || !d_wRc_out || !d_wtc_out || (Mdl::kCal > 0 && !d_calib_out) || !d_point_out ||
        !d_track_keep || !d_cam_keep || !d_stats || !(measurement_sigma > 0) || !(cam_pose3_prior_sigma > 0) ||
        max_iterations < 0 || !(pcg_rel_tol > 0) || pcg_max_iter <= 0 || !(reproj_error_thresh > 0) ||
        (uv_is_f64 != 0 && uv_is_f64 != 1))
        return GTSFM_ERR_ARG;
    if ((n_img > 0 && (!d_wRc || !d_wtc || !d_cam)) || (n_tracks > 0 && (!d_track_offsets || !d_point)) ||
        (n_meas > 0 && (!d_track_img || !d_track_uv)))
        return GTSFM_ERR_ARG;
    const int T = (int)n_tracks, M = (int)n_meas, C = n_img;
    double nothing[Mdl::kStats] = {};
    nothing[9] = 1;
    // the reference's early return (bundle_adjustment.py:319-324): inputs copied through, keep all zero, error 0
    auto copy_through = [&]() -> int {
        if (C > 0) {
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_wRc_out, d_wRc, (size_t)C * 9 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_wtc_out, d_wtc, (size_t)C * 3 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            if constexpr (Mdl::kCal > 0)
                GTSFM_CHECK_HIP(hipMemcpyAsync(d_calib_out, d_cam, (size_t)C * Mdl::kCamStride * sizeof(double),
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
    GbaArgs<Mdl> a;
    static_cast<typename Mdl::Extra&>(a) = extra;
    if (workspace_bytes < gba_carve(a, (uintptr_t)d_workspace, T, M, C)) return GTSFM_ERR_CAPACITY;
    a.off = d_track_offsets; a.img = d_track_img; a.uv = d_track_uv; a.uv64 = uv_is_f64; a.d_nt = d_n_tracks;
    a.T = T; a.M = M; a.C = C;
    a.point_in = d_point; a.tvalid = d_track_valid; a.mvalid = d_meas_valid;
    a.wRc = d_wRc; a.wtc = d_wtc; a.cam = d_cam; a.cvalid = d_cam_valid;
    a.robust = robust != 0;
    a.isig = 1.0 / measurement_sigma;
    a.prior_w = 1.0 / (cam_pose3_prior_sigma * cam_pose3_prior_sigma);

    const unsigned B = 256;
    const unsigned gT = blocks_for(T, B), gM = blocks_for(M, B), gC = blocks_for(C, B);
    const size_t nmax = (size_t)(T > M ? T : M) > (size_t)C ? (size_t)(T > M ? T : M) : (size_t)C;
    int icnt[I_COUNT];
    double scal[6];
    auto read_icnt = [&]() { return read_back(icnt, a.icnt, I_COUNT, stream); };
    auto read_scal = [&]() { return read_back(scal, a.scal, 6, stream); };

    hipLaunchKernelGGL(gba_init<Mdl>, dim3(blocks_for(nmax, B)), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(gba_setup_tracks<Mdl>, dim3(gT), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(gba_setup_cams<Mdl>, dim3(gC), dim3(B), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    int rc = read_icnt();
    if (rc != GTSFM_OK) return rc;
    if (icnt[I_NPART] == 0 || icnt[I_NMOD] == 0) return copy_through();
    if constexpr (Mdl::kCal > 0) Mdl::start_calib(a, gC, B, stream);

    if ((rc = csr_build(GbaByCamera{a.mtrack, a.img, a.perm}, M, C, a.chunks, a.hist, a.cam_off, stream)) != GTSFM_OK)
        return rc;

    // The variables are double-buffered: a trial writes (Xn, Kn, Pn) and an accepted one swaps. The refined model's
    // calibration is swapped inside `a`, so that a.KA is the current one and a.KB the trial's; the fixed model's K and Kn
    // are both the input intrinsics, read only.
    double* X = a.XA;
    double* Xn = a.XB;
    double* P = a.PA;
    double* Pn = a.PB;
    const double* K = a.cam;
    const double* Kn = a.cam;
    if constexpr (Mdl::kCal > 0) {
        K = a.KA;
        Kn = a.KB;
    }
    hipLaunchKernelGGL(gba_eval<Mdl>, dim3(gT), dim3(B), 0, stream, a, X, K, P);
    hipLaunchKernelGGL(gba_reduce<Mdl>, dim3(1), dim3(kVecBlock), 0, stream, a, X, K, 0);
    GTSFM_CHECK_HIP(hipGetLastError());
    if ((rc = read_scal()) != GTSFM_OK) return rc;
    const double err0 = scal[S_NEWERR];
    double err = err0, lambda = 1e-5;
    const int max_iters = max_iterations > 0 ? max_iterations : 100;
    long long iters = 0, trials = 0, pcg_total = 0, cap_hits = 0;
    if (err > 0.0) {
        for (;;) {  // ends: every outer step either accepts (iters <= max_iters) or leaves err unchanged (dec = 0)
            const double cur = err;
            hipLaunchKernelGGL(gba_linearize<Mdl>, dim3(gM), dim3(B), 0, stream, a, X, K, P);
            hipLaunchKernelGGL(gba_track_lin<Mdl>, dim3(gT), dim3(B), 0, stream, a, P);
            hipLaunchKernelGGL(gba_cam_lin<Mdl>, dim3(C), dim3(kCamBlock), 0, stream, a, X, K);
            hipLaunchKernelGGL(gba_oldlin<Mdl>, dim3(1), dim3(kVecBlock), 0, stream, a);
            double oldLin = 0.0;
            bool have_oldlin = false;
            for (int inner = 0; inner < kInnerMax; ++inner) {
                ++trials;
                GTSFM_CHECK_HIP(hipMemsetAsync(a.icnt + I_BAD, 0, sizeof(int), stream));
                hipLaunchKernelGGL(gba_track_damp<Mdl>, dim3(gT), dim3(B), 0, stream, a, lambda);
                hipLaunchKernelGGL(gba_cam_build<Mdl>, dim3(C), dim3(kCamBlock), 0, stream, a, lambda);
                hipLaunchKernelGGL(gba_pcg_init<Mdl>, dim3(1), dim3(kVecBlock), 0, stream, a, lambda);
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
                        hipLaunchKernelGGL(gba_prod_tracks<Mdl>, dim3(gT), dim3(B), 0, stream, a);
                        hipLaunchKernelGGL(gba_prod_cams<Mdl>, dim3(C), dim3(kCamBlock), 0, stream, a, lambda);
                        hipLaunchKernelGGL(gba_pcg_step<Mdl>, dim3(1), dim3(kVecBlock), 0, stream, a, lambda);
                        GTSFM_CHECK_HIP(hipGetLastError());
                        const int rc2 = read_scal();
                        rr = scal[S_RR];
                        return rc2;
                    });
                    if (rc != GTSFM_OK) return rc;
                    hipLaunchKernelGGL(gba_retract<Mdl>, dim3(gC), dim3(B), 0, stream, a, X, Xn);
                    hipLaunchKernelGGL(gba_backsub<Mdl>, dim3(gT), dim3(B), 0, stream, a, Xn, Kn, P, Pn);
                    hipLaunchKernelGGL(gba_reduce<Mdl>, dim3(1), dim3(kVecBlock), 0, stream, a, Xn, Kn, 1);
                    GTSFM_CHECK_HIP(hipGetLastError());
                    if ((rc = read_scal()) != GTSFM_OK) return rc;
                    trial = lm_judge(err, oldLin, scal[S_NEWLIN], scal[S_NEWERR]);
                }
                if (trial.success) {
                    double* s = X; X = Xn; Xn = s;
                    s = P; P = Pn; Pn = s;
                    if constexpr (Mdl::kCal > 0) {
                        s = a.KA; a.KA = a.KB; a.KB = s;
                        K = a.KA;
                        Kn = a.KB;
                    }
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
    hipLaunchKernelGGL(gba_filter<Mdl>, dim3(gT), dim3(B), 0, stream, a, X, K, P, reproj_error_thresh, d_track_keep,
                       d_cam_keep);
    hipLaunchKernelGGL(gba_output<Mdl>, dim3(blocks_for(T > C ? T : C, B)), dim3(B), 0, stream, a, X, K, P, d_wRc_out,
                       d_wtc_out, d_calib_out, d_point_out);
    hipLaunchKernelGGL(gba_stats<Mdl>, dim3(1), dim3(Mdl::kCal > 0 ? kVecBlock : 64), 0, stream, a, K, d_stats, err0,
                       err, (double)iters, (double)trials, (double)pcg_total, (double)cap_hits, 0.0);
    GTSFM_CHECK_HIP(hipGetLastError());
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    return GTSFM_OK;
}

}  // namespace
