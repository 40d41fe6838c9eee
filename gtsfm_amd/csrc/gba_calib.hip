// Self-calibrating global bundle adjustment: gba.hip's Levenberg-Marquardt over every camera pose and every landmark,
// with the Cal3Bundler calibration (f, k1, k2) of the cameras as variables too, one per modelled camera or one shared.
//
// Reference: gtsfm/bundle/bundle_adjustment.py:58-66 ("refines global pose estimates and intrinsics of cameras"),
// :103-131 and :180-208 (a K(i) per camera, or a single K(0) with shared_calib, in every GeneralSFMFactor2Cal3Bundler,
// and a PriorFactorCal3Bundler of calibration_prior_noise_sigma on each), :188-195 and :258-260 (the shared variable is
// the first camera's calibration, principal point included), on GTSAM 4.2's Cal3Bundler: u = f g x + u0 with
// g = 1 + (k1 + k2 r2) r2, three degrees of freedom (f, k1, k2), additive retraction. Everything else (participation,
// the pose and point priors, Huber, the cheirality treatment, the LM schedule, point elimination, PCG from a zero start,
// block-Jacobi preconditioning, fixed summation orders) is gba.hip's; gba_shared.hpp holds the common device code.
//
// A measurement's record is Jx 2 x 6, Jk 2 x 3, Jp 2 x 3, b 2: 208 bytes (gba.hip: 160). With J9 = [Jx | Jk], every
// per-camera sum is gba.hip's with 9 in place of 6: H9_c = sum J9^T J9, the 9 x 9 block of the damped Schur complement
// and the 9-vector sum J9^T (Jp y) of a product. The two modes differ only in where the last three entries go:
//   per camera  the unknown is [C][9]; camera c's block is its own 9 x 9, inverted for the preconditioner;
//   shared      the unknown is [6C poses | 3]. A camera workgroup keeps the pose part (6 x 6 block, 6 entries of q) and
//               writes its contribution to the 3-wide border (the 3 x 3 diagonal block and right-hand side at build time,
//               the border row of q = S p in a product) into a slot of its own; the single-workgroup kernel that follows
//               (gbc_pcg_init, gbc_pcg_step) sums the slots in a fixed order (reduce.hpp), adds the prior and the
//               damping and, at build time, inverts the border block for the preconditioner.
// No floating-point atomics: two calls return the same bytes. LM / PCG control flow is host code (lm.hpp), so the entry
// point synchronises its stream; it allocates nothing.
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

constexpr int kLin = 26;        // doubles per measurement: Jx[12], Jk[6], Jp[6], b[2]
constexpr int kJk = 12, kJp = 18, kB = 24;
constexpr int kCamBlock = 256;  // lanes of a camera-grouped workgroup
constexpr int kVecBlock = 1024; // lanes of the single-workgroup vector kernels
constexpr int kSortChunksMax = 1024;
constexpr int kSym9 = 45;       // upper triangle of a 9 x 9

// scal[] slots (doubles, device)
enum { S_RR = 0, S_RZ = 1, S_BB = 2, S_OLDLIN = 3, S_NEWLIN = 4, S_NEWERR = 5, S_XI0 = 8, S_COUNT = 16 };
// icnt[] slots (ints, device)
enum { I_NPART = 0, I_NMOD = 1, I_T0 = 2, I_C0 = 3, I_NFAC = 4, I_NKEPT = 5, I_BAD = 6, I_COUNT = 8 };

struct GbcArgs {
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
    const double* calib;  // [C][5] = (f, k1, k2, u0, v0)
    const uint8_t* cvalid;
    int robust;
    int shared;
    double isig;      // 1 / measurement_sigma
    double prior_w;   // 1 / cam_pose3_prior_sigma^2
    double kprior_w;  // 1 / calibration_prior_sigma^2
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
    double* KA;         // [C][5]
    double* KB;
    double* PA;         // [T][3]
    double* PB;
    double* lin;        // [M][kLin]
    double* H9;         // [C][81]
    double* g9;         // [C][9]
    double* Pinv;       // [C][81]; shared: the 6 x 6 in the first 36
    double* PinvK;      // [9] shared: the border block's inverse
    double* dk;         // [C][3] calibration minus its prior at the linearisation point (shared: row c0 only)
    double* bslot;      // [C][9] shared, build: the camera's share of the border block (6) and right-hand side (3)
    double* pslot;      // [C][3] shared, product: the camera's share of the border row of q
    double* Hpp;        // [T][9] undamped
    double* Minv;       // [T][9]
    double* rp;         // [T][3]
    double* y;          // [T][3]
    double* tl;         // [T]
    double* te;         // [T]
    double* bvec;       // [nvec] each
    double* x;
    double* r;
    double* z;
    double* p;
    double* q;
    double* scal;       // [S_COUNT]
    CsrChunks chunks;   // of the sort by camera
};

__device__ __forceinline__ int nvec(const GbcArgs& a) { return a.shared ? 6 * a.C + 3 : 9 * a.C; }
// the pose and the calibration entries of camera c in an unknown-sized vector
__device__ __forceinline__ const double* vec_pose(const GbcArgs& a, const double* v, int c) {
    return v + (size_t)(a.shared ? 6 : 9) * c;
}
__device__ __forceinline__ const double* vec_calib(const GbcArgs& a, const double* v, int c) {
    return a.shared ? v + 6 * (size_t)a.C : v + 9 * (size_t)c + 6;
}
// the calibration the prior of camera c's variable sits at
__device__ __forceinline__ const double* calib_prior(const GbcArgs& a, int c) {
    return a.calib + 5 * (size_t)(a.shared ? a.icnt[I_C0] : c);
}

__device__ __forceinline__ int n_tracks_eff(const GbcArgs& a) {
    if (!a.d_nt) return a.T;
    const long long n = a.d_nt[0];
    return n < 0 ? 0 : (n < (long long)a.T ? (int)n : a.T);
}

__device__ __forceinline__ void load_uv(const GbcArgs& a, int m, double* uv) {
    if (a.uv64) {
        uv[0] = ((const double*)a.uv)[2 * (size_t)m];
        uv[1] = ((const double*)a.uv)[2 * (size_t)m + 1];
    } else {
        uv[0] = ((const float*)a.uv)[2 * (size_t)m];
        uv[1] = ((const float*)a.uv)[2 * (size_t)m + 1];
    }
}

__device__ __forceinline__ bool meas_flag(const GbcArgs& a, int m) { return !a.mvalid || a.mvalid[m] != 0; }
__device__ __forceinline__ bool cam_ok(const GbcArgs& a, int c) {
    return c >= 0 && c < a.C && (!a.cvalid || a.cvalid[c] != 0);
}
__device__ __forceinline__ bool track_range(const GbcArgs& a, int t, int& b, int& e) {
    b = a.off[t];
    e = a.off[t + 1];
    return b >= 0 && e >= b && e <= a.M;
}
__device__ __forceinline__ void load_pose(const double* X, int c, Pose& P) {
    const double* s = X + 12 * (size_t)c;
    for (int k = 0; k < 9; ++k) P.R[k] = s[k];
    for (int k = 0; k < 3; ++k) P.t[k] = s[9 + k];
}

// Cal3Bundler projection, K = (f, k1, k2, u0, v0); pc is the point in the camera frame; false when z <= 0
__device__ __forceinline__ bool project_k(const Pose& X, const double* K, const double* p, double* pc, double* uv) {
    const double d[3] = {p[0] - X.t[0], p[1] - X.t[1], p[2] - X.t[2]};
    mtv3(X.R, d, pc);
    if (pc[2] <= 0.0) return false;
    const double x = pc[0] / pc[2], y = pc[1] / pc[2];
    const double r2 = x * x + y * y;
    const double g = 1.0 + (K[1] + K[2] * r2) * r2;
    uv[0] = K[0] * g * x + K[3];
    uv[1] = K[0] * g * y + K[4];
    return true;
}

// d uv / d p (Jp, 2 x 3), d uv / d pose (Jx, 2 x 6, body frame, rotation first) and d uv / d (f, k1, k2) (Jk, 2 x 3)
__device__ __forceinline__ void project_k_jac(const Pose& X, const double* K, const double* pc, double* Jp, double* Jx,
                                              double* Jk) {
    const double iz = 1.0 / pc[2], x = pc[0] * iz, y = pc[1] * iz, f = K[0];
    const double r2 = x * x + y * y;
    const double g = 1.0 + (K[1] + K[2] * r2) * r2;
    const double h = 2.0 * (K[1] + 2.0 * K[2] * r2);
    // d uv / d (x, y) = f (g I + h [x; y][x y])
    const double A00 = f * (g + h * x * x), A01 = f * (h * x * y), A11 = f * (g + h * y * y);
    // times d (x, y) / d pc = [[iz, 0, -x iz], [0, iz, -y iz]]
    const double D[6] = {A00 * iz, A01 * iz, -(A00 * x + A01 * y) * iz, A01 * iz, A11 * iz, -(A01 * x + A11 * y) * iz};
#pragma unroll
    for (int r = 0; r < 2; ++r) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Jp[3 * r + j] = D[3 * r] * X.R[3 * j] + D[3 * r + 1] * X.R[3 * j + 1] + D[3 * r + 2] * X.R[3 * j + 2];
        const double* d = D + 3 * r;
        Jx[6 * r + 0] = d[1] * pc[2] - d[2] * pc[1];
        Jx[6 * r + 1] = -d[0] * pc[2] + d[2] * pc[0];
        Jx[6 * r + 2] = d[0] * pc[1] - d[1] * pc[0];
        Jx[6 * r + 3] = -d[0];
        Jx[6 * r + 4] = -d[1];
        Jx[6 * r + 5] = -d[2];
    }
    Jk[0] = x * g; Jk[1] = f * x * r2; Jk[2] = f * x * r2 * r2;
    Jk[3] = y * g; Jk[4] = f * y * r2; Jk[5] = f * y * r2 * r2;
}

// entry a of row r of J9 = [Jx | Jk] in a measurement's record
__device__ __forceinline__ double j9(const double* L, int r, int a) {
    return a < 6 ? L[6 * r + a] : L[kJk + 3 * r + (a - 6)];
}

// ------------------------------------------------------------------ setup
__global__ void gbc_init(GbcArgs a) {
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
        for (int k = 0; k < 5; ++k) a.KA[5 * i + k] = a.KB[5 * i + k] = a.calib[5 * i + k];
        for (int k = 0; k < 3; ++k) a.dk[3 * i + k] = 0.0;
    }
    if (i < (size_t)a.T) {
        a.part[i] = 0;
        a.tl[i] = 0.0;
        a.te[i] = 0.0;
        for (int k = 0; k < 3; ++k) a.PA[3 * i + k] = a.PB[3 * i + k] = a.point_in[3 * i + k];
    }
    if (i < (size_t)a.M) a.mtrack[i] = -1;
}

__global__ void gbc_setup_tracks(GbcArgs a) {
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

__global__ void gbc_setup_cams(GbcArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    atomicAdd(&a.icnt[I_NMOD], 1);
    atomicMin(&a.icnt[I_C0], c);
}

// shared mode: every modelled camera starts from the calibration of the modelled camera of lowest index, principal
// point included (bundle_adjustment.py:188-195, :258-260)
__global__ void gbc_share_calib(GbcArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    const double* k0 = a.calib + 5 * (size_t)a.icnt[I_C0];
    for (int k = 0; k < 5; ++k) a.KA[5 * (size_t)c + k] = a.KB[5 * (size_t)c + k] = k0[k];
}

// ------------------------------------------------------------------ nonlinear error of (X, K, P): per-track partials
__device__ double track_error(const GbcArgs& a, const double* X, const double* K, const double* p, int t, int b,
                              int e) {
    double s = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const int c = a.img[m];
        Pose Xc;
        load_pose(X, c, Xc);
        double pc[3], pr[2], uv[2];
        if (!project_k(Xc, K + 5 * (size_t)c, p, pc, pr)) continue;
        load_uv(a, m, uv);
        const double dx = pr[0] - uv[0], dy = pr[1] - uv[1];
        const double d = sqrt(dx * dx + dy * dy) * a.isig;
        s += a.robust ? huber_loss(d) : 0.5 * d * d;
    }
    return s;
}

__global__ void gbc_eval(GbcArgs a, const double* X, const double* K, const double* P) {
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

// scal[S_NEWERR] = sum te + pose prior(Xerr) + calibration priors(Kerr); with_lin: scal[S_NEWLIN] = 0.5 (sum tl + the
// prior rows of the step)
__global__ __launch_bounds__(kVecBlock) void gbc_reduce(GbcArgs a, const double* Xerr, const double* Kerr,
                                                        int with_lin) {
    __shared__ double sh[16 * 4];
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < a.T; t += kVecBlock) {
        v[0] += a.te[t];
        v[1] += a.tl[t];
    }
    const int c0 = a.icnt[I_C0];
    for (int c = threadIdx.x; c < a.C; c += kVecBlock) {
        if (!a.modelled[c] || (a.shared && c != c0)) continue;
        const double* k0 = calib_prior(a, c);
        const double* dx = vec_calib(a, a.x, c);
        for (int k = 0; k < 3; ++k) {
            const double d = Kerr[5 * (size_t)c + k] - k0[k];
            v[2] += d * d;
            if (with_lin) {
                const double l = dx[k] + a.dk[3 * (size_t)c + k];
                v[3] += l * l;
            }
        }
    }
    block_sum<4>(v, sh);
    if (threadIdx.x == 0) {
        Pose A, B;
        for (int k = 0; k < 9; ++k) A.R[k] = a.wRc[9 * (size_t)c0 + k];
        for (int k = 0; k < 3; ++k) A.t[k] = a.wtc[3 * (size_t)c0 + k];
        load_pose(Xerr, c0, B);
        double xi[6], s = 0.0;
        pose_local(A, B, xi);
        for (int k = 0; k < 6; ++k) s += xi[k] * xi[k];
        a.scal[S_NEWERR] = v[0] + 0.5 * s * a.prior_w + 0.5 * v[2] * a.kprior_w;
        if (with_lin) {
            double nl = v[1];
            const double* dx = vec_pose(a, a.x, c0);
            for (int k = 0; k < 6; ++k) {
                const double d = dx[k] + a.scal[S_XI0 + k];
                nl += d * d * a.prior_w;
            }
            nl += v[3] * a.kprior_w;
            a.scal[S_NEWLIN] = 0.5 * nl;
        }
    }
}

// ------------------------------------------------------------------ linearisation
__global__ void gbc_linearize(GbcArgs a, const double* X, const double* K, const double* P) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= a.M) return;
    const int t = a.mtrack[m];
    if (t < 0) return;
    const int c = a.img[m];
    Pose Xc;
    load_pose(X, c, Xc);
    const double* Kc = K + 5 * (size_t)c;
    double* L = a.lin + (size_t)m * kLin;
    double pc[3], pr[2], uv[2], Jx[12], Jp[6], Jk[6];
    if (!project_k(Xc, Kc, P + 3 * (size_t)t, pc, pr)) {
        for (int k = 0; k < kLin; ++k) L[k] = 0.0;
        return;
    }
    project_k_jac(Xc, Kc, pc, Jp, Jx, Jk);
    load_uv(a, m, uv);
    const double e0 = (pr[0] - uv[0]) * a.isig, e1 = (pr[1] - uv[1]) * a.isig;
    const double sw = a.robust ? sqrt(huber_weight(sqrt(e0 * e0 + e1 * e1))) : 1.0;
    const double s = sw * a.isig;
    for (int k = 0; k < 12; ++k) L[k] = Jx[k] * s;
    for (int k = 0; k < 6; ++k) L[kJk + k] = Jk[k] * s;
    for (int k = 0; k < 6; ++k) L[kJp + k] = Jp[k] * s;
    L[kB] = -sw * e0;
    L[kB + 1] = -sw * e1;
}

// per track: undamped Hpp (with the first track's prior), the point right-hand side, the track's share of oldLin
__global__ void gbc_track_lin(GbcArgs a, const double* P) {
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
            const double* jp = L + kJp + 3 * r;
            const double br = L[kB + r];
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

// per camera: H9 = sum J9^T J9 and g9 = sum J9^T b, with the pose prior on the first camera and, per-camera mode, the
// calibration prior of this camera's variable (the shared variable's prior joins the border in gbc_pcg_init); stores
// the priors' residuals xi0 = Logmap(X0^-1 X) and dk = K - K0
__global__ __launch_bounds__(kCamBlock) void gbc_cam_lin(GbcArgs a, const double* X, const double* K) {
    __shared__ double sh[16 * 54];
    const int c = blockIdx.x;
    if (!a.modelled[c]) return;
    double v[54];
    for (int k = 0; k < 54; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const double* L = a.lin + (size_t)a.perm[i] * kLin;
        int n = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
#pragma unroll
            for (int s = r; s < 9; ++s, ++n) v[n] += j9(L, 0, r) * j9(L, 0, s) + j9(L, 1, r) * j9(L, 1, s);
            v[kSym9 + r] += j9(L, 0, r) * L[kB] + j9(L, 1, r) * L[kB + 1];
        }
    }
    block_sum<54>(v, sh);
    if (threadIdx.x == 0) {
        double* H = a.H9 + 81 * (size_t)c;
        double* g = a.g9 + 9 * (size_t)c;
        int n = 0;
        for (int r = 0; r < 9; ++r)
            for (int s = r; s < 9; ++s, ++n) H[9 * r + s] = H[9 * s + r] = v[n];
        for (int r = 0; r < 9; ++r) g[r] = v[kSym9 + r];
        const int c0 = a.icnt[I_C0];
        if (c == c0) {
            Pose A, B;
            for (int k = 0; k < 9; ++k) A.R[k] = a.wRc[9 * (size_t)c + k];
            for (int k = 0; k < 3; ++k) A.t[k] = a.wtc[3 * (size_t)c + k];
            load_pose(X, c, B);
            double xi[6];
            pose_local(A, B, xi);
            for (int k = 0; k < 6; ++k) {
                a.scal[S_XI0 + k] = xi[k];
                H[10 * k] += a.prior_w;
                g[k] += -xi[k] * a.prior_w;
            }
        }
        if (!a.shared || c == c0) {
            const double* k0 = calib_prior(a, c);
            for (int k = 0; k < 3; ++k) {
                const double d = K[5 * (size_t)c + k] - k0[k];
                a.dk[3 * (size_t)c + k] = d;
                if (!a.shared) {
                    H[10 * (6 + k)] += a.kprior_w;
                    g[6 + k] += -d * a.kprior_w;
                }
            }
        }
    }
}

// scal[S_OLDLIN] = 0.5 (sum tl + |xi0|^2 / sigma^2 + sum |dk|^2 / sigma_k^2); runs after gbc_track_lin and gbc_cam_lin
__global__ __launch_bounds__(kVecBlock) void gbc_oldlin(GbcArgs a) {
    __shared__ double sh[16 * 2];
    double v[2] = {0.0, 0.0};
    for (int t = threadIdx.x; t < a.T; t += kVecBlock) v[0] += a.tl[t];
    const int c0 = a.icnt[I_C0];
    for (int c = threadIdx.x; c < a.C; c += kVecBlock) {
        if (!a.modelled[c] || (a.shared && c != c0)) continue;
        for (int k = 0; k < 3; ++k) v[1] += a.dk[3 * (size_t)c + k] * a.dk[3 * (size_t)c + k];
    }
    block_sum<2>(v, sh);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += a.scal[S_XI0 + k] * a.scal[S_XI0 + k];
        a.scal[S_OLDLIN] = 0.5 * (v[0] + s * a.prior_w + v[1] * a.kprior_w);
    }
}

// ------------------------------------------------------------------ one LM trial: damping, preconditioner, rhs
__global__ void gbc_track_damp(GbcArgs a, double lambda) {
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

// per camera: the 9 x 9 block S9 = H9 - sum W Hpp^-1 W^T of the Schur complement, W = J9^T Jp, and the 9 entries
// g9 - sum W Hpp^-1 rp of the reduced right-hand side. Per camera mode: the damped block inverted is the preconditioner.
// Shared mode: the damped 6 x 6 pose block inverted, and the calibration rows and columns go to the camera's border slot.
__global__ __launch_bounds__(kCamBlock) void gbc_cam_build(GbcArgs a, double lambda) {
    __shared__ double sh[16 * 54];
    const int c = blockIdx.x;
    const int nb = a.shared ? 6 : 9;
    if (!a.modelled[c]) {
        if (threadIdx.x < 81) a.Pinv[81 * (size_t)c + threadIdx.x] = 0.0;
        if (threadIdx.x < nb) a.bvec[(size_t)nb * c + threadIdx.x] = 0.0;
        if (a.shared && threadIdx.x < 9) a.bslot[9 * (size_t)c + threadIdx.x] = 0.0;
        return;
    }
    double v[54];
    for (int k = 0; k < 54; ++k) v[k] = 0.0;
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const int m = a.perm[i];
        const double* L = a.lin + (size_t)m * kLin;
        const size_t t = (size_t)a.mtrack[m];
        const double* Mi = a.Minv + 9 * t;
        const double* rp = a.rp + 3 * t;
        double W[27], WM[27], Mr[3];
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) W[3 * r + k] = j9(L, 0, r) * L[kJp + k] + j9(L, 1, r) * L[kJp + 3 + k];
#pragma unroll
        for (int r = 0; r < 9; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                WM[3 * r + k] = W[3 * r] * Mi[k] + W[3 * r + 1] * Mi[3 + k] + W[3 * r + 2] * Mi[6 + k];
        mv3(Mi, rp, Mr);
        int n = 0;
#pragma unroll
        for (int r = 0; r < 9; ++r) {
#pragma unroll
            for (int s = r; s < 9; ++s, ++n)
                v[n] += WM[3 * r] * W[3 * s] + WM[3 * r + 1] * W[3 * s + 1] + WM[3 * r + 2] * W[3 * s + 2];
            v[kSym9 + r] += W[3 * r] * Mr[0] + W[3 * r + 1] * Mr[1] + W[3 * r + 2] * Mr[2];
        }
    }
    block_sum<54>(v, sh);
    if (threadIdx.x == 0) {
        const double* H = a.H9 + 81 * (size_t)c;
        const double* g = a.g9 + 9 * (size_t)c;
        double S[81], Inv[81];
        int n = 0;
        for (int r = 0; r < 9; ++r)
            for (int s = r; s < 9; ++s, ++n) S[9 * r + s] = S[9 * s + r] = H[9 * r + s] - v[n];
        double* Pm = a.Pinv + 81 * (size_t)c;
        if (!a.shared) {
            for (int k = 0; k < 9; ++k) S[10 * k] += lambda;
            if (!spd_inverse<9>(S, Inv)) {
                for (int k = 0; k < 81; ++k) Inv[k] = 0.0;
                a.icnt[I_BAD] = 1;
            }
            for (int k = 0; k < 81; ++k) Pm[k] = Inv[k];
            for (int r = 0; r < 9; ++r) a.bvec[9 * (size_t)c + r] = g[r] - v[kSym9 + r];
        } else {
            double S6[36];
            for (int r = 0; r < 6; ++r)
                for (int s = 0; s < 6; ++s) S6[6 * r + s] = S[9 * r + s];
            for (int k = 0; k < 6; ++k) S6[7 * k] += lambda;
            if (!spd_inverse<6>(S6, Inv)) {
                for (int k = 0; k < 36; ++k) Inv[k] = 0.0;
                a.icnt[I_BAD] = 1;
            }
            for (int k = 0; k < 36; ++k) Pm[k] = Inv[k];
            for (int k = 36; k < 81; ++k) Pm[k] = 0.0;
            for (int r = 0; r < 6; ++r) a.bvec[6 * (size_t)c + r] = g[r] - v[kSym9 + r];
            double* bs = a.bslot + 9 * (size_t)c;
            n = 0;
            for (int r = 6; r < 9; ++r)
                for (int s = r; s < 9; ++s, ++n) bs[n] = S[9 * r + s];
            for (int r = 0; r < 3; ++r) bs[6 + r] = g[6 + r] - v[kSym9 + 6 + r];
        }
    }
}

// ------------------------------------------------------------------ PCG
__device__ __forceinline__ double precond_row(const GbcArgs& a, int i) {
    double s = 0.0;
    if (!a.shared) {
        const int c = i / 9, k = i - 9 * c;
        const double* Pm = a.Pinv + 81 * (size_t)c + 9 * k;
        const double* rc = a.r + 9 * (size_t)c;
#pragma unroll
        for (int j = 0; j < 9; ++j) s += Pm[j] * rc[j];
    } else if (i < 6 * a.C) {
        const int c = i / 6, k = i - 6 * c;
        const double* Pm = a.Pinv + 81 * (size_t)c + 6 * k;
        const double* rc = a.r + 6 * (size_t)c;
#pragma unroll
        for (int j = 0; j < 6; ++j) s += Pm[j] * rc[j];
    } else {
        const double* Pm = a.PinvK + 3 * (i - 6 * a.C);
        const double* rc = a.r + 6 * (size_t)a.C;
#pragma unroll
        for (int j = 0; j < 3; ++j) s += Pm[j] * rc[j];
    }
    return s;
}

__global__ __launch_bounds__(kVecBlock) void gbc_pcg_init(GbcArgs a, double lambda) {
    __shared__ double sh[16 * 9];
    const int n = nvec(a);
    if (a.shared) {
        // the border: its 3 x 3 block of the damped Schur complement, inverted, and its right-hand side
        double w[9];
        for (int k = 0; k < 9; ++k) w[k] = 0.0;
        for (int c = threadIdx.x; c < a.C; c += kVecBlock)
            for (int k = 0; k < 9; ++k) w[k] += a.bslot[9 * (size_t)c + k];
        block_sum<9>(w, sh);
        if (threadIdx.x == 0) {
            const int c0 = a.icnt[I_C0];
            double S[9], Inv[9];
            int m = 0;
            for (int r = 0; r < 3; ++r)
                for (int s = r; s < 3; ++s, ++m) S[3 * r + s] = S[3 * s + r] = w[m];
            for (int k = 0; k < 3; ++k) S[4 * k] += a.kprior_w + lambda;
            if (!spd_inverse<3>(S, Inv)) {
                for (int k = 0; k < 9; ++k) Inv[k] = 0.0;
                a.icnt[I_BAD] = 1;
            }
            for (int k = 0; k < 9; ++k) a.PinvK[k] = Inv[k];
            for (int k = 0; k < 3; ++k)
                a.bvec[6 * (size_t)a.C + k] = w[6 + k] + -a.dk[3 * (size_t)c0 + k] * a.kprior_w;
        }
        __syncthreads();
    }
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

// s = sum_m Jp_m^T (J9_m vec_cam(m)): one lane per track, CSR order. vec is p (a product) or the solved step x
// (back-substitution reuses the inner sum).
__device__ __forceinline__ void track_wtx(const GbcArgs& a, const double* vec, int t, int b, int e, double* s) {
    s[0] = s[1] = s[2] = 0.0;
    for (int m = b; m < e; ++m) {
        if (a.mtrack[m] != t) continue;
        const double* L = a.lin + (size_t)m * kLin;
        const int c = a.img[m];
        const double* pc = vec_pose(a, vec, c);
        const double* pk = vec_calib(a, vec, c);
        double u0 = 0.0, u1 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            u0 += L[k] * pc[k];
            u1 += L[6 + k] * pc[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            u0 += L[kJk + k] * pk[k];
            u1 += L[kJk + 3 + k] * pk[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += L[kJp + k] * u0 + L[kJp + 3 + k] * u1;
    }
}

__global__ void gbc_prod_tracks(GbcArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.T || !a.part[t]) return;
    int b, e;
    track_range(a, t, b, e);
    double s[3], y[3];
    track_wtx(a, a.p, t, b, e, s);
    mv3(a.Minv + 9 * (size_t)t, s, y);
    for (int k = 0; k < 3; ++k) a.y[3 * (size_t)t + k] = y[k];
}

// one workgroup per camera over the camera-major index: w = H9_c [p_c; p_k] - sum_m J9_m^T (Jp_m y_track(m)). Per camera
// mode: q_c = w + lambda [p_c; p_k]. Shared mode: q_c = w[0:6] + lambda p_c, and w[6:9] is the camera's share of the
// border row, written to its slot.
__global__ __launch_bounds__(kCamBlock) void gbc_prod_cams(GbcArgs a, double lambda) {
    __shared__ double sh[16 * 9];
    const int c = blockIdx.x;
    const int nb = a.shared ? 6 : 9;
    if (!a.modelled[c]) {
        if (threadIdx.x < nb) a.q[(size_t)nb * c + threadIdx.x] = 0.0;
        if (a.shared && threadIdx.x < 3) a.pslot[3 * (size_t)c + threadIdx.x] = 0.0;
        return;
    }
    double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = a.cam_off[c] + threadIdx.x; i < a.cam_off[c + 1]; i += kCamBlock) {
        const int m = a.perm[i];
        const double* L = a.lin + (size_t)m * kLin;
        const double* y = a.y + 3 * (size_t)a.mtrack[m];
        const double u0 = L[kJp] * y[0] + L[kJp + 1] * y[1] + L[kJp + 2] * y[2];
        const double u1 = L[kJp + 3] * y[0] + L[kJp + 4] * y[1] + L[kJp + 5] * y[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] += j9(L, 0, k) * u0 + j9(L, 1, k) * u1;
    }
    block_sum<9>(v, sh);
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        const double* H = a.H9 + 81 * (size_t)c + 9 * k;
        const double* pc = vec_pose(a, a.p, c);
        const double* pk = vec_calib(a, a.p, c);
        double s = 0.0;
        for (int j = 0; j < 6; ++j) s += H[j] * pc[j];
        for (int j = 0; j < 3; ++j) s += H[6 + j] * pk[j];
        if (k < nb) {
            s += lambda * (k < 6 ? pc[k] : pk[k - 6]);
            a.q[(size_t)nb * c + k] = s - v[k];
        } else {
            a.pslot[3 * (size_t)c + (k - 6)] = s - v[k];
        }
    }
}

__global__ __launch_bounds__(kVecBlock) void gbc_pcg_step(GbcArgs a, double lambda) {
    __shared__ double sh[16 * 3];
    const int n = nvec(a);
    double v[3] = {0.0, 0.0, 0.0};
    if (a.shared) {
        // the border row of q: the cameras' slots in a fixed order, then the prior and the damping
        for (int c = threadIdx.x; c < a.C; c += kVecBlock)
            for (int k = 0; k < 3; ++k) v[k] += a.pslot[3 * (size_t)c + k];
        block_sum<3>(v, sh);
        if (threadIdx.x < 3) {
            const size_t i = 6 * (size_t)a.C + threadIdx.x;
            a.q[i] = v[threadIdx.x] + (a.kprior_w + lambda) * a.p[i];
        }
        __syncthreads();
        v[0] = v[1] = 0.0;
    }
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
__global__ void gbc_retract(GbcArgs a, const double* X, const double* K, double* Xn, double* Kn) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    Pose A, B;
    load_pose(X, c, A);
    pose_retract(A, vec_pose(a, a.x, c), B);
    for (int k = 0; k < 9; ++k) Xn[12 * (size_t)c + k] = B.R[k];
    for (int k = 0; k < 3; ++k) Xn[12 * (size_t)c + 9 + k] = B.t[k];
    const double* dk = vec_calib(a, a.x, c);
    for (int k = 0; k < 3; ++k) Kn[5 * (size_t)c + k] = K[5 * (size_t)c + k] + dk[k];
    for (int k = 3; k < 5; ++k) Kn[5 * (size_t)c + k] = K[5 * (size_t)c + k];
}

__global__ void gbc_backsub(GbcArgs a, const double* Xn, const double* Kn, const double* P, double* Pn) {
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
        const double* dc = vec_pose(a, a.x, a.img[m]);
        const double* dk = vec_calib(a, a.x, a.img[m]);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            double v = -L[kB + r];
#pragma unroll
            for (int k = 0; k < 6; ++k) v += L[6 * r + k] * dc[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) v += L[kJk + 3 * r + k] * dk[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) v += L[kJp + 3 * r + k] * dp[k];
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
__global__ void gbc_filter(GbcArgs a, const double* X, const double* K, const double* P, double thresh,
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
        if (!project_k(Xc, K + 5 * (size_t)c, P + 3 * (size_t)t, pc, pr)) { good = false; break; }
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

__global__ void gbc_output(GbcArgs a, const double* X, const double* K, const double* P, double* wRc_out,
                           double* wtc_out, double* calib_out, double* point_out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)a.C) {
        for (int k = 0; k < 9; ++k) wRc_out[9 * i + k] = X[12 * i + k];
        for (int k = 0; k < 3; ++k) wtc_out[3 * i + k] = X[12 * i + 9 + k];
        for (int k = 0; k < 5; ++k) calib_out[5 * i + k] = K[5 * i + k];
    }
    if (i < (size_t)a.T)
        for (int k = 0; k < 3; ++k) point_out[3 * i + k] = P[3 * i + k];
}

__global__ __launch_bounds__(kVecBlock) void gbc_stats(GbcArgs a, const double* K, double* stats, double err0,
                                                       double err, double iters, double trials, double pcg_iters,
                                                       double cap_hits, double status) {
    __shared__ double sh[kVecBlock];
    double mx = 0.0;  // the largest |f - f_initial| / f_initial of a modelled camera (its own input f, in both modes)
    for (int c = threadIdx.x; c < a.C; c += kVecBlock)
        if (a.modelled[c]) mx = fmax(mx, fabs(K[5 * (size_t)c] - a.calib[5 * (size_t)c]) / fabs(a.calib[5 * (size_t)c]));
    sh[threadIdx.x] = mx;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int k = 1; k < kVecBlock; ++k) mx = fmax(mx, sh[k]);
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
    stats[10] = a.shared ? 1.0 : (double)a.icnt[I_NMOD];
    stats[11] = mx;
}

// ------------------------------------------------------------------ workspace
struct GbcLayout {
    size_t part, modelled, mtrack, cam_off, perm, hist, icnt, XA, XB, KA, KB, PA, PB, lin, H9, g9, Pinv, PinvK, dk,
        bslot, pslot, Hpp, Minv, rp, y, tl, te, vec, scal, total;
    CsrChunks chunks;
};

bool gbc_sizes_ok(long long n_tracks, long long n_meas, int n_img) {
    return n_tracks > 0 && n_meas > 0 && n_img > 0 && n_tracks < (1ll << 31) - 1 && n_meas < (1ll << 31) - 1 &&
           n_img <= (1 << 20);
}

constexpr size_t gbc_vec_len(size_t c) { return 9 * c + 3; }  // room for either mode: [C][9] or [6C | 3]

GbcLayout gbc_layout(long long T, long long M, int C) {
    GbcLayout L;
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
    L.KA = w.take(c * 5 * d);
    L.KB = w.take(c * 5 * d);
    L.PA = w.take(t * 3 * d);
    L.PB = w.take(t * 3 * d);
    L.lin = w.take(m * kLin * d);
    L.H9 = w.take(c * 81 * d);
    L.g9 = w.take(c * 9 * d);
    L.Pinv = w.take(c * 81 * d);
    L.PinvK = w.take(9 * d);
    L.dk = w.take(c * 3 * d);
    L.bslot = w.take(c * 9 * d);
    L.pslot = w.take(c * 3 * d);
    L.Hpp = w.take(t * 9 * d);
    L.Minv = w.take(t * 9 * d);
    L.rp = w.take(t * 3 * d);
    L.y = w.take(t * 3 * d);
    L.tl = w.take(t * d);
    L.te = w.take(t * d);
    L.vec = w.take(6 * gbc_vec_len(c) * d);
    L.scal = w.take(S_COUNT * d);
    L.total = w.o;
    return L;
}

}  // namespace

extern "C" {

size_t gtsfm_global_ba_calib_workspace_bytes(long long n_tracks, long long n_meas, int n_img) {
    if (!gbc_sizes_ok(n_tracks, n_meas, n_img)) return 0;
    return gbc_layout(n_tracks, n_meas, n_img).total;
}

int gtsfm_global_ba_calib(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                          long long n_tracks, const long long* d_n_tracks, long long n_meas, const double* d_point,
                          const uint8_t* d_track_valid, const uint8_t* d_meas_valid, const double* d_wRc,
                          const double* d_wtc, const double* d_calib, const uint8_t* d_cam_valid, int n_img,
                          int robust, double measurement_sigma, double cam_pose3_prior_sigma, int shared_calib,
                          double calibration_prior_sigma, int max_iterations, double pcg_rel_tol, int pcg_max_iter,
                          double reproj_error_thresh, void* d_workspace, size_t workspace_bytes, double* d_wRc_out,
                          double* d_wtc_out, double* d_calib_out, double* d_point_out, uint8_t* d_track_keep,
                          uint8_t* d_cam_keep, double* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_tracks < 0 || n_meas < 0 || n_img < 0 || n_tracks >= (1ll << 31) - 1 || n_meas >= (1ll << 31) - 1 ||
        n_img > (1 << 20) || !d_wRc_out || !d_wtc_out || !d_calib_out || !d_point_out || !d_track_keep ||
        !d_cam_keep || !d_stats || !(measurement_sigma > 0) || !(cam_pose3_prior_sigma > 0) ||
        !(calibration_prior_sigma > 0) || (shared_calib != 0 && shared_calib != 1) || max_iterations < 0 ||
        !(pcg_rel_tol > 0) || pcg_max_iter <= 0 || !(reproj_error_thresh > 0) || (uv_is_f64 != 0 && uv_is_f64 != 1))
        return GTSFM_ERR_ARG;
    if ((n_img > 0 && (!d_wRc || !d_wtc || !d_calib)) || (n_tracks > 0 && (!d_track_offsets || !d_point)) ||
        (n_meas > 0 && (!d_track_img || !d_track_uv)))
        return GTSFM_ERR_ARG;
    const int T = (int)n_tracks, M = (int)n_meas, C = n_img;
    const double nothing[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0};
    // the reference's early return (bundle_adjustment.py:319-324): inputs copied through, keep all zero, error 0
    auto copy_through = [&]() -> int {
        if (C > 0) {
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_wRc_out, d_wRc, (size_t)C * 9 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_wtc_out, d_wtc, (size_t)C * 3 * sizeof(double),
                                           hipMemcpyDeviceToDevice, stream));
            GTSFM_CHECK_HIP(hipMemcpyAsync(d_calib_out, d_calib, (size_t)C * 5 * sizeof(double),
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
    const GbcLayout L = gbc_layout(T, M, C);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    GbcArgs a;
    a.off = d_track_offsets; a.img = d_track_img; a.uv = d_track_uv; a.uv64 = uv_is_f64; a.d_nt = d_n_tracks;
    a.T = T; a.M = M; a.C = C;
    a.point_in = d_point; a.tvalid = d_track_valid; a.mvalid = d_meas_valid;
    a.wRc = d_wRc; a.wtc = d_wtc; a.calib = d_calib; a.cvalid = d_cam_valid;
    a.robust = robust != 0;
    a.shared = shared_calib;
    a.isig = 1.0 / measurement_sigma;
    a.prior_w = 1.0 / (cam_pose3_prior_sigma * cam_pose3_prior_sigma);
    a.kprior_w = 1.0 / (calibration_prior_sigma * calibration_prior_sigma);
    a.part = ws + L.part; a.modelled = ws + L.modelled;
    a.mtrack = (int*)(ws + L.mtrack); a.cam_off = (int*)(ws + L.cam_off); a.perm = (int*)(ws + L.perm);
    a.hist = (int*)(ws + L.hist); a.icnt = (int*)(ws + L.icnt);
    a.XA = (double*)(ws + L.XA); a.XB = (double*)(ws + L.XB);
    a.KA = (double*)(ws + L.KA); a.KB = (double*)(ws + L.KB);
    a.PA = (double*)(ws + L.PA); a.PB = (double*)(ws + L.PB);
    a.lin = (double*)(ws + L.lin); a.H9 = (double*)(ws + L.H9); a.g9 = (double*)(ws + L.g9);
    a.Pinv = (double*)(ws + L.Pinv); a.PinvK = (double*)(ws + L.PinvK); a.dk = (double*)(ws + L.dk);
    a.bslot = (double*)(ws + L.bslot); a.pslot = (double*)(ws + L.pslot);
    a.Hpp = (double*)(ws + L.Hpp); a.Minv = (double*)(ws + L.Minv);
    a.rp = (double*)(ws + L.rp); a.y = (double*)(ws + L.y); a.tl = (double*)(ws + L.tl);
    a.te = (double*)(ws + L.te);
    double* vec = (double*)(ws + L.vec);
    const size_t nv = gbc_vec_len((size_t)C);
    a.bvec = vec; a.x = vec + nv; a.r = vec + 2 * nv; a.z = vec + 3 * nv; a.p = vec + 4 * nv; a.q = vec + 5 * nv;
    a.scal = (double*)(ws + L.scal);
    a.chunks = L.chunks;

    const unsigned B = 256;
    const unsigned gT = blocks_for(T, B), gM = blocks_for(M, B), gC = blocks_for(C, B);
    const size_t nmax = (size_t)(T > M ? T : M) > (size_t)C ? (size_t)(T > M ? T : M) : (size_t)C;
    int icnt[I_COUNT];
    double scal[6];
    auto read_icnt = [&]() { return read_back(icnt, a.icnt, I_COUNT, stream); };
    auto read_scal = [&]() { return read_back(scal, a.scal, 6, stream); };

    hipLaunchKernelGGL(gbc_init, dim3(blocks_for(nmax, B)), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(gbc_setup_tracks, dim3(gT), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(gbc_setup_cams, dim3(gC), dim3(B), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    int rc = read_icnt();
    if (rc != GTSFM_OK) return rc;
    if (icnt[I_NPART] == 0 || icnt[I_NMOD] == 0) return copy_through();
    if (a.shared) hipLaunchKernelGGL(gbc_share_calib, dim3(gC), dim3(B), 0, stream, a);

    if ((rc = csr_build(GbaByCamera{a.mtrack, a.img, a.perm}, M, C, a.chunks, a.hist, a.cam_off, stream)) != GTSFM_OK)
        return rc;

    double* X = a.XA;
    double* Xn = a.XB;
    double* K = a.KA;
    double* Kn = a.KB;
    double* P = a.PA;
    double* Pn = a.PB;
    hipLaunchKernelGGL(gbc_eval, dim3(gT), dim3(B), 0, stream, a, X, K, P);
    hipLaunchKernelGGL(gbc_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, X, K, 0);
    GTSFM_CHECK_HIP(hipGetLastError());
    if ((rc = read_scal()) != GTSFM_OK) return rc;
    const double err0 = scal[S_NEWERR];
    double err = err0, lambda = 1e-5;
    const int max_iters = max_iterations > 0 ? max_iterations : 100;
    long long iters = 0, trials = 0, pcg_total = 0, cap_hits = 0;
    if (err > 0.0) {
        for (;;) {  // ends: every outer step either accepts (iters <= max_iters) or leaves err unchanged (dec = 0)
            const double cur = err;
            hipLaunchKernelGGL(gbc_linearize, dim3(gM), dim3(B), 0, stream, a, X, K, P);
            hipLaunchKernelGGL(gbc_track_lin, dim3(gT), dim3(B), 0, stream, a, P);
            hipLaunchKernelGGL(gbc_cam_lin, dim3(C), dim3(kCamBlock), 0, stream, a, X, K);
            hipLaunchKernelGGL(gbc_oldlin, dim3(1), dim3(kVecBlock), 0, stream, a);
            double oldLin = 0.0;
            bool have_oldlin = false;
            for (int inner = 0; inner < kInnerMax; ++inner) {
                ++trials;
                GTSFM_CHECK_HIP(hipMemsetAsync(a.icnt + I_BAD, 0, sizeof(int), stream));
                hipLaunchKernelGGL(gbc_track_damp, dim3(gT), dim3(B), 0, stream, a, lambda);
                hipLaunchKernelGGL(gbc_cam_build, dim3(C), dim3(kCamBlock), 0, stream, a, lambda);
                hipLaunchKernelGGL(gbc_pcg_init, dim3(1), dim3(kVecBlock), 0, stream, a, lambda);
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
                        hipLaunchKernelGGL(gbc_prod_tracks, dim3(gT), dim3(B), 0, stream, a);
                        hipLaunchKernelGGL(gbc_prod_cams, dim3(C), dim3(kCamBlock), 0, stream, a, lambda);
                        hipLaunchKernelGGL(gbc_pcg_step, dim3(1), dim3(kVecBlock), 0, stream, a, lambda);
                        GTSFM_CHECK_HIP(hipGetLastError());
                        const int rc2 = read_scal();
                        rr = scal[S_RR];
                        return rc2;
                    });
                    if (rc != GTSFM_OK) return rc;
                    hipLaunchKernelGGL(gbc_retract, dim3(gC), dim3(B), 0, stream, a, X, K, Xn, Kn);
                    hipLaunchKernelGGL(gbc_backsub, dim3(gT), dim3(B), 0, stream, a, Xn, Kn, P, Pn);
                    hipLaunchKernelGGL(gbc_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, Xn, Kn, 1);
                    GTSFM_CHECK_HIP(hipGetLastError());
                    if ((rc = read_scal()) != GTSFM_OK) return rc;
                    trial = lm_judge(err, oldLin, scal[S_NEWLIN], scal[S_NEWERR]);
                }
                if (trial.success) {
                    double* s = X; X = Xn; Xn = s;
                    s = K; K = Kn; Kn = s;
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
    hipLaunchKernelGGL(gbc_filter, dim3(gT), dim3(B), 0, stream, a, X, K, P, reproj_error_thresh, d_track_keep,
                       d_cam_keep);
    hipLaunchKernelGGL(gbc_output, dim3(blocks_for(T > C ? T : C, B)), dim3(B), 0, stream, a, X, K, P, d_wRc_out,
                       d_wtc_out, d_calib_out, d_point_out);
    hipLaunchKernelGGL(gbc_stats, dim3(1), dim3(kVecBlock), 0, stream, a, K, d_stats, err0, err, (double)iters,
                       (double)trials, (double)pcg_total, (double)cap_hits, 0.0);
    GTSFM_CHECK_HIP(hipGetLastError());
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    return GTSFM_OK;
}

}  // extern "C"
