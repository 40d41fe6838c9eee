// Self-calibrating global bundle adjustment: gba.hip's Levenberg-Marquardt over every camera pose and every landmark,
// with the Cal3Bundler calibration (f, k1, k2) of the cameras as variables too, one per modelled camera or one shared.
//
// Reference: gtsfm/bundle/bundle_adjustment.py:58-66 ("refines global pose estimates and intrinsics of cameras"),
// :103-131 and :180-208 (a K(i) per camera, or a single K(0) with shared_calib, in every GeneralSFMFactor2Cal3Bundler,
// and a PriorFactorCal3Bundler of calibration_prior_noise_sigma on each), :188-195 and :258-260 (the shared variable is
// the first camera's calibration, principal point included), on GTSAM 4.2's Cal3Bundler: u = f g x + u0 with
// g = 1 + (k1 + k2 r2) r2, three degrees of freedom (f, k1, k2), additive retraction. Everything else (participation,
// the pose and point priors, Huber, the cheirality treatment, the LM schedule, point elimination, PCG from a zero start,
// block-Jacobi preconditioning, fixed summation orders) is gba.hip's: both are gba_core.hpp's one solver, and this file
// is the refined model (the projection, the calibration prior, the shared mode's border, the retraction of K, the two
// extra stats) and its C entry points.
//
// A measurement's record is Jx 2 x 6, Jk 2 x 3, Jp 2 x 3, b 2: 208 bytes (gba.hip: 160). With J9 = [Jx | Jk], every
// per-camera sum is gba.hip's with 9 in place of 6: H9_c = sum J9^T J9, the 9 x 9 block of the damped Schur complement
// and the 9-vector sum J9^T (Jp y) of a product. The two modes differ only in where the last three entries go:
//   per camera  the unknown is [C][9]; camera c's block is its own 9 x 9, inverted for the preconditioner;
//   shared      the unknown is [6C poses | 3]. A camera workgroup keeps the pose part (6 x 6 block, 6 entries of q) and
//               writes its contribution to the 3-wide border (the 3 x 3 diagonal block and right-hand side at build time,
//               the border row of q = S p in a product) into a slot of its own; the single-workgroup kernel that follows
//               (gba_pcg_init, gba_pcg_step) sums the slots in a fixed order (reduce.hpp), adds the prior and the
//               damping and, at build time, inverts the border block for the preconditioner.
// No floating-point atomics: two calls return the same bytes. LM / PCG control flow is host code (lm.hpp), so the entry
// point synchronises its stream; it allocates nothing.
#include "common.hpp"

#pragma clang fp contract(off)

#include "gba_core.hpp"

namespace {

struct GbaRefined;
using GbcArgs = GbaArgs<GbaRefined>;

__global__ void gbc_share_calib(GbcArgs a);

// Cal3Bundler (f, k1, k2) refined: a camera's block is [pose 6 | calibration 3] and its parameters are
// calib = (f, k1, k2, u0, v0). The static functions after project_k_jac are the hooks gba_core.hpp calls.
struct GbaRefined {
    static constexpr int kCal = 3, kCamStride = 5, kStats = 12;
    struct Extra {
        int shared;
        double kprior_w;  // 1 / calibration_prior_sigma^2
        double* KA;       // [C][5] the calibration variable, double-buffered like the poses: KA is the current one,
        double* KB;       // KB the trial's (the driver swaps them when a trial is accepted)
        double* PinvK;    // [9] shared: the border block's inverse
        double* dk;       // [C][3] calibration minus its prior at the linearisation point (shared: row c0 only)
        double* bslot;    // [C][9] shared, build: the camera's share of the border block (6) and right-hand side (3)
        double* pslot;    // [C][3] shared, product: the camera's share of the border row of q
    };

    // Cal3Bundler projection, K = (f, k1, k2, u0, v0); pc is the point in the camera frame; false when z <= 0
    __device__ static __forceinline__ bool project(const Pose& X, const double* K, const double* p, double* pc,
                                                   double* uv) {
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
    __device__ static __forceinline__ void project_jac(const Pose& X, const double* K, const double* pc, double* Jp,
                                                       double* Jx, double* Jk) {
        const double iz = 1.0 / pc[2], x = pc[0] * iz, y = pc[1] * iz, f = K[0];
        const double r2 = x * x + y * y;
        const double g = 1.0 + (K[1] + K[2] * r2) * r2;
        const double h = 2.0 * (K[1] + 2.0 * K[2] * r2);
        // d uv / d (x, y) = f (g I + h [x; y][x y])
        const double A00 = f * (g + h * x * x), A01 = f * (h * x * y), A11 = f * (g + h * y * y);
        // times d (x, y) / d pc = [[iz, 0, -x iz], [0, iz, -y iz]]
        const double D[6] = {A00 * iz, A01 * iz, -(A00 * x + A01 * y) * iz,
                             A01 * iz, A11 * iz, -(A01 * x + A11 * y) * iz};
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

    // the calibration the prior of camera c's variable sits at
    __device__ static __forceinline__ const double* calib_prior(const GbcArgs& a, int c) {
        return a.cam + 5 * (size_t)(a.shared ? a.icnt[I_C0] : c);
    }

    // gba_init, camera i
    __device__ static __forceinline__ void init_cam(const GbcArgs& a, size_t i) {
        for (int k = 0; k < 5; ++k) a.KA[5 * i + k] = a.KB[5 * i + k] = a.cam[5 * i + k];
        for (int k = 0; k < 3; ++k) a.dk[3 * i + k] = 0.0;
    }

    // after the setup kernels
    static void start_calib(const GbcArgs& a, unsigned grid, unsigned block, hipStream_t stream) {
        if (a.shared) hipLaunchKernelGGL(gbc_share_calib, dim3(grid), dim3(block), 0, stream, a);
    }

    // ---------------------------------------------------------------- the calibration prior
    // gba_reduce, every lane: v[2] += |Kerr - K0|^2 and, with_lin, v[3] += |dx_k + dk|^2 over the calibration variables
    __device__ static __forceinline__ void reduce_calib_prior(const GbcArgs& a, const double* Kerr, int with_lin,
                                                              double* v) {
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
    }

    // gba_cam_lin, lane 0 of camera c: stores the prior's residual dk = K - K0 and, per camera mode, adds the prior of
    // this camera's variable to H and g (the shared variable's prior joins the border in border_init)
    __device__ static __forceinline__ void cam_lin_calib_prior(const GbcArgs& a, int c, const double* K, double* H,
                                                               double* g) {
        if (a.shared && c != a.icnt[I_C0]) return;
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

    // gba_oldlin, every lane: v[1] += sum |dk|^2
    __device__ static __forceinline__ void oldlin_calib_prior(const GbcArgs& a, double* v) {
        const int c0 = a.icnt[I_C0];
        for (int c = threadIdx.x; c < a.C; c += kVecBlock) {
            if (!a.modelled[c] || (a.shared && c != c0)) continue;
            for (int k = 0; k < 3; ++k) v[1] += a.dk[3 * (size_t)c + k] * a.dk[3 * (size_t)c + k];
        }
    }

    // ---------------------------------------------------------------- the shared mode's border
    // gba_cam_build, lane 0 of camera c, shared mode. S is the undamped 9 x 9 block, v the workgroup's sums: the damped
    // 6 x 6 pose block inverted is the preconditioner, and the calibration rows and columns go to the camera's slot.
    __device__ static __forceinline__ void build_border(const GbcArgs& a, int c, double lambda, const double* S,
                                                        const double* g, const double* v, double* Inv) {
        constexpr int kSym = GbaDims<GbaRefined>::kSym;
        double* Pm = a.Pinv + 81 * (size_t)c;
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
        for (int r = 0; r < 6; ++r) a.bvec[6 * (size_t)c + r] = g[r] - v[kSym + r];
        double* bs = a.bslot + 9 * (size_t)c;
        int n = 0;
        for (int r = 6; r < 9; ++r)
            for (int s = r; s < 9; ++s, ++n) bs[n] = S[9 * r + s];
        for (int r = 0; r < 3; ++r) bs[6 + r] = g[6 + r] - v[kSym + 6 + r];
    }

    // precond_row, shared mode: a pose row of its camera's 6 x 6, or a row of the border block
    __device__ static __forceinline__ double precond_row_shared(const GbcArgs& a, int i) {
        double s = 0.0;
        if (i < 6 * a.C) {
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

    // gba_pcg_init, every lane, shared mode: the border's 3 x 3 block of the damped Schur complement, inverted, and its
    // right-hand side. sh holds 16 * 9 doubles.
    __device__ static __forceinline__ void border_init(const GbcArgs& a, double lambda, double* sh) {
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

    // gba_pcg_step, every lane, shared mode: the border row of q is the cameras' slots in a fixed order, then the prior
    // and the damping. sh holds 16 * 3 doubles.
    __device__ static __forceinline__ void border_q(const GbcArgs& a, double lambda, double* sh) {
        double w[3] = {0.0, 0.0, 0.0};
        for (int c = threadIdx.x; c < a.C; c += kVecBlock)
            for (int k = 0; k < 3; ++k) w[k] += a.pslot[3 * (size_t)c + k];
        block_sum<3>(w, sh);
        if (threadIdx.x < 3) {
            const size_t i = 6 * (size_t)a.C + threadIdx.x;
            a.q[i] = w[threadIdx.x] + (a.kprior_w + lambda) * a.p[i];
        }
        __syncthreads();
    }

    // ---------------------------------------------------------------- the retraction of K, the stats, the workspace
    // gba_retract, camera c, from the current calibration KA to the trial's KB: additive in (f, k1, k2); the principal
    // point is not a variable
    __device__ static __forceinline__ void retract_calib(const GbcArgs& a, int c) {
        const double* dk = vec_calib(a, a.x, c);
        for (int k = 0; k < 3; ++k) a.KB[5 * (size_t)c + k] = a.KA[5 * (size_t)c + k] + dk[k];
        for (int k = 3; k < 5; ++k) a.KB[5 * (size_t)c + k] = a.KA[5 * (size_t)c + k];
    }

    // gba_stats, every lane of its kVecBlock: stats[10] the calibration variables, stats[11] the largest
    // |f - f_initial| / f_initial of a modelled camera (its own input f, in both modes)
    __device__ static __forceinline__ void extra_stats(const GbcArgs& a, const double* K, double* stats) {
        __shared__ double sh[kVecBlock];
        double mx = 0.0;
        for (int c = threadIdx.x; c < a.C; c += kVecBlock)
            if (a.modelled[c]) mx = fmax(mx, fabs(K[5 * (size_t)c] - a.cam[5 * (size_t)c]) / fabs(a.cam[5 * (size_t)c]));
        sh[threadIdx.x] = mx;
        __syncthreads();
        if (threadIdx.x != 0) return;
        for (int k = 1; k < kVecBlock; ++k) mx = fmax(mx, sh[k]);
        stats[10] = a.shared ? 1.0 : (double)a.icnt[I_NMOD];
        stats[11] = mx;
    }

    static void carve(GbcArgs& a, GbaCarver& cv, size_t c) {
        cv.piece(a.KA, c * 5);
        cv.piece(a.KB, c * 5);
        cv.piece(a.PinvK, 9);
        cv.piece(a.dk, c * 3);
        cv.piece(a.bslot, c * 9);
        cv.piece(a.pslot, c * 3);
    }
};

// shared mode: every modelled camera starts from the calibration of the modelled camera of lowest index, principal
// point included (bundle_adjustment.py:188-195, :258-260)
__global__ void gbc_share_calib(GbcArgs a) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C || !a.modelled[c]) return;
    const double* k0 = a.cam + 5 * (size_t)a.icnt[I_C0];
    for (int k = 0; k < 5; ++k) a.KA[5 * (size_t)c + k] = a.KB[5 * (size_t)c + k] = k0[k];
}

}  // namespace

extern "C" {

size_t gtsfm_global_ba_calib_workspace_bytes(long long n_tracks, long long n_meas, int n_img) {
    return gba_workspace_bytes<GbaRefined>(n_tracks, n_meas, n_img);
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
    if (!(calibration_prior_sigma > 0) || (shared_calib != 0 && shared_calib != 1)) return GTSFM_ERR_ARG;
    GbaRefined::Extra extra = {};
    extra.shared = shared_calib;
    extra.kprior_w = 1.0 / (calibration_prior_sigma * calibration_prior_sigma);
    return gba_run<GbaRefined>(extra, d_track_offsets, d_track_img, d_track_uv, uv_is_f64, n_tracks, d_n_tracks,
                               n_meas, d_point, d_track_valid, d_meas_valid, d_wRc, d_wtc, d_calib, d_cam_valid, n_img,
                               robust, measurement_sigma, cam_pose3_prior_sigma, max_iterations, pcg_rel_tol,
                               pcg_max_iter, reproj_error_thresh, d_workspace, workspace_bytes, d_wRc_out, d_wtc_out,
                               d_calib_out, d_point_out, d_track_keep, d_cam_keep, d_stats, (hipStream_t)stream_v);
}

}  // extern "C"
