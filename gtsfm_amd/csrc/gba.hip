// Global bundle adjustment: one Levenberg-Marquardt over every camera pose and every landmark of a track CSR.
//
// Reference: gtsfm/bundle/bundle_adjustment.py:58-397 (BundleAdjustmentOptimizer.run_ba_stage_with_filtering, run_ba),
// gtsfm/bundle/global_ba.py and gtsfm/common/gtsfm_data.py:389-427 (filter_landmarks), on GTSAM 4.2's
// LevenbergMarquardtOptimizer. The factors, the priors, the retraction, the cheirality treatment and the LM schedule
// are ba2.hip's, generalised from two cameras (camera 0 = identity) to N cameras with an arbitrary first camera; the
// SO(3) / SE(3) helpers are se3.hpp's for both. This entry point holds calibration fixed (k1 = k2 = 0), as
// ba2.hip:19-22 states; gba_calib.hip is the same solver with Cal3Bundler (f, k1, k2) refined, per camera or shared. The
// solver itself (kernels, workspace, host driver) is gba_core.hpp's, a template on the camera model; this file is the
// fixed model and its C entry points.
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
#include "common.hpp"

#pragma clang fp contract(off)

#include "gba_core.hpp"

namespace {

// Calibration held fixed: a camera's block is its 6 pose columns, its parameters are intr = (f, u0, v0), and the
// projection is se3.hpp's (k1 = k2 = 0). No model-specific argument.
struct GbaFixed {
    static constexpr int kCal = 0, kCamStride = 3, kStats = 10;
    struct Extra {};
    __device__ static __forceinline__ bool project(const Pose& X, const double* K, const double* p, double* pc,
                                                   double* uv) {
        return ::project(X, K, p, pc, uv);
    }
    __device__ static __forceinline__ void project_jac(const Pose& X, const double* K, const double* pc, double* Jp,
                                                       double* Jx, double*) {
        ::project_jac(X, K, pc, Jp, Jx);
    }
};

}  // namespace

extern "C" {

size_t gtsfm_global_ba_workspace_bytes(long long n_tracks, long long n_meas, int n_img) {
    return gba_workspace_bytes<GbaFixed>(n_tracks, n_meas, n_img);
}

int gtsfm_global_ba(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                    long long n_tracks, const long long* d_n_tracks, long long n_meas, const double* d_point,
                    const uint8_t* d_track_valid, const uint8_t* d_meas_valid, const double* d_wRc,
                    const double* d_wtc, const double* d_intrinsics, const uint8_t* d_cam_valid, int n_img, int robust,
                    double measurement_sigma, double cam_pose3_prior_sigma, int max_iterations, double pcg_rel_tol,
                    int pcg_max_iter, double reproj_error_thresh, void* d_workspace, size_t workspace_bytes,
                    double* d_wRc_out, double* d_wtc_out, double* d_point_out, uint8_t* d_track_keep,
                    uint8_t* d_cam_keep, double* d_stats, void* stream_v) {
    return gba_run<GbaFixed>({}, d_track_offsets, d_track_img, d_track_uv, uv_is_f64, n_tracks, d_n_tracks, n_meas,
                             d_point, d_track_valid, d_meas_valid, d_wRc, d_wtc, d_intrinsics, d_cam_valid, n_img,
                             robust, measurement_sigma, cam_pose3_prior_sigma, max_iterations, pcg_rel_tol,
                             pcg_max_iter, reproj_error_thresh, d_workspace, workspace_bytes, d_wRc_out, d_wtc_out,
                             nullptr, d_point_out, d_track_keep, d_cam_keep, d_stats, (hipStream_t)stream_v);
}

}  // extern "C"
