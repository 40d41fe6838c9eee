/*
 * gtsfm_hip.h — C ABI of the MI355X-native GTSfM two-view front-end (libgtsfm_hip.so, gfx950).
 *
 * Every entry point takes plain pointers and sizes. Pointers named d_* are DEVICE pointers (HBM);
 * `stream` is a hipStream_t passed as void* (NULL = default stream). No entry point allocates,
 * synchronises or copies to the host: callers own every buffer and size workspaces with the
 * matching *_workspace_bytes() query, so a call can be captured into a hipGraph. The one exception is
 * gtsfm_global_ba, whose LM / PCG control flow reads scalars back and synchronises its stream (see its block).
 * Return value: GTSFM_OK (0) or a negative GTSFM_ERR_* code. Degenerate DATA (too few matches,
 * no model) is never an error: it is reported per pair, as the reference reports a failure tuple.
 *
 * Reference interfaces replaced (file:line in alphonse-CHEN/gtsfm @ 2025-01-17):
 *   gtsfm_match_*           <- gtsfm/frontend/matcher/twoway_matcher.py:42-144 TwoWayMatcher.match
 *                              (cv.BFMatcher(NORM_L2).knnMatch(k=2) x 2 directions + ratio + mutual + sort)
 *   gtsfm_ransac_*          <- gtsfm/frontend/verifier/opencv_verifier_base.py:45-109 verify +
 *                              gtsfm/frontend/verifier/ransac.py:52-82 estimate_E +
 *                              gtsfm/utils/verification.py:52-94 recover_relative_pose_from_essential_matrix +
 *                              gtsfm/frontend/inlier_support_processor.py:39-95 run_inlier_support
 *   gtsfm_sift_*            <- gtsfm/frontend/detector_descriptor/sift.py:27-56 detect_and_describe
 *                              (cv.cvtColor RGB2GRAY + cv.SIFT_create().detectAndCompute + Keypoints.get_top_k)
 *   gtsfm_d2net_*           <- gtsfm/frontend/detector_descriptor/d2net.py:47-88 detect_and_describe +
 *                              thirdparty/d2net/lib/model_test.py:12-200, pyramid.py:16-146, utils.py:34-38, 77-164
 *   gtsfm_retrieval_*       <- gtsfm/retriever/netvlad_retriever.py:77-228 (similarity blocks + pairs_from_score_matrix)
 *   gtsfm_netvlad_*         <- gtsfm/frontend/global_descriptor/netvlad_global_descriptor.py:27-46 describe +
 *                              thirdparty/hloc/netvlad.py:28-71 (NetVLADLayer), :160-191 (NetVLAD.forward)
 *   gtsfm_viewgraph_*       <- gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:49-152
 *                              CycleConsistentRotationViewGraphEstimator.run + gtsfm/utils/graph.py:100-135
 *                              extract_cyclic_triplets_from_edges + gtsfm/utils/geometry_comparisons.py:355-370
 *                              compute_cyclic_rotation_error
 *   gtsfm_tracks_*          <- gtsfm/data_association/dsf_tracks_estimator.py:56-85 DsfTracksEstimator.run,
 *                              cpp_dsf_tracks_estimator.py:63-74 (gtsam tracksFromPairwiseMatches) and
 *                              gtsfm/common/sfm_track.py:105-112 validate_unique_cameras
 *   gtsfm_triangulate_*     <- gtsfm/data_association/point3d_initializer.py:117-380 Point3dInitializer.triangulate
 *                              (execute_ransac_variant, sample_ransac_hypotheses, extract_measurements), one call per
 *                              track from gtsfm/data_association/data_assoc.py:211-273 run_triangulation;
 *                              gtsfm/utils/reprojection.py:48-83 and gtsfm/utils/tracks.py:82-102
 *   gtsfm_global_ba*        <- gtsfm/bundle/bundle_adjustment.py:58-397 BundleAdjustmentOptimizer.run_ba,
 *                              gtsfm/bundle/global_ba.py and gtsfm/common/gtsfm_data.py:389-427 filter_landmarks
 *   gtsfm_assemble_ba_input* <- gtsfm/data_association/data_assoc.py:123-160 assemble_gtsfm_data_from_tracks (no
 *                              metrics), gtsfm/common/gtsfm_data.py:238-317 select_largest_connected_component and
 *                              from_selected_cameras, gtsfm/utils/graph.py:20-39
 *   gtsfm_mvs_*             <- gtsfm/densify/patchmatchnet_data.py:78-162 select_src_views_depth_ranges,
 *                              gtsfm/densify/mvs_patchmatchnet.py:201-437 filter_depth with
 *                              thirdparty/patchmatchnet/eval.py:11-125, gtsfm/densify/mvs_base.py:75-92 and
 *                              gtsfm/densify/mvs_utils.py:148-221 (everything around the depth network)
 *   gtsfm_patchmatchnet_*   <- gtsfm/densify/mvs_patchmatchnet.py:95-175 (the model call of densify) and
 *                              thirdparty/patchmatchnet/models/net.py, patchmatch.py, module.py (the network)
 */
#ifndef GTSFM_HIP_H_
#define GTSFM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GTSFM_OK 0
#define GTSFM_ERR_ARG (-1)      /* invalid argument (shape, null pointer, unsupported mode) */
#define GTSFM_ERR_HIP (-2)      /* a HIP runtime call failed */
#define GTSFM_ERR_CAPACITY (-3) /* workspace too small */

/* ----------------------------------------------------------------------------------------------
 * Library
 * ---------------------------------------------------------------------------------------------- */
/* ABI version (major*100 + minor); a binding built against this header checks that the library
 * returns GTSFM_HIP_ABI_VERSION before binding anything else. */
/* Stays 407 with gtsfm_rotavg_* and gtsfm_assemble_ba_input* added: new symbols only, no existing signature or
 * meaning changed, so no caller of a 407 library breaks. */
#define GTSFM_HIP_ABI_VERSION 407
int gtsfm_hip_abi_version(void);
/* Name of the offload target the kernels were compiled for (e.g. "gfx950"). */
const char* gtsfm_hip_target(void);

/* ----------------------------------------------------------------------------------------------
 * Matcher: mutual nearest neighbour + Lowe ratio test over a batch of image pairs.
 *
 * Descriptors of all images live in one padded array d_desc[n_img][kmax][dim] float32 with
 * d_counts[n_img] valid rows per image. d_pairs[n_pairs][2] holds (i1, i2) image indices.
 * Output: d_out_idx[n_pairs][kmax][2] uint32 (i1 keypoint, i2 keypoint) and d_out_count[n_pairs];
 * rows 0..count-1 of each pair are ordered exactly like TwoWayMatcher.match's result
 * (ascending 1->2 distance, ties by i1 index). ratio < 0 disables the ratio test.
 *
 * mode GTSFM_MATCH_EXACT_F32: any float descriptors; distances are sum_k (a_k-b_k)^2 in float32,
 *      sequential k (bit-exact with the oracle; equals OpenCV for integer data or dim == 1).
 * mode GTSFM_MATCH_INT_F16:   integer-valued descriptors in [0, 1023] with squared norm < 2^19
 *      (every SIFT descriptor). One fp16 MFMA distance GEMM per pair with the norms and a 4-bit row code
 *      folded into extra K columns (every accumulator is d2 + code/16, exact in any summation order), fused
 *      row/column top-2. Exact integer arithmetic: bit-identical to EXACT_F32.
 *      kmax <= 8192, dim <= 139. (EXACT_F32: kmax <= 65535.)
 * mode GTSFM_MATCH_F16_RERANK: any float descriptors with dim <= 512 (e.g. SuperPoint's 256-D and D2-Net's 512-D
 *      unit vectors). An fp16 MFMA distance GEMM shortlists 8 candidates per keypoint and side (operands zero-padded
 *      to 64, 128, 256 or 512 columns), an exact fp32 re-rank with EXACT_F32's arithmetic recomputes them, and a
 *      rounding-error certificate proves the shortlist holds the exact top 2; uncertified keypoints (and images
 *      with |value| > 60000 or non-finite values) are rescanned exactly. Bit-identical to EXACT_F32. dim > 512 runs
 *      the EXACT_F32 kernels. kmax <= 65535.
 * ---------------------------------------------------------------------------------------------- */
#define GTSFM_MATCH_EXACT_F32 0
#define GTSFM_MATCH_INT_F16 1
#define GTSFM_MATCH_F16_RERANK 2

size_t gtsfm_match_workspace_bytes(int n_img, int kmax, int dim, int n_pairs, int mode);

int gtsfm_match_batched(const float* d_desc, const int* d_counts, int n_img, int kmax, int dim,
                        const int* d_pairs, int n_pairs, double ratio, int mode, void* d_workspace,
                        size_t workspace_bytes, uint32_t* d_out_idx, int* d_out_count, void* stream);

/* gtsfm_match_batched with the INT_F16 distance GEMM's work laid out by the caller (no reference counterpart: the
 * reference matches one pair per call, twoway_matcher.py:42-144 via det_desc_correspondence_generator.py:60-75).
 * d_groups[n_groups][group_size] lists pair indices (-1 = empty slot); every pair must appear exactly once, and the
 * pairs of one group should share image i1 (the operand a workgroup keeps in registers: it is then read once per
 * group instead of once per pair; a group mixing i1 images is correct, only slower). group_size <=
 * gtsfm_match_max_group(kmax, dim). Group order sets which workgroups run side by side on an XCD: consecutive groups
 * that stream the same few i2 images share that XCD's L2. d_groups == NULL is gtsfm_match_batched. Other modes
 * ignore the groups. */
int gtsfm_match_batched_grouped(const float* d_desc, const int* d_counts, int n_img, int kmax, int dim,
                                const int* d_pairs, int n_pairs, const int* d_groups, int n_groups, int group_size,
                                double ratio, int mode, void* d_workspace, size_t workspace_bytes,
                                uint32_t* d_out_idx, int* d_out_count, void* stream);

/* Largest group_size gtsfm_match_batched_grouped accepts for this kmax / dim (its LDS holds the column state of every
 * pair of a group); 0 when INT_F16 does not support the shape. */
int gtsfm_match_max_group(int kmax, int dim);

/* Measurement hook (no reference counterpart): hipEvent_t handles recorded on the call's stream immediately before
 * and after the distance-GEMM kernel of every later GTSFM_MATCH_INT_F16 gtsfm_match_batched call, so a benchmark can
 * time that one kernel. NULL, NULL switches it off. Process-wide; not thread-safe. */
int gtsfm_match_set_kernel_events(void* hip_event_start, void* hip_event_stop);

/* Measurement hook (no reference counterpart): after a GTSFM_MATCH_F16_RERANK gtsfm_match_batched call (dim <= 512) has
 * completed on `stream`, the number of (keypoint, side) entries whose fp16 shortlist was not certified (and were
 * recomputed exactly), and optionally per pair and side (h_uncertified_per_side[side * n_pairs + p], side 0 = rows of
 * i1). A (pair, side) with at least 1/32 of its keypoints uncertified is recomputed whole by the exact tile kernel,
 * the rest one keypoint at a time. Same workspace and shape arguments as the call; blocks until the copies land. */
int gtsfm_match_rerank_stats(const void* d_workspace, size_t workspace_bytes, int n_img, int kmax, int dim,
                             int n_pairs, int* h_uncertified, int* h_uncertified_per_side, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Verifier: essential-matrix RANSAC over a batch of image pairs (use_intrinsics_in_verification=True path).
 *
 * Keypoints of all images: d_kp_xy[n_img][kmax][2] float32 pixels; d_intrinsics[n_img][3] = (f, u0, v0)
 * (Cal3Bundler with k1 = k2 = 0). Putatives per pair: d_match_idx[n_pairs][mcap][2] uint32 keypoint indices
 * and d_match_count[n_pairs] (exactly the matcher's output). Threshold thr_px / max(f1, f2) in normalized
 * coordinates on the squared Sampson distance, success probability `prob`, at most `max_iters` hypotheses
 * (checked per batch of 64); `seed` and the pair id key the deterministic sampling of pair p: d_pair_ids[p]
 * when d_pair_ids is non-NULL (e.g. all 0 to reproduce one-pair calls), else pair_id_base + p.
 * Model selection `scoring` (ransac.py:58 robust_estimation_type): GTSFM_RANSAC_SCORING_MSAC for USAC_* (the default
 * USAC_ACCURATE scores models by MSAC: sum of min(squared Sampson error, thr^2)), each term quantised to
 * floor(e * 2^16 / thr^2) (65536 for an outlier) so the sum is exact in any order; GTSFM_RANSAC_SCORING_RANSAC for
 * cv2 RANSAC (inlier count). Local optimisation keeps a refit by the same criterion.
 * Outputs per pair: E, R (i2Ri1) row-major 3x3, unit t (i2ti1), inlier count, status (0 ok, 1 fewer than
 * 6 putatives, 2 no model), number of hypotheses evaluated (d_n_hyp may be NULL), number of candidate models scored
 * (the real 5-point solutions of those hypotheses; d_n_models may be NULL; a measurement output with no reference
 * counterpart, it prices the RANSAC FLOP count of SURVEY.md §8(d)) and the inlier mask d_inlier_mask[n_pairs][mcap]
 * over the putatives in matcher order. mcap < 2^19, and mcap <= 65535 with MSAC (the selection key's widths):
 * GTSFM_ERR_ARG otherwise.
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_ransac_workspace_bytes(int n_pairs, int mcap);

#define GTSFM_RANSAC_SCORING_RANSAC 0 /* most inliers wins (cv2 RANSAC) */
#define GTSFM_RANSAC_SCORING_MSAC 1   /* lowest truncated-quadratic cost wins (USAC_ACCURATE's MSAC score) */

int gtsfm_ransac_E_batched(const float* d_kp_xy, const double* d_intrinsics, int n_img, int kmax,
                           const int* d_pairs, int n_pairs, const uint32_t* d_match_idx,
                           const int* d_match_count, int mcap, double thr_px, double prob, int max_iters,
                           int scoring, uint64_t seed, int pair_id_base, const int* d_pair_ids, void* d_workspace,
                           size_t workspace_bytes, double* d_E, double* d_R, double* d_t, int* d_n_inliers, int* d_status,
                           int* d_n_hyp, int* d_n_models, uint8_t* d_inlier_mask, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Verifier, fundamental-matrix path (use_intrinsics_in_verification=False). Replaces Ransac.estimate_F
 * (gtsfm/frontend/verifier/ransac.py:84-111: cv2.findFundamentalMat(FM_RANSAC, thr_px, 0.999999, 1e6)) and the
 * F branch of OpencvVerifierBase.verify (opencv_verifier_base.py:90-109: E = K2^T F K1, recoverPose on the
 * K-normalised inliers). Same inputs as gtsfm_ransac_E_batched; pixel coordinates are used for estimation.
 * 7-point RANSAC for M >= 15, LMedS for 8 <= M < 15, normalised 8-point refit on the inliers.
 * Outputs per pair: F (F33 = 1), E, R (i2Ri1), unit t (i2ti1), inlier count, status (0 ok, 1 fewer than 8
 * putatives, 2 no model), hypotheses drawn (d_n_hyp may be NULL), inlier mask d_inlier_mask[n_pairs][mcap].
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_ransac_F_workspace_bytes(int n_pairs, int mcap);

int gtsfm_ransac_F_batched(const float* d_kp_xy, const double* d_intrinsics, int n_img, int kmax,
                           const int* d_pairs, int n_pairs, const uint32_t* d_match_idx,
                           const int* d_match_count, int mcap, double thr_px, double prob, int max_iters,
                           uint64_t seed, int pair_id_base, const int* d_pair_ids, void* d_workspace,
                           size_t workspace_bytes, double* d_F, double* d_E, double* d_R, double* d_t,
                           int* d_n_inliers, int* d_status, int* d_n_hyp, uint8_t* d_inlier_mask, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Two-view triangulation + bundle adjustment. Replaces TwoViewEstimator.bundle_adjust and the run_2view branch
 * that calls it (gtsfm/two_view_estimator.py:101-208, 311-337; gtsam.triangulatePoint3 + the 2-view
 * BundleAdjustmentOptimizer, bundle/bundle_adjustment.py:269-275, 359-419), batched over pairs; the restatement is
 * oracle/ba2.c (calibrations held fixed; the reference's sigma 1e-5 prior pins them).
 * Inputs: the verifier's keypoints / intrinsics / pairs / putatives exactly as gtsfm_ransac_E_batched takes them,
 * its inlier mask d_in_mask[n_pairs][mcap] (the pre-BA verified rows), i2Ri1 d_R_in[n_pairs][9], unit i2ti1
 * d_t_in[n_pairs][3] and status d_status_in (0 = verified). Optional relative-pose priors (two_view_estimator.py:165,
 * 192: bundle_adjust's i2Ti1_prior): d_prior_Rt[n_pairs][12] = the prior's i2Ti1 (R row-major, then t) and
 * d_prior_sigmas[n_pairs][6] its sigmas (PosePrior.covariance, rotation first); a pair with sigma[0] <= 0 has none,
 * both NULL = no priors. A prior initialises the second camera and adds BetweenFactorPose3(X0, X1, prior^-1)
 * (bundle_adjustment.py:136-152). Per pair with status 0 and >= min_inliers verified rows:
 * every verified row is triangulated (DLT + LM point refinement, cheirality, reprojection < tri_thresh px), the
 * 2-view BA runs (Huber 1.345 on 1 px, X0 prior 0.1, first-point prior 0.1, Levenberg-Marquardt <= max_iters
 * iterations), and rows whose two reprojections stay < reproj_thresh px survive (filter_landmarks).
 * Outputs: d_R_out / d_t_out (post-BA i2Ri1, unit i2ti1; the inputs when BA did not produce a pose),
 * d_out_mask[n_pairs][mcap] (post-BA verified rows; the input mask when BA did not run), d_n_out (its count),
 * d_status_out (0 BA ok, 1 no track triangulated, 2 no track valid after BA, 3 not run), d_iters (LM iterations,
 * may be NULL).
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_ba2_workspace_bytes(int n_pairs, int mcap);

int gtsfm_ba2_batched(const float* d_kp_xy, const double* d_intrinsics, int n_img, int kmax, const int* d_pairs,
                      int n_pairs, const uint32_t* d_match_idx, const int* d_match_count, int mcap,
                      const uint8_t* d_in_mask, const double* d_R_in, const double* d_t_in, const int* d_status_in,
                      const double* d_prior_Rt, const double* d_prior_sigmas, int min_inliers, int max_iters,
                      double reproj_thresh, double tri_thresh, void* d_workspace,
                      size_t workspace_bytes, double* d_R_out, double* d_t_out, uint8_t* d_out_mask, int* d_n_out,
                      int* d_status_out, int* d_iters, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Verified-correspondence compaction + inlier-support filter (the device half of the hand-off to the host).
 * d_n_inliers are the rows of d_inlier_mask each pair keeps (the verifier's counts, or gtsfm_ba2_batched's post-BA
 * counts with its mask); inlier_ratio = d_n_inliers / d_match_count unless d_ratio_inliers (may be NULL) gives the
 * count the ratio is taken on (the reference keeps the pre-BA ratio after BA: two_view_estimator.py:326-327).
 * Replaces, for every pair at once: v_corr_idxs = match_indices[mask == 1] and inlier_ratio = mean(mask)
 * (gtsfm/frontend/verifier/opencv_verifier_base.py:98-101) and InlierSupportProcessor.run_inlier_support
 * (gtsfm/frontend/inlier_support_processor.py:73-87: fail iff ratio < min_inlier_ratio or 0 < n < min_inliers).
 * Inputs are the matcher's d_match_idx[n_pairs][mcap][2] / d_match_count and the verifier's mask, status and inlier
 * counts. Outputs: d_offsets[n_pairs + 1] (exclusive scan of the rows each pair contributes: n_inliers when status is
 * 0, else 0), d_v_corr[offsets[p] .. offsets[p+1])[2] uint32 = pair p's inlier putatives in matcher order (rows past
 * `capacity` are not written; capacity = sum of match counts always suffices), d_isp_ok[n_pairs] = 1 iff the pair
 * verified and passes the inlier-support filter.
 * ---------------------------------------------------------------------------------------------- */
int gtsfm_compact_verified(const uint32_t* d_match_idx, const int* d_match_count, int mcap,
                           const uint8_t* d_inlier_mask, const int* d_status, const int* d_n_inliers,
                           const int* d_ratio_inliers, int n_pairs, int min_inliers, double min_inlier_ratio,
                           int* d_offsets, uint32_t* d_v_corr, int capacity, uint8_t* d_isp_ok, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Squared Sampson distances. Replaces gtsfm/utils/verification.py:170-214 compute_epipolar_distances_sq_sampson (the
 * two-view report's ground-truth correspondence metric, gtsfm/utils/metrics.py:99-128), batched over pairs:
 * row r (of n_rows) pairs d_x1[r] (x, y) with d_x2[r] under matrix d_F[d_row_pair[r]] (row-major 3x3, n_mats of them):
 *   d_out[r] = (x2^T F x1)^2 / ((F x1)_x^2 + (F x1)_y^2 + (F^T x2)_x^2 + (F^T x2)_y^2).
 * precision GTSFM_SAMPSON_F64: float64 (the reference's numpy arithmetic). GTSFM_SAMPSON_F32_VERIFIER: the fp32 FMA
 * expression the essential-matrix RANSAC thresholds (its inlier test is d_out <= thr^2), for pinning the verifier.
 * ---------------------------------------------------------------------------------------------- */
#define GTSFM_SAMPSON_F64 0
#define GTSFM_SAMPSON_F32_VERIFIER 1

int gtsfm_sampson_sq_batched(const double* d_F, int n_mats, const int* d_row_pair, const double* d_x1,
                             const double* d_x2, int n_rows, int precision, double* d_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Detector-descriptor: SIFT (OpenCV defaults) + top-k by response over a batch of same-sized images.
 *
 * d_images[n_img][H][W][channels] uint8, channels 1 (gray) or 3 (RGB, converted like cv.COLOR_RGB2GRAY).
 * d_masks[n_img][H][W] uint8 or NULL: as detectAndCompute(gray, image.mask) (reference sift.py:47), a keypoint is
 * dropped when its pixel mask[(int)(y + 0.5)][(int)(x + 0.5)] is 0, before the top-k.
 * Outputs per image, rows 0..count-1 valid, ordered by descending response:
 *   d_xy[n_img][max_kpts][2]   keypoint (x, y) in pixels (x right, y down, origin top-left corner)
 *   d_attr[n_img][max_kpts][3] (size, angle in degrees, response) as cv.KeyPoint
 *   d_desc[n_img][max_kpts][128] float32 descriptors with integer values in [0, 255]
 *   d_counts[n_img] = min(#keypoints, max_kpts); d_n_detected[n_img] (may be NULL) = #keypoints before top-k
 *   (after the mask).
 * Limits: 16 <= H, W < 4096, max_kpts <= 8192.
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_sift_workspace_bytes(int n_img, int H, int W, int max_kpts);

int gtsfm_sift_batched(const uint8_t* d_images, const uint8_t* d_masks, int n_img, int H, int W, int channels,
                       int max_kpts, void* d_workspace, size_t workspace_bytes, float* d_xy, float* d_attr, float* d_desc,
                       int* d_counts, int* d_n_detected, void* stream);

/* ----------------------------------------------------------------------------------------------
 * SuperPoint detector-descriptor. Replaces SuperPointDetectorDescriptor.detect_and_describe
 * (gtsfm/frontend/detector_descriptor/superpoint.py:48-74) and the network it wraps
 * (thirdparty/SuperGluePretrainedNetwork/models/superpoint.py:145-202), batched over n same-sized images
 * d_images[n][H][W][C] (C = 1 gray or 3 RGB -> cv COLOR_RGB2GRAY fixed point), scaled by 1/255.
 * d_weights: packed fp32 blob of gtsfm_superpoint_weights_floats() floats, layers in the order
 *   conv1a, conv1b, conv2a, conv2b, conv3a, conv3b, conv4a, conv4b, [convPa | convDa], convPb, convDb
 * each as W[k*k][cin][cout_pad] (W[ky*k+kx][ci][co] = torch weight[co][ci][ky][kx]) followed by bias[cout_pad];
 * (k, cin, cout_pad) = (3,1,64) (3,64,64) (3,64,64) (3,64,64) (3,64,128) (3,128,128) (3,128,128) (3,128,128)
 * (3,128,512: Pa in 0..255, Da in 256..511) (1,256,128: 65 used) (1,256,256); padded outputs are zero.
 * Detection: softmax over 65, 8x8 depth-to-space, simple_nms(nms_radius), score > keypoint_threshold, border
 * remove_borders; d_masks[n][H][W] u8 or NULL: as Keypoints.filter_by_mask (reference superpoint.py:68-70), a
 * detection at pixel (x, y) is kept iff mask[y][x] == 1, before the top-k; the max_kpts highest scores are kept
 * (ties by raster order) and emitted in raster order (the reference's own order when max_kpts >= detections).
 * Outputs: d_xy[n][max_kpts][2] (x, y) float, d_scores[n][max_kpts], d_desc[n][max_kpts][256] unit-norm,
 * d_count[n], d_n_detected[n] (detections after border and mask, before the top-k; may be NULL).
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_superpoint_weights_floats(void);

size_t gtsfm_superpoint_workspace_bytes(int n, int H, int W, int max_kpts);

int gtsfm_superpoint_batched(const uint8_t* d_images, const uint8_t* d_masks, int n, int H, int W, int C,
                             const float* d_weights, int max_kpts, float keypoint_threshold, int nms_radius,
                             int remove_borders, void* d_workspace, size_t workspace_bytes, float* d_xy,
                             float* d_scores, float* d_desc, int* d_count, int* d_n_detected, void* stream);

/* ----------------------------------------------------------------------------------------------
 * D2-Net detector-descriptor. Replaces D2NetDetDesc.detect_and_describe
 * (gtsfm/frontend/detector_descriptor/d2net.py:47-88, USE_MULTISCALE False) after its resize_image, and what it runs:
 * preprocess_image 'torch' (thirdparty/d2net/lib/utils.py:34-38), process_multiscale with scales = [1]
 * (thirdparty/d2net/lib/pyramid.py:16-146), DenseFeatureExtractionModule, HardDetectionModule and
 * HandcraftedLocalizationModule (thirdparty/d2net/lib/model_test.py:12-200), interpolate_dense_features and
 * upscale_positions (utils.py:77-80, 89-164). GTSFM_HIP_ABI_VERSION stays 407: new symbols only.
 * Batched over n_img same-sized images d_images[n_img][H][W][C] u8, C = 3 RGB or 1 (the gray value in all three
 * channels, as resize_image repeats it); H, W >= 12 (a smaller image gives a map below 2 x 2: GTSFM_ERR_ARG).
 * Network: x = ((u / 255) - mean) / std with mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225); conv3x3 3->64,
 * 64->64, max-pool 2/2 (floor), 64->128, 128->128, max-pool 2/2, 128->256, 256->256, 256->256, average pool 2x2 stride
 * 1, then conv3x3 with padding 2 and dilation 2: 256->512, 512->512, 512->512; ReLU after every convolution. The map F
 * is (512, h, w), h = (H / 2) / 2 - 1, w likewise (integer divisions).
 * d_weights: gtsfm_d2net_weights_floats() floats, per convolution l = 0..9 (state_dict keys
 * dense_feature_extraction.model.{0,2,5,7,10,12,14,17,19,21}): W[9][cin][cout] (W[ky*3+kx][ci][co] = torch
 * weight[co][ci][ky][kx]) then bias[cout].
 * Detection: element (c, i, j) is a candidate iff F[c,i,j] equals the maximum over the 512 channels at (i, j) (every
 * channel of an exact tie is tested) and the maximum of its 3x3 neighbourhood in channel c (out-of-map neighbours
 * ignored), and with dii = F[i-1] - 2 F[i] + F[i+1], djj likewise along j, dij = 0.25 (F[i-1,j-1] - F[i-1,j+1] -
 * F[i+1,j-1] + F[i+1,j+1]) (out-of-map neighbours 0), det = dii djj - dij^2, tr = dii + djj: det > 0 and tr^2 / det <=
 * 7.2; and with di = 0.5 (F[i+1] - F[i-1]), dj likewise, step_i = -(djj di - dij dj) / det, step_j = -(-dij di + dii
 * dj) / det: |step_i| < 0.5, |step_j| < 0.5, and p = (i + step_i, j + step_j) has floor(p) >= 0, ceil(p_i) < h,
 * ceil(p_j) < w. Its score is F[c,i,j]. Candidates are listed in torch.nonzero's order (c, then i, then j); the list
 * holds h w per image (more would take exact ties of the channel maximum at a location; d_n_candidates still counts
 * them, the list drops those last in (i, j, c) order). The max_keypoints highest scores are kept in descending score.
 * Deviation: equal scores are ordered by position in the candidate list (the reference's np.argsort(-scores) is not
 * stable and leaves that order open). Descriptor: bilinear interpolation of the 512 channels at p (weights (1-a)(1-b),
 * (1-a) b, a (1-b), a b, a = p_i - floor(p_i), b = p_j - floor(p_j), corners floor/floor, floor/ceil, ceil/floor,
 * ceil/ceil), then x / max(||x||, 1e-12). Coordinates: ((p * 2 + 0.5) * 2 + 0.5) times fact_i (rows) and fact_j
 * (columns), the ratios of the original to the resized shape (1 without a resize), written (x, y) = (column, row).
 * Outputs: d_xy[n_img][max_keypoints][2], d_score[n_img][max_keypoints], d_desc[n_img][max_keypoints][512],
 * d_count[n_img]; rows past the count are zeroed. d_n_candidates[n_img] (may be NULL): candidates before the top-k.
 * d_dense_map (NULL in the product path): F as [n_img][h][w][512], for tests. The call allocates nothing and does not
 * synchronise; two calls on the same input give the same bytes. fp32-accurate arithmetic (convolutions as split-bf16
 * MFMA products): parity with the reference is a tolerance on F and exact wherever fp32 cannot flip a test.
 * gtsfm_d2net_workspace_bytes is 0 for a shape the call does not take.
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_d2net_weights_floats(void);

size_t gtsfm_d2net_workspace_bytes(int n_img, int H, int W, int max_keypoints);

int gtsfm_d2net_batched(const uint8_t* d_images, int n_img, int H, int W, int C, const float* d_weights,
                        int max_keypoints, float fact_i, float fact_j, void* d_workspace, size_t workspace_bytes,
                        float* d_xy, float* d_score, float* d_desc, int* d_count, int* d_n_candidates,
                        float* d_dense_map, void* stream);

/* Measurement hook (tools/d2net_bench.py): gtsfm_d2net_batched stopped after stage last_stage, so that a stage's time
 * is the difference of two calls. Outputs of the stages not run are left untouched. */
#define GTSFM_D2NET_STAGE_TRUNK 0    /* preprocessing, conv1_1 .. conv3_3, average pool */
#define GTSFM_D2NET_STAGE_DILATED 1  /* + the three dilated convolutions (d_dense_map) */
#define GTSFM_D2NET_STAGE_DETECT 2   /* + detection, candidate list, top-k (d_xy, d_score, d_count, d_n_candidates) */
#define GTSFM_D2NET_STAGE_DESCRIBE 3 /* + descriptors: the whole call */
int gtsfm_d2net_stages(const uint8_t* d_images, int n_img, int H, int W, int C, const float* d_weights,
                       int max_keypoints, float fact_i, float fact_j, void* d_workspace, size_t workspace_bytes,
                       float* d_xy, float* d_score, float* d_desc, int* d_count, int* d_n_candidates,
                       float* d_dense_map, int last_stage, void* stream);

/* ----------------------------------------------------------------------------------------------
 * SuperGlue matcher. Replaces SuperGlueMatcher.match (gtsfm/frontend/matcher/superglue_matcher.py:43-111) and
 * the network it wraps (thirdparty/SuperGluePretrainedNetwork/models/superglue.py:228-283), batched over pairs.
 * Features of all images: d_kp[n_img][kmax][2] (x, y) float, d_scores[n_img][kmax], d_desc[n_img][kmax][256],
 * d_counts[n_img], d_image_hw[n_img][2] = (H, W); kmax a multiple of 64. Pairs d_pairs[n_pairs][2] (both sides
 * must hold >= 1 keypoint: the reference returns no matches for an empty side before running the network).
 * d_weights: gtsfm_superglue_weights_floats(n_layers) floats (layout in superglue.hip: W^T[cin][cout] per 1x1 conv,
 * eval BatchNorm folded to scale/shift, q/k/v/merge weights permuted head-major). GNN layer l is 'self' for even l,
 * 'cross' for odd l. Outputs: matches (i, j) with i ascending in d_out_idx[n_pairs][kmax][2] uint32, counts
 * d_out_count[n_pairs], and the matching scores of image-0 keypoints d_out_mscores[n_pairs][kmax] (may be NULL).
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_superglue_weights_floats(int n_layers);

size_t gtsfm_superglue_workspace_bytes(int n_pairs, int kmax);

int gtsfm_superglue_batched(const float* d_kp, const float* d_scores, const float* d_desc, const int* d_counts,
                            const int* d_image_hw, int n_img, int kmax, const int* d_pairs, int n_pairs,
                            const float* d_weights, int n_layers, int sinkhorn_iters, float match_threshold,
                            void* d_workspace, size_t workspace_bytes, uint32_t* d_out_idx, int* d_out_count,
                            float* d_out_mscores, void* stream);

/* Inspection hook (the reference keeps this matrix internal: superglue.py:261-263 `scores`): after a
 * gtsfm_superglue_batched call, writes pair `pair`'s final log-assignment matrix (log_optimal_transport's output, the
 * Sinkhorn result + the normalisation) from that call's workspace into d_out[(kmax + 1)][(kmax + 1)]: rows 0..m,
 * columns 0..n (the last of each being the dustbin), NaN elsewhere. Same n_pairs / kmax as the call. */
int gtsfm_superglue_log_assignment(const void* d_workspace, size_t workspace_bytes, int n_pairs, int kmax, int pair,
                                   float* d_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * LightGlue matcher at SuperPoint's width. Replaces LightGlueMatcher.match
 * (gtsfm/frontend/matcher/lightglue_matcher.py:24-93) and the network it wraps, batched over pairs: d = 256, 4 heads
 * of 64, n_layers (9) layers of one self block (rotary position encoding) and one cross block (shared projection,
 * both directions), LayerNorm + GELU feed-forward, adaptive depth, double-softmax assignment with matchability.
 * Point pruning (width_confidence) is not built: the result is the never-pruned one. Parity with the authors' code
 * and the published checkpoint is unpinned (neither is part of the reference checkout): the arithmetic is the
 * restatement in DESIGN.md.
 * Features of all images: d_kp[n_img][kmax][2] (x, y) float, d_desc[n_img][kmax][256], d_counts[n_img],
 * d_image_hw[n_img][2] = (H, W); kmax a multiple of 64. Pairs d_pairs[n_pairs][2]; a pair with an empty side gives no
 * matches without running the network. d_weights: gtsfm_lightglue_weights_floats(n_layers) floats (layout in
 * lightglue.hip: W^T[cin][cout] per Linear, the interleaved Wqkv permuted to [q | k | v] head-major).
 * depth_confidence <= 0 disables stopping (every pair runs n_layers layers). Outputs: matches (i, j) with i
 * ascending in d_out_idx[n_pairs][kmax][2] uint32, counts d_out_count[n_pairs], the matching scores of image-0
 * keypoints d_out_mscores[n_pairs][kmax] (may be NULL), and the layer each pair left the network at,
 * d_out_exit_layer[n_pairs] (may be NULL; n_layers - 1 for a pair that never stopped). Argument errors return
 * GTSFM_ERR_ARG. The call allocates nothing and does not synchronise.
 * ---------------------------------------------------------------------------------------------- */
size_t gtsfm_lightglue_weights_floats(int n_layers);

/* lightglue_matcher.py:24-93: bytes of device workspace for one call over n_pairs pairs (0 for an empty shape). */
size_t gtsfm_lightglue_workspace_bytes(int n_pairs, int kmax);

/* lightglue_matcher.py:24-93: the batched match call described above. */
int gtsfm_lightglue_batched(const float* d_kp, const float* d_desc, const int* d_counts, const int* d_image_hw,
                            int n_img, int kmax, const int* d_pairs, int n_pairs, const float* d_weights, int n_layers,
                            float depth_confidence, float filter_threshold, void* d_workspace, size_t workspace_bytes,
                            uint32_t* d_out_idx, int* d_out_count, float* d_out_mscores, int* d_out_exit_layer,
                            void* stream);

/* Inspection hook (lightglue_matcher.py:24-93 keeps only the matches): after a gtsfm_lightglue_batched call, writes
 * pair `pair`'s log-assignment matrix from that call's workspace into d_out[(kmax + 1)][(kmax + 1)]: rows 0..m,
 * columns 0..n (the last of each being the dustbin), NaN elsewhere. Same n_pairs / kmax as the call. */
int gtsfm_lightglue_log_assignment(const void* d_workspace, size_t workspace_bytes, int n_pairs, int kmax, int pair,
                                   float* d_out, void* stream);

/* ---- Retrieval (f3): NetVLAD global-descriptor similarity + top-k image pairs ---------------------------------- */

/* Replaces NetVLADRetriever.compute_similarity_matrix (gtsfm/retriever/netvlad_retriever.py:77-107) together with
 * _compute_similarity_subblock (:109-134, the einsum "id,jd->ij" per block pair block_j >= block_i) and
 * _aggregate_subblocks (:136-149). d_desc: [n_img][dim] f32 global descriptors; d_sim: [n_img][n_img] f32, fully
 * written: the dot product where block(j) >= block(i) (block = index / blocksize), 0 elsewhere, as the reference's
 * zero-initialised aggregate. fp32 accumulation (summation order differs from torch: parity is a tolerance). */
int gtsfm_retrieval_similarity(const float* d_desc, int n_img, int dim, int blocksize, float* d_sim, void* stream);

/* Replaces pairs_from_score_matrix (netvlad_retriever.py:196-228). d_scores: [n_rows][n_cols] f32. d_invalid:
 * [n_rows][n_cols] u8 (nonzero = invalid), or NULL for compute_pairs_from_similarity_matrix's mask (:164-167: every
 * entry not strictly above the diagonal is invalid). k = min(num_select, n_rows) (:213-215; k > n_cols is
 * GTSFM_ERR_ARG, as torch.topk raises); scores < min_score are invalid when use_min_score != 0. For row i,
 * d_out_pairs[(i * k + r) * 2 + {0,1}] = (i, j_r) for r < d_row_count[i]: the finite entries of torch.topk(row, k) in
 * rank order (NaN ranks first and takes a slot but is not emitted; equal scores by ascending column, an order torch
 * leaves unspecified). The reference's pair list is the rows concatenated in order. d_scores is read only (the
 * reference masks its argument in place). */
int gtsfm_retrieval_pairs(const float* d_scores, int n_rows, int n_cols, const unsigned char* d_invalid, int num_select,
                          float min_score, int use_min_score, int* d_out_pairs, int* d_row_count, void* stream);

/* ---- Global descriptor (f3): NetVLAD ---------------------------------------------------------------------------- */

/* Replaces NetVLADGlobalDescriptor.describe (gtsfm/frontend/global_descriptor/netvlad_global_descriptor.py:27-46)
 * and the network it runs (thirdparty/hloc/netvlad.py:160-191), batched over n same-sized RGB images
 * d_images[n][H][W][3] u8 (describe()'s image.value_array). Per image: x = clamp(u / 255 * 255, 0, 255) - mean,
 * VGG16 features[:-2] (13 conv3x3 + ReLU except the last, 2x2 max-pools after convs 2, 4, 7, 10, floor), per-location
 * L2 pre-normalisation, NetVLADLayer (K = 64 clusters, D = 512: softmax(score_proj x), residual sums, intra-norm,
 * d-major flatten, L2), then (whiten != 0) the 32768 -> 4096 whitening Linear and L2.
 * d_weights: gtsfm_netvlad_weights_floats() floats:
 *   mean[4] (averageImage RGB, 1 pad); per conv l = 0..12: W[9][cin][cout] (W[ky*3+kx][ci][co] = torch
 *   backbone weight[co][ci][ky][kx]) then bias[cout], (cin, cout) = (3,64) (64,64) (64,128) (128,128) (128,256)
 *   (256,256) (256,256) (256,512) (512,512) x 5; score_proj[64][512]; centers[512][64]; whiten W[4096][32768]
 *   (nn.Linear's weight, row = output); whiten b[4096].
 * Outputs: d_vlad[n][32768] (may be NULL when whiten != 0) and d_desc[n][4096] (whiten != 0). fp32-accurate
 * arithmetic (convolutions as split-bf16 MFMA products, the rest fp32): parity with the reference is a tolerance. */
size_t gtsfm_netvlad_weights_floats(void);

size_t gtsfm_netvlad_workspace_bytes(int n, int H, int W);

int gtsfm_netvlad_batched(const uint8_t* d_images, int n, int H, int W, int C, const float* d_weights, int whiten,
                          float* d_vlad, float* d_desc, void* d_workspace, size_t workspace_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * View graph: cycle-consistent rotation filter. Replaces CycleConsistentRotationViewGraphEstimator.run
 * (gtsfm/view_graph_estimator/cycle_consistent_rotation_estimator.py:78-152), with the triplet extraction
 * (gtsfm/utils/graph.py:100-135) and the cycle error (gtsfm/utils/geometry_comparisons.py:355-370) it calls.
 * Edges d_edges[n_edges][2] = (i1, i2) image indices with i1 < i2 < n_img, each pair at most once, in any order (sorted
 * by (i1, i2), as the front-end emits them, is the cache-friendly order); d_R[n_edges][9] row-major i2Ri1;
 * d_valid[n_edges] (0 = the edge is absent from the graph: it is no adjacency and gets no result) or NULL (all valid).
 * An edge whose indices are out of range or not ordered is treated as invalid.
 * A triplet is three images i0 < i1 < i2 whose three edges are all valid. Its cycle error is the rotation angle in
 * degrees of M = R(i0,i2)^T R(i1,i2) R(i0,i1), computed in fp64 as
 *   atan2(|(M32 - M23, M13 - M31, M21 - M12)| / 2, (tr M - 1) / 2)
 * (equal to the reference's scipy as_rotvec norm to 1e-13 degrees, and well-conditioned near 0, where acos is not).
 * Per edge, over every triplet that contains it: d_n_triplets = their number, d_agg_error_deg = np.amin
 * (GTSFM_VG_MIN_EDGE_ERROR) or np.median (GTSFM_VG_MEDIAN_EDGE_ERROR; exact, an even count gives the mean of the two
 * middle values) of their cycle errors, NaN when one of them is NaN, and NaN when the edge is invalid or in no triplet;
 * d_keep = 1 iff n_triplets > 0 and the aggregate < error_threshold_deg (the reference's ERROR_THRESHOLD is 7.0).
 * d_total_triplets[0] (may be NULL) = the number of distinct triplets. Results are bit-identical from run to run.
 * n_img <= 8192 (the workspace holds a dense n_img x n_img edge lookup: 4 n_img^2 + n_img^2 / 8 bytes; an edge may
 * have up to n_img - 2 triplets and all of them are aggregated): GTSFM_ERR_ARG above it, and for a negative size, an
 * unknown criterion or a workspace smaller than the query's answer. n_edges == 0 returns GTSFM_OK and launches nothing.
 * ---------------------------------------------------------------------------------------------- */
#define GTSFM_VG_MIN_EDGE_ERROR 0
#define GTSFM_VG_MEDIAN_EDGE_ERROR 1

/* 0 when n_edges == 0 (or the shape is unsupported). */
size_t gtsfm_viewgraph_workspace_bytes(int n_img, int n_edges);

int gtsfm_viewgraph_cycle_filter(const int* d_edges, const double* d_R, const uint8_t* d_valid, int n_img, int n_edges,
                                 int criterion, double error_threshold_deg, void* d_workspace, size_t workspace_bytes,
                                 double* d_agg_error_deg, int* d_n_triplets, uint8_t* d_keep,
                                 unsigned long long* d_total_triplets, void* stream);

/* ----------------------------------------------------------------------------------------------
 * 2D feature tracks from verified correspondences (disjoint-set forest). Replaces DsfTracksEstimator.run
 * (gtsfm/data_association/dsf_tracks_estimator.py:56-85: one dsf.merge per correspondence row, dsf.sets(), and the
 * unique-camera filter of gtsfm/common/sfm_track.py:105-112) and CppDsfTracksEstimator.run
 * (cpp_dsf_tracks_estimator.py:63-74), the step get_2d_tracks (gtsfm/multi_view_optimizer.py:195-199) runs on the
 * view graph's correspondences.
 * Inputs: d_pairs[n_pairs][2] = (i1, i2) image indices in any order, i1 == i2 and repeated pairs allowed;
 * d_offsets[n_pairs + 1] and d_v_corr[..][2] = (k1, k2) uint32, the CSR gtsfm_compact_verified writes (pair p owns rows
 * offsets[p] .. offsets[p + 1]); n_rows = the rows of d_v_corr that may be read, at least offsets[n_pairs] (the
 * `capacity` given to gtsfm_compact_verified will do: the row count itself stays on the device; rows from n_rows on
 * are never read); d_valid[n_pairs] (0 = skip the pair's rows; keep & isp_ok goes here) or NULL (all valid);
 * d_kp_count[n_img] and kmax, the [n_img][kmax] keypoint layout of the verifier; d_kp_xy[n_img][kmax][2] or NULL.
 * A node is (image i, keypoint k) with id i * kmax + k, so ascending id is ascending (i, k). n_img * kmax < 2^31 and
 * n_rows < 2^31, else GTSFM_ERR_ARG.
 * Semantics: a node is touched when a row of a valid pair names it; rows merge their two nodes transitively; every
 * connected component of touched nodes is a candidate, and it is a track iff no two of its nodes share an image. A
 * row whose two ends are one node gives a one-measurement track, as the Python reference does. A row of a valid pair
 * whose image index is outside [0, n_img) or whose k >= min(d_kp_count[i], kmax) is ignored and counted.
 * Canonical order (this library's definition; the reference's track order follows gtsam's internal representative
 * and its SfmTrack2d.__eq__ ignores measurement order): tracks by ascending smallest node id, measurements inside a
 * track by ascending node id, the order of gtsam's std::set<IndexPair> and the one test_dsf_tracks_estimator.py:86-112
 * asserts. The outputs depend on the set of rows alone and are byte-identical from launch to launch.
 * Outputs (caller-owned): d_track_offsets[track_cap + 1] (track t owns measurements offsets[t] .. offsets[t + 1]),
 * d_track_img / d_track_kp[meas_cap], d_track_uv[meas_cap][2] = d_kp_xy of the node (written only when d_kp_xy and
 * d_track_uv are both non-NULL), d_stats[5] = { n_tracks, n_measurements, n_components (the reference's len(key_set)),
 * n_erroneous (components dropped for a repeated image), n_bad_rows }.
 * Capacities: touched nodes <= min(2 * rows, n_img * kmax) bounds n_tracks and n_measurements, so that value always
 * suffices for both. When a capacity is short nothing is written past it (measurement entries from meas_cap on and
 * offsets entries after track_cap are dropped; the offsets that are written hold their true values) and d_stats still
 * carries the true counts, as `capacity` does for gtsfm_compact_verified.
 * Workspace: 30 bytes per node (n_img * kmax) plus the scans' tile sums; the query is constant in n_pairs and n_rows.
 * n_pairs == 0 or n_rows == 0 returns GTSFM_OK with zeroed stats and offsets[0] = 0 and launches no kernel. A negative
 * size, a NULL required pointer or a short workspace returns GTSFM_ERR_ARG. Nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
/* 0 for an empty shape (a size <= 0) or an unsupported one (n_img * kmax or n_rows >= 2^31). */
size_t gtsfm_tracks_workspace_bytes(int n_img, int kmax, int n_pairs, long long n_rows);

int gtsfm_tracks_from_matches(const int* d_pairs, const int* d_offsets, const uint32_t* d_v_corr,
                              const uint8_t* d_valid, int n_pairs, long long n_rows, const int* d_kp_count,
                              const float* d_kp_xy, int n_img, int kmax, void* d_workspace, size_t workspace_bytes,
                              int* d_track_offsets, long long track_cap, int* d_track_img, int* d_track_kp,
                              float* d_track_uv, long long meas_cap, long long* d_stats, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Triangulation of 2D tracks to 3D landmarks: gtsfm/data_association/point3d_initializer.py:117-380
 * Point3dInitializer.triangulate for every track of a CSR in one call (the reference makes one Python call per track,
 * data_assoc.py:211-273, each with up to num_ransac_hypotheses gtsam.triangulatePoint3 calls).
 *
 * Tracks: d_track_offsets[n_tracks + 1] int32 and d_track_img[n_meas] int32 exactly as gtsfm_tracks_from_matches
 * writes them; d_track_uv[n_meas][2] is that call's float32 track_uv (uv_is_f64 = 0) or a double array (uv_is_f64 = 1;
 * SfmMeasurement.uv is float64). n_tracks is the number of tracks or, with d_n_tracks non-NULL, a capacity: the
 * kernels then use min(n_tracks, d_n_tracks[0]) read on the device (pass the d_stats of gtsfm_tracks_from_matches: its
 * entry 0 is the track count), so the chain needs no host synchronisation. n_meas bounds every offset; a track whose
 * range is not inside [0, n_meas] gets exit code 2 and nothing else. d_track_id[n_tracks] (or NULL = the track's
 * index) is the id the sampling hash is keyed by, so that a reordered set of tracks draws the same hypotheses.
 * Cameras, indexed by image: d_wRc[n_img][9] row-major, d_wtc[n_img][3], d_intrinsics[n_img][3] = (f, u0, v0), all
 * double, and d_cam_valid[n_img] (0 = the reference's camera missing from track_camera_dict or None) or NULL (all
 * valid). An image index outside [0, n_img) counts as an invalid camera.
 *
 * Per-track semantics (point3d_initializer.py:225-295). err(measurement, X) is NaN for an invalid camera or z <= 0
 * in the camera frame (projectSafe), else the pixel distance (reprojection.py:48-83); inlier iff err < threshold.
 * triangulate(S) is gtsam.triangulatePoint3(rank_tol 1e-9, optimize): DLT null vector of the 2|S| x 4 system (folded
 * row by row into a 4 x 4 triangular factor by Givens rotations, then one-sided Jacobi; rank >= 3), LM on the unit-noise
 * reprojection factors (lambda 1, factor 10, <= 100 iterations, absoluteErrorTol 1), and it fails on rank < 3 or z <= 0
 * in a camera of S.
 * mode GTSFM_TRI_NO_RANSAC: best_inliers = all. Else the hypotheses are the pairs (k1 < k2) of the track's n
 * measurements, pair index j in itertools.combinations order; m = min(n_hyp, n (n - 1) / 2) of them are evaluated: all
 * of them when m equals their number, otherwise the m with the smallest (key_j, j), where
 *   GTSFM_TRI_RANSAC_SAMPLE_UNIFORM: key_j = mix(mix(seed ^ mix(track id)) + j), mix = the splitmix64 finaliser
 *       (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *       z ^ z >> 31) -- a fixed pseudo-random subset instead of the reference's np.random.choice(replace=False);
 *   GTSFM_TRI_RANSAC_TOPK_BASELINES: key_j = ~bits(|wtc_i1 - wtc_i2|^2), the three fp64 products summed left to
 *       right, so descending squared baseline (the reference's argsort of the norm, ties there unordered); a pair with
 *       an invalid camera has key ~0;
 *   GTSFM_TRI_RANSAC_SAMPLE_BIASED_BASELINE is not built: GTSFM_ERR_ARG.
 * A hypothesis with an invalid camera or a failed two-view triangulate is skipped; else votes = inliers among all n
 * measurements and avg_err their mean inlier error; votes == 0 does not compete. The winner is the minimum of
 * (-votes, avg_err, j) (the reference keeps the first of equals in its random sample order); best_inliers is its
 * inlier mask, all zero when nothing competes.
 * Exit codes (TriangulationExitCode), in this order: < 2 inliers: 2; < 2 inliers with a valid camera: 3;
 * triangulate(inliers with a valid camera) fails: 1; some inlier's err not < threshold (NaN included): 4;
 * min_triangulation_angle > 0 and the largest angle (degrees) at the point between the rays to two inliers' camera
 * centres is below it: 5; else 0.
 * Outputs (caller-owned): d_exit_code[n_tracks] int32; d_point[n_tracks][3], written when the final triangulate
 * succeeded (exits 0, 4, 5); d_avg_err[n_tracks] = nanmean of the inliers' errors for exits 0, 4, 5, NaN for 1-3;
 * d_inlier[n_meas] = best_inliers, parallel to d_track_img; d_stats[8] int64 = the six exit-code counts, the inlier
 * measurements of exit-0 tracks, the hypotheses evaluated (sum of m). Optional, for inspection: d_track_n_hyp[n_tracks]
 * = m per track; d_hyp_pair[hyp_cap] = the pair index j of every evaluated hypothesis, track by track, ascending j
 * inside a track (entries from hyp_cap on are dropped). Either may be NULL.
 * All outputs are functions of a track's own measurements, cameras and id: they do not depend on the other tracks, on
 * the workspace size or on the launch, and are byte-identical from call to call. No floating-point atomics.
 * Workspace: 8 bytes per track plus a hypothesis buffer of 20 bytes per (track, hypothesis) item. The tracks are
 * processed in chunks whose items fit the buffer; the query asks for all items up to 64 MiB, and at least one track's
 * worst case min(n_hyp, n_meas (n_meas - 1) / 2) items. A smaller workspace that still holds that worst case gives
 * more chunks and the same result; one that does not returns GTSFM_ERR_CAPACITY.
 * n_tracks == 0 returns GTSFM_OK with zeroed stats. A negative size, a NULL required pointer, a threshold that is
 * not > 0, n_hyp == 0 with a RANSAC mode or an unknown mode returns GTSFM_ERR_ARG. Nothing allocates or synchronises.
 * ---------------------------------------------------------------------------------------------- */
#define GTSFM_TRI_NO_RANSAC 0
#define GTSFM_TRI_RANSAC_SAMPLE_UNIFORM 1
#define GTSFM_TRI_RANSAC_SAMPLE_BIASED_BASELINE 2
#define GTSFM_TRI_RANSAC_TOPK_BASELINES 3
/* 0 for an empty shape (n_tracks or n_meas <= 0), n_hyp < 0 or a size >= 2^31. */
size_t gtsfm_triangulate_workspace_bytes(long long n_tracks, long long n_meas, int n_hyp);

int gtsfm_triangulate_tracks(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                             const int* d_track_id, long long n_tracks, const long long* d_n_tracks, long long n_meas,
                             const double* d_wRc, const double* d_wtc, const double* d_intrinsics,
                             const uint8_t* d_cam_valid, int n_img, int mode, double reproj_error_threshold,
                             double min_triangulation_angle, int n_hyp, uint64_t seed, void* d_workspace,
                             size_t workspace_bytes, int* d_exit_code, double* d_point, double* d_avg_err,
                             uint8_t* d_inlier, long long* d_stats, int* d_track_n_hyp, long long* d_hyp_pair,
                             long long hyp_cap, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Global bundle adjustment: gtsfm/bundle/bundle_adjustment.py:58-397 BundleAdjustmentOptimizer
 * (run_ba_stage_with_filtering :292-357, the factor graph :106-267, run_ba :359-397), gtsfm/bundle/global_ba.py and
 * gtsfm/common/gtsfm_data.py:389-427 filter_landmarks: one GTSAM LevenbergMarquardtOptimizer over every camera pose and
 * every landmark, the consumer of gtsfm_triangulate_tracks' device tensors.
 *
 * Inputs, laid out as the two upstream calls write them: the track CSR d_track_offsets[n_tracks + 1], d_track_img[n_meas],
 * d_track_uv[n_meas][2] (float32, or double with uv_is_f64 = 1); n_tracks is the track count or, with d_n_tracks
 * non-NULL, a capacity (min(n_tracks, d_n_tracks[0]) is used, read on the device); d_point[n_tracks][3] the initial
 * landmarks; d_track_valid[n_tracks], a byte per track (the `valid` of DataAssociation.run_triangulation_arrays) or NULL
 * (all); d_meas_valid[n_meas] (the triangulation's inlier bytes) or NULL (all): a measurement with 0 is not a factor and
 * is not checked by the filter, as the reference's SfmTrack holds inliers only. Cameras indexed by image: d_wRc[n_img][9]
 * row-major, d_wtc[n_img][3], d_intrinsics[n_img][3] = (f, u0, v0), d_cam_valid[n_img] or NULL (all valid); an image
 * index outside [0, n_img) counts as an invalid camera.
 * Options: robust (Huber 1.345 on the whitened residual norm), measurement_sigma (pixels), cam_pose3_prior_sigma (the
 * reference's default 0.1), max_iterations (0 = GTSAM's 100), pcg_rel_tol (1e-10 is the binding's default),
 * pcg_max_iter (2000), reproj_error_thresh (+inf = the reference's None).
 *
 * The problem. A measurement is usable when its d_meas_valid byte is set and its camera is valid. A track participates
 * when it is valid, its offsets lie inside [0, n_meas] and at least two of its measurements are usable. A camera is
 * modelled when it is valid and has a usable measurement in a participating track. Variables: one Pose3 per modelled
 * camera, one point per participating track. Factors: a reprojection factor per usable measurement of a participating
 * track; PriorFactorPose3 on the modelled camera of lowest index at its initial pose, isotropic
 * cam_pose3_prior_sigma; PriorFactorPoint3, sigma 0.1, on the first participating track at its initial point.
 * This entry point holds calibration fixed at k1 = k2 = 0, the approximation gtsfm_ba2_batched states (the limit of the
 * reference's 1e-5 calibration prior as that sigma goes to 0), so the reference's shared_calib does not enter it;
 * gtsfm_global_ba_calib below is the same solver with the Cal3Bundler calibration refined, per camera or shared.
 * BetweenFactorPose3 relative-pose priors are not built.
 * Taken from gtsfm_ba2_batched (ba2.hip), generalised from camera 0 = identity to an arbitrary first camera: the
 * reprojection residual and its Jacobians (pose in the body frame, rotation first), the Huber loss and sqrt-weight
 * scaling of the rows, a measurement with z <= 0 contributing nothing to the linear system or the cost, the pose prior
 * as Logmap(X0^-1 X) with an identity Jacobian, the point prior, the Pose3 retraction (full exponential map) and the
 * point update p + dp.
 * The optimiser is GTSAM's LM as ba2.hip restates it: lambda 1e-5, factor 10, upper bound 1e5, isotropic damping,
 * minModelFidelity 1e-3, relative and absolute error tolerances 1e-5. Each trial eliminates the points (3 x 3 blocks,
 * damped) and solves the 6C x 6C reduced camera system without forming it, by preconditioned conjugate gradients from
 * a zero start; the preconditioner is the inverse of the 6 x 6 diagonal blocks of the damped Schur complement. PCG
 * stops at ||r||_2 <= pcg_rel_tol ||b||_2 or after pcg_max_iter products (a cap hit is counted; the step then goes
 * through the ordinary accept test). Then the points are back-substituted and the linearised and non-linear costs of
 * the step evaluated. Every sum is taken in a fixed order and there are no floating-point atomics: two calls on the
 * same inputs return byte-identical outputs.
 *
 * Outputs (caller-owned): d_wRc_out[n_img][9], d_wtc_out[n_img][3] (a camera that is not modelled is copied through);
 * d_point_out[n_tracks][3] (non-participating tracks copied through); d_track_keep[n_tracks] bytes, GtsfmData.
 * filter_landmarks: 1 iff the track participates and every measurement whose d_meas_valid byte is set has a valid
 * camera (the reference's error is NaN otherwise), lies in front of it and reprojects with error <
 * reproj_error_thresh; with an infinite threshold every participating track is kept, without the cheirality test
 * (bundle_adjustment.py:353-355); d_cam_keep[n_img] bytes: the camera has such a measurement in a kept track (the
 * cameras of filtered_result); d_stats[10] doubles = { initial error, final error (graph.error), LM iterations, LM
 * trials, PCG iterations in total, PCG cap hits, cameras modelled, tracks participating, tracks kept, status }.
 * Status 0: optimised. Status 1: nothing to optimise (no participating track or no modelled camera, the reference's
 * early return at :319-324): inputs copied through, both keep masks zero, errors and counts 0.
 * The LM and PCG control flow runs on the host: the call enqueues its kernels on `stream` and reads a few scalars back
 * per PCG iteration and per LM trial, so, unlike every other entry point, it SYNCHRONISES its stream (and returns with
 * the stream idle) and cannot be captured into a hipGraph. It still allocates nothing: all state lives in the
 * workspace, 160 bytes per measurement for the linearisation plus about 350 bytes per track and 1 KiB per camera.
 * A negative size, a size >= 2^31 - 1, n_img > 2^20, a NULL required pointer, a sigma, tolerance or threshold that is
 * not > 0, max_iterations < 0 or pcg_max_iter <= 0 returns GTSFM_ERR_ARG; a workspace smaller than the query's answer
 * returns GTSFM_ERR_CAPACITY. n_tracks, n_meas or n_img == 0 gives status 1.
 * ---------------------------------------------------------------------------------------------- */
/* 0 for an empty shape (a size <= 0) or an unsupported one (n_tracks or n_meas >= 2^31 - 1, n_img > 2^20). */
size_t gtsfm_global_ba_workspace_bytes(long long n_tracks, long long n_meas, int n_img);

int gtsfm_global_ba(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                    long long n_tracks, const long long* d_n_tracks, long long n_meas, const double* d_point,
                    const uint8_t* d_track_valid, const uint8_t* d_meas_valid, const double* d_wRc,
                    const double* d_wtc, const double* d_intrinsics, const uint8_t* d_cam_valid, int n_img, int robust,
                    double measurement_sigma, double cam_pose3_prior_sigma, int max_iterations, double pcg_rel_tol,
                    int pcg_max_iter, double reproj_error_thresh, void* d_workspace, size_t workspace_bytes,
                    double* d_wRc_out, double* d_wtc_out, double* d_point_out, uint8_t* d_track_keep,
                    uint8_t* d_cam_keep, double* d_stats, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Global bundle adjustment with the calibration refined: gtsfm/bundle/bundle_adjustment.py:58-66 ("refines global pose
 * estimates and intrinsics of cameras"), :103-131 and :180-208 (a K(i) variable per camera, or a single K(0) when
 * shared_calib = True, in every GeneralSFMFactor2Cal3Bundler, and a PriorFactorCal3Bundler of
 * calibration_prior_noise_sigma on each calibration variable), :188-195 and :258-260 (the shared variable).
 *
 * Everything gtsfm_global_ba's block states holds here, with these differences.
 * Cameras: d_calib[n_img][5] = (f, k1, k2, u0, v0), the argument order of GTSAM 4.2's Cal3Bundler, replaces
 * d_intrinsics. Projection of a camera-frame point pc: x = pc_x / pc_z, y = pc_y / pc_z, r2 = x^2 + y^2,
 * g = 1 + (k1 + k2 r2) r2, u = f g x + u0, v = f g y + v0. d uv / d (x, y) = f (g I + 2 (k1 + 2 k2 r2) [x; y][x y]),
 * chained with the pinhole Jacobians of pose (body frame, rotation first) and point; d uv / d (f, k1, k2) =
 * [[x g, f x r2, f x r2^2], [y g, f y r2, f y r2^2]]. u0 and v0 are not variables (Cal3Bundler::dim() == 3).
 * Calibration variables: with shared_calib = 0 one (f, k1, k2) per modelled camera, with its prior at that camera's
 * input calibration; with shared_calib = 1 a single one, initialised from and with its prior at the calibration of the
 * modelled camera of lowest index, whose u0, v0 are then used for EVERY camera. The prior's residual is
 * (f, k1, k2) - (f, k1, k2)_initial, isotropic calibration_prior_sigma (the reference's default is 1e-5, at which this
 * call returns gtsfm_global_ba's result to rounding on undistorted input); the retraction is (f, k1, k2) + delta.
 * The reduced system has 9 x 9 blocks (pose + calibration) per camera, or, shared, 6 x 6 blocks per camera and one
 * 3 x 3 border block coupled to every camera; the unknown vector is [C][9] or [6C | 3]. The preconditioner is the inverse
 * of the diagonal blocks of the damped Schur complement, the border block included. In shared mode each camera's
 * workgroup writes its share of the border (of its diagonal block and right-hand side, and of the border row of every
 * product q = S p) to a slot of its own, and one workgroup sums the slots in a fixed order. No floating-point atomics:
 * two calls return byte-identical outputs. The filter reprojects with the refined, distorted model.
 *
 * Outputs: gtsfm_global_ba's, plus d_calib_out[n_img][5]: a modelled camera's refined calibration (shared mode: the
 * shared one, the same five values in every modelled camera's row); a camera that is not modelled is copied through
 * bit for bit. d_stats[12]: gtsfm_global_ba's ten slots, then the number of calibration variables and the largest
 * |f_out - f_in| / f_in of a modelled camera. Status codes, argument checks and capacity errors are gtsfm_global_ba's;
 * in addition calibration_prior_sigma not > 0 or shared_calib outside {0, 1} returns GTSFM_ERR_ARG. On status 1 d_calib
 * is copied through and the two new slots are 0.
 * Workspace: 208 bytes per measurement for the linearisation (Jx 2 x 6, Jk 2 x 3, Jp 2 x 3, b 2) plus 8 for the two
 * indices, about 350 bytes per track (as gtsfm_global_ba) and about 2.2 KiB per camera (two 9 x 9 blocks, the poses and
 * calibrations twice, the border slots and six vectors of 9 entries). As gtsfm_global_ba the call SYNCHRONISES its
 * stream and allocates nothing.
 * ---------------------------------------------------------------------------------------------- */
/* 0 for an empty shape (a size <= 0) or an unsupported one (n_tracks or n_meas >= 2^31 - 1, n_img > 2^20). */
size_t gtsfm_global_ba_calib_workspace_bytes(long long n_tracks, long long n_meas, int n_img);

int gtsfm_global_ba_calib(const int* d_track_offsets, const int* d_track_img, const void* d_track_uv, int uv_is_f64,
                          long long n_tracks, const long long* d_n_tracks, long long n_meas, const double* d_point,
                          const uint8_t* d_track_valid, const uint8_t* d_meas_valid, const double* d_wRc,
                          const double* d_wtc, const double* d_calib, const uint8_t* d_cam_valid, int n_img,
                          int robust, double measurement_sigma, double cam_pose3_prior_sigma, int shared_calib,
                          double calibration_prior_sigma, int max_iterations, double pcg_rel_tol, int pcg_max_iter,
                          double reproj_error_thresh, void* d_workspace, size_t workspace_bytes, double* d_wRc_out,
                          double* d_wtc_out, double* d_calib_out, double* d_point_out, uint8_t* d_track_keep,
                          uint8_t* d_cam_keep, double* d_stats, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Translation averaging, 1DSfM: gtsfm/averaging/translation/averaging_1dsfm.py TranslationAveraging1DSFM, in three
 * calls that share one measurement list. The global rotations wRi are an input (gtsfm_rotavg_shonan below computes them).
 *
 * The measurement list. Nodes: camera i is node i, landmark s (the s-th selected track) is node n_img + s. Measurement
 * e has d_meas_key[e] = (key1, key2) int32, a unit direction d_meas_dir[e][3] double and a byte d_meas_valid[e].
 * gtsfm_transavg_measurements writes n_edges + n_meas slots: slot e < n_edges is camera edge e (keys (i2, i1), the
 * flip of _binary_measurements_from_dict :152-153); the track measurements follow from slot n_edges on, selected track
 * by selected track in selection order, a track's measurements in CSR order (keys (camera, n_img + s), :154-155).
 * Unused slots have valid = 0, keys -1 and a zero direction. d_counts[4] int64 = { valid camera edges, track slots in
 * use, selected tracks, track measurements whose camera has no rotation }.
 *
 * gtsfm_transavg_measurements: (a) get_valid_measurements_in_world_frame :593-616 and _get_landmark_directions
 * :341-372, (b) _select_tracks_for_averaging :273-339.
 * (a) Edge e = d_edges[e] = (i1, i2) with d_i2Ui1[e][3] is valid iff d_edge_valid[e] != 0 (NULL = all), both indices
 * lie in [0, n_img), i1 != i2 and d_rot_valid[i2] != 0 (NULL = all). Its direction is Unit3(wRi[i2] i2Ui1): the
 * row-major 3 x 3 product, each row summed left to right, then every component divided by the norm sqrt(x x + y y +
 * z z); a zero vector stays zero. Both endpoints become valid cameras (d_cam_valid[n_img]). A track measurement (u, v)
 * in camera c has direction Unit3(wRi[c] Unit3(((u - u0) / f, (v - v0) / f, 1))), calibration (f, u0, v0) =
 * d_intrinsics[c], k1 = k2 = 0. Where the reference raises (camera c valid but d_rot_valid[c] == 0) the slot stays
 * unused and counts[3] is incremented.
 * (b) Integer only, so exact: a track (d_track_offsets / d_track_img / d_track_uv as gtsfm_triangulate_tracks takes
 * them, n_tracks a capacity when d_n_tracks is given) is restricted to its measurements in valid cameras and dropped
 * when fewer than 3 remain. improvement[t] starts at that count, remaining[c] at measurements_per_camera (the
 * reference's TRACKS_MEASUREMENTS_PER_CAMERA = 12). Repeat: take the track of largest improvement, lowest index first
 * (np.argmax); stop when it is <= 0; append it to d_selected; set its improvement to 0; for each of its measurements
 * in order whose camera c has remaining[c] > 0: decrement remaining[c], and when that reaches 0 lower the improvement
 * of every track by one, not below 0, once per measurement that the track has in c (the reference's camera -> tracks
 * lookup holds one entry per measurement). d_selected[n_tracks] holds the track ids in selection order, -1 after them.
 * One workgroup runs the loop; nothing synchronises and nothing allocates.
 *
 * gtsfm_transavg_mfas: (c) the MFAS outlier weights of compute_inliers :212-237, all projection directions in one
 * launch (the reference: one gtsam.MFAS per direction in a Python loop, "TODO: parallelize this step").
 * d_proj[n_dir][3] are the projection directions. Only measurements with valid != 0 (NULL = all), keys in [0, n_nodes)
 * and key1 != key2 take part. For direction d, w_e = u_e . d with the three products summed x, y, z left to right;
 * edge e is oriented key1 -> key2 if w_e >= 0, else key2 -> key1, with weight |w_e|. inSum[v] and outSum[v] add the
 * weights of v's incoming and outgoing edges in ascending measurement index. Then, until no node remains: if a
 * remaining node has inSum < 1e-8, pick the one of lowest index; otherwise pick the remaining node with the largest
 * (outSum + 1) / (inSum + 1), lowest index on ties. Remove it; each remaining out-neighbour gets inSum -= |w| and each
 * remaining in-neighbour outSum -= |w|, one subtraction per removed edge (two edges to the same neighbour: ascending
 * measurement index), so a node's sequence of subtractions is fixed by the removal order alone. Edge e is violated for
 * d when its sink was removed before its source; its outlier weight is then |w_e|, else 0.
 * d_outlier_sum[e] adds the outlier weights in ascending direction index; d_inlier[e] = 1 iff the measurement takes
 * part and outlier_sum / n_dir < outlier_weight_threshold (the reference's 0.125). d_violated (optional, else NULL):
 * [n_dir][ceil(n_meas / 32)] uint32, bit (e & 31) of word e >> 5 set iff e is violated for that direction.
 * Stated deviation: GTSAM's MFAS walks an unordered_map, so its choice among simultaneous sources and among exact ties
 * of the heuristic is implementation-defined; the lowest-index rule replaces it.
 * One workgroup per direction keeps inSum, outSum and the removal position in LDS, 20 bytes per node, so n_nodes <=
 * GTSFM_TRANSAVG_MFAS_MAX_NODES (160 KiB of LDS); beyond it, for n_dir > 2^20 or n_meas >= 2^30: GTSFM_ERR_ARG.
 * The loop runs n_nodes steps by construction; there is no wait between workgroups, no floating-point atomic, nothing
 * allocates or synchronises, and two calls return the same bytes.
 *
 * gtsfm_transavg_recover: (d) the last loop of compute_inliers :239-256 and __run_averaging :374-430, i.e. GTSAM's
 * TranslationRecovery.run(measurements, scale) without priors.
 * A measurement is kept iff d_meas_inlier[e] != 0, key1 is a camera, key2 a node, key1 != key2 and, for a track
 * measurement (key2 >= n_img), its camera is an endpoint of an inlier camera edge. Every node of a kept measurement
 * is a variable. Nodes joined by a kept measurement with a zero direction (every |component| <= 1e-9) share one
 * position, that of the lowest index of their set (TranslationRecovery's same-translation sets); measurements inside
 * a set are dropped. Factors, per remaining measurement (a, b) = the sets of (key1, key2): residual
 * normalize(t_b - t_a) - u_e, isotropic sigma 0.01, under Huber k = 1.345 on the whitened norm when robust != 0, with
 * the sqrt-weight row scaling of gtsfm_global_ba. Gauge: PriorFactor<Point3> at the origin, sigma 0.01, on key1 of the
 * first remaining measurement in input order. Scale: BetweenFactor<Point3>(key1, key2, scale u) on that measurement
 * with its noise model. Initial values (stated deviation: GTSAM draws uniform (-1, 1) from a static mt19937(42) in
 * hash-map order): coordinate k of node v is 2 U - 1, U = (h >> 11) 2^-53, h = mix(mix(seed ^ mix(v)) + k), mix the
 * splitmix64 finaliser stated at gtsfm_triangulate_tracks. A set with no factor sits at the origin (GTSAM does that
 * only when no factor remains at all).
 * LM: GTSAM's default LevenbergMarquardtParams as gtsfm_global_ba restates them (lambda 1e-5, factor 10, upper bound
 * 1e5, minModelFidelity 1e-3, relative and absolute tolerances 1e-5, max_iterations 0 = 100). Linear solve: conjugate
 * gradients on the damped normal equations, never formed (one pass over the factors, one over the node-major lists),
 * preconditioned by the inverse 3 x 3 diagonal blocks, from a zero start, until ||r|| <= pcg_rel_tol ||b|| or
 * pcg_max_iter products (counted as a cap hit). No elimination.
 * Outputs: d_wti[n_img][3] and d_wti_valid[n_img] (0: the camera is not a variable or d_rot_valid is 0; position
 * zeroed), d_landmark[n_landmarks][3] and d_landmark_valid, d_stats[10] doubles = { initial error, final error, LM
 * iterations, LM trials, PCG iterations, PCG cap hits, optimised sets, factors (without prior and scale), valid
 * cameras, status }. Status 0: done (possibly with no factor: every variable at the origin); 1: no measurement kept;
 * 2: the error is not finite. As gtsfm_global_ba, the LM / PCG control flow is host code, so the call SYNCHRONISES its
 * stream; it allocates nothing, sums in a fixed order, uses no floating-point atomic, and two calls return the same
 * bytes. n_meas <= 0 or >= 2^30, n_img <= 0, n_img + n_landmarks > 2^24, a NULL required pointer, max_iterations < 0,
 * pcg_rel_tol not > 0 or pcg_max_iter <= 0: GTSFM_ERR_ARG; a short workspace: GTSFM_ERR_CAPACITY.
 * ---------------------------------------------------------------------------------------------- */
#define GTSFM_TRANSAVG_MFAS_MAX_NODES 8000
/* 0 for n_edges <= 0, n_img <= 0 or an unsupported shape (a size >= 2^30, n_img > 2^20). */
size_t gtsfm_transavg_measurements_workspace_bytes(int n_edges, long long n_tracks, long long n_meas, int n_img);

int gtsfm_transavg_measurements(const int* d_edges, const double* d_i2Ui1, const uint8_t* d_edge_valid, int n_edges,
                                const double* d_wRi, const uint8_t* d_rot_valid, int n_img,
                                const int* d_track_offsets, const int* d_track_img, const void* d_track_uv,
                                int uv_is_f64, long long n_tracks, const long long* d_n_tracks, long long n_meas,
                                const double* d_intrinsics, int measurements_per_camera, void* d_workspace,
                                size_t workspace_bytes, int* d_meas_key, double* d_meas_dir, uint8_t* d_meas_valid,
                                int* d_selected, uint8_t* d_cam_valid, long long* d_counts, void* stream);

/* 0 for an empty or unsupported shape (see above). */
size_t gtsfm_transavg_mfas_workspace_bytes(long long n_meas, int n_nodes, int n_dir);

int gtsfm_transavg_mfas(const int* d_meas_key, const double* d_meas_dir, const uint8_t* d_meas_valid, long long n_meas,
                        int n_nodes, const double* d_proj, int n_dir, double outlier_weight_threshold,
                        void* d_workspace, size_t workspace_bytes, double* d_outlier_sum, uint8_t* d_inlier,
                        uint32_t* d_violated, void* stream);

/* 0 for an empty or unsupported shape (see above). */
size_t gtsfm_transavg_recover_workspace_bytes(long long n_meas, int n_img, int n_landmarks);

int gtsfm_transavg_recover(const int* d_meas_key, const double* d_meas_dir, const uint8_t* d_meas_inlier,
                           long long n_meas, int n_img, int n_landmarks, const uint8_t* d_rot_valid, int robust,
                           double scale, uint64_t seed, int max_iterations, double pcg_rel_tol, int pcg_max_iter,
                           void* d_workspace, size_t workspace_bytes, double* d_wti, uint8_t* d_wti_valid,
                           double* d_landmark, uint8_t* d_landmark_valid, double* d_stats, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Rotation averaging, Shonan: gtsfm/averaging/rotation/shonan.py ShonanRotationAveraging, i.e. GTSAM's
 * ShonanAveraging3::run(initial, p_min, p_max) with LevenbergMarquardtParams::CeresDefaults (:54), no Huber (:56)
 * and certifyOptimality (:57), in one call. "GTSAM does" below is GTSAM 4.2 as remembered; this text is the contract.
 *
 * The problem. Edge e = (a, b) = d_edges[e] with aRb = d_aRb[e] (row-major 3 x 3) and kappa = d_kappa[e] (NULL = 1)
 * asks that wRa aRb = wRb. A two-view measurement (i1, i2) -> i2Ri1 is the edge a = i2, b = i1, aRb = i2Ri1
 * (BetweenFactorPose3(i2_, i1_, i2Ti1) :75); a pose prior on (i1, i2) with value i1Ti2 is a = i1, b = i2, aRb =
 * R(i1Ti2) (:97); kappa = 1 / sigma^2 with sigma = two_view_rotation_sigma (:65) or sqrt(mean(diag(covariance)))
 * (:85-90). A pair given twice contributes twice. At level p camera i has Y_i in St(p, 3), a p x 3 matrix with
 * orthonormal columns, stored [n][p][3]; the cost is f(Y) = sum_e kappa_e |Y_a aRb - Y_b|_F^2 = tr(Y Q Y'), Q the
 * 3n x 3n connection Laplacian. Stated deviation: GTSAM optimises over SO(p) and uses the first three columns, the
 * same problem with a redundant gauge.
 *
 * Setup. An edge is valid iff d_edge_valid[e] != 0 (NULL = all), both indices lie in [0, n_img), a != b, aRb is
 * finite and kappa is finite and > 0. Of the connected components of the valid edges the largest is kept, ties to the
 * one holding the lowest camera index (stated deviation: GTSAM requires a connected graph and GTSfM prunes to the
 * largest component upstream). Cameras outside it and cameras with no valid edge (the reference's None, :195-197) get
 * d_rot_valid = 0 and a zero matrix. The kept cameras are renumbered consecutively in ascending index
 * (old_to_new_idxes :183-184) and the half-edges listed node-major in ascending edge index.
 *
 * The staircase, p = p_min .. p_max with 3 <= p_min <= p_max <= 30 (the reference: 5 and 30, :50-51).
 * Initial values: rows 0..2 of Y_i are d_wRi_init[i] (row-major), the other rows zero; with d_wRi_init NULL the
 * seeded rotation of camera i: entry k of a 3 x 3 matrix is 2 U - 1, U = (h >> 11) 2^-53, h = mix(mix(seed ^ mix(i))
 * + k), mix the splitmix64 finaliser stated at gtsfm_triangulate_tracks, then its polar factor, third column negated
 * when the determinant is negative (stated deviation: GTSAM's initializeRandomly uses its own generator). Either way
 * Y_i then goes through the retraction once.
 * Level p: Riemannian Levenberg-Marquardt on St(p, 3)^n. Gradient g = 2 Proj_Y(Y Q), Proj_Y(V)_i = V_i - Y_i
 * sym(Y_i' V_i); Hessian H V = 2 Proj_Y(V Q - V Lambda), Lambda_i = sym(Y_i' (Y Q)_i); damped system (H + lambda D)
 * x = -g with D_i = 2 sum of the kappa at camera i, the diagonal of 2 Q (CeresDefaults' diagonalDamping; stated
 * deviation: the diagonal of Q, not of the projected Hessian). CeresDefaults: lambdaInitial 1e-4, lambdaFactor 2,
 * lambdaUpperBound 1e32, lambdaLowerBound 1e-16, useFixedLambdaFactor false, minModelFidelity 1e-3: a step is
 * accepted when rho = (f - f_new) / (-<g, x> - <x, H x> / 2) > 1e-3 and f_new < f, then lambda *= max(1/3, 1 -
 * (2 rho - 1)^3), not below 1e-16, and the factor returns to 2; otherwise lambda *= factor, factor *= 2, and the
 * level ends when lambda passes 1e32. Stated deviation: CeresDefaults stops on relativeErrorTol 1e-6 after at most
 * 50 iterations; here a level stops when |g| <= grad_rel_tol G0, G0 = sqrt(3 sum_i D_i^2) (the norm of 2 diag(Q) Y),
 * or after max_iterations accepted steps.
 * Linear solve: conjugate gradients, matrix-free, preconditioned by the inverse diagonal blocks of 2 (1 + lambda) Q,
 * D_i (1 + lambda) I, from a zero start until |r| <= pcg_rel_tol |g| or pcg_max_iter products (a cap hit); when a
 * product finds <p, (H + lambda D) p> <= 0 the solve stops with what it has, the preconditioned steepest descent
 * step if it was the first product.
 * Retraction: the polar factor A (A'A)^-1/2 of A = Y_i + x_i (3 x 3 Jacobi).
 * Certificate: S = Q - blockdiag(Lambda). Its smallest eigenpair (theta, v) by Lanczos with the basis on the device,
 * full reorthogonalisation (two passes), the tridiagonal problem solved on the host by cyclic Jacobi, cycles of at
 * most 128 vectors restarted from the Ritz vector, a seeded start vector, until |S v - theta v| <= eig_tol or
 * eig_max_steps products. theta is the Rayleigh quotient of the normalised Ritz vector, so theta >= lambda_min(S).
 * The level is certified iff theta > optimality_threshold (the reference's -1e-4): "not certified" is therefore always
 * right, "certified" relies on the residual, which is reported in d_stats and enters the decision only as the
 * stopping rule (when the step cap ends the iteration the last theta decides).
 * Not certified and p < p_max: append a zero row to every Y_i and step along e_{p+1} v_i' through the retraction, from
 * alpha = max(10.24, 0.1 / |theta|), halving while alpha >= 0.01; the first point of lower cost is taken, else the
 * last tried (GTSAM's initializeWithDescent, without its gradient-norm condition). p_max reached uncertified: the
 * reference raises; here status 2 and the rotations are rounded from the last level and returned.
 * Rounding (roundSolution): the three dominant eigenvectors U (p x 3) of sum_i Y_i Y_i' (host Jacobi) give the blocks
 * U' Y_i; when more than half of them have a negative determinant the third row of every block is negated; each block
 * is projected to the closest rotation by a 3 x 3 SVD. No anchoring: the frame is what rounding gives.
 *
 * Outputs: d_wRi[n_img][9] row-major, d_rot_valid[n_img], d_stats[12] doubles = { initial cost, final cost, final p,
 * theta, eigen residual, accepted LM steps, PCG products, PCG cap hits, Lanczos products, valid cameras, edges used,
 * status }. Status 0: certified; 1: no valid edge; 2: p_max reached uncertified; 3: a cost was not finite (no camera
 * valid). The LM / PCG / Lanczos control flow is host code, so the call SYNCHRONISES its stream; it allocates
 * nothing, sums in a fixed order (a camera's half-edges are split over the lanes of one wave and added in a fixed
 * tree), uses no floating-point atomic, and two calls return the same bytes.
 * n_edges <= 0 or >= 2^30, n_img <= 0 or > 2^20, p_min < 3, p_max < p_min, p_max > 30, a NULL d_edges, d_aRb,
 * d_workspace or output, a tolerance not > 0, a cap <= 0 or a non-finite threshold: GTSFM_ERR_ARG; a short workspace:
 * GTSFM_ERR_CAPACITY.
 * ---------------------------------------------------------------------------------------------- */
/* 0 for an empty or unsupported shape (see above). */
size_t gtsfm_rotavg_workspace_bytes(int n_edges, int n_img, int p_max);

int gtsfm_rotavg_shonan(const int* d_edges, const double* d_aRb, const double* d_kappa, const uint8_t* d_edge_valid,
                        int n_edges, int n_img, const double* d_wRi_init, uint64_t seed, int p_min, int p_max,
                        double optimality_threshold, double grad_rel_tol, int max_iterations, double pcg_rel_tol,
                        int pcg_max_iter, double eig_tol, int eig_max_steps, void* d_workspace, size_t workspace_bytes,
                        double* d_wRi, uint8_t* d_rot_valid, double* d_stats, void* stream);

/* ----------------------------------------------------------------------------------------------
 * The input of global bundle adjustment: gtsfm/data_association/data_assoc.py:123-160
 * assemble_gtsfm_data_from_tracks without its metrics (the valid tracks, then
 * GtsfmData.select_largest_connected_component, gtsfm/common/gtsfm_data.py:238-274, get_nodes_in_largest_connected_
 * component, gtsfm/utils/graph.py:20-39, and from_selected_cameras, gtsfm_data.py:286-317). It sits between
 * gtsfm_triangulate_tracks and gtsfm_global_ba: the masks it writes are the d_cam_valid and d_track_valid of the latter.
 *
 * Inputs, as the upstream calls leave them: the track CSR d_track_offsets[n_tracks + 1] (ascending over the tracks in
 * use, as gtsfm_tracks_from_matches writes it) and d_track_img[n_meas]; n_tracks is the track count or, with d_n_tracks
 * non-NULL, a capacity (min(n_tracks, d_n_tracks[0]) is used, read on the device); d_track_valid[n_tracks], the `valid`
 * byte of DataAssociation.run_triangulation_arrays, or NULL (all); d_meas_inlier[n_meas], the triangulation's inlier
 * bytes, or NULL (all); d_cam_valid[n_img] or NULL (all); d_extra_edges[n_extra][2] int32 or NULL with n_extra == 0: the
 * reference's extra_camera_edges, the keys of the relative-pose priors. An extra edge with an end outside [0, n_img)
 * or at an invalid camera is ignored.
 * Semantics.
 *   Accepted track: its valid byte is set and its offsets lie inside [0, n_meas]. Its measurements are those whose
 *     inlier byte is set (the reference's SfmTrack holds inliers only). valid already requires exit code 0, so the
 *     reference's skip of CHEIRALITY_FAILURE tracks (data_assoc.py:134-135) needs no test of its own.
 *   Graph nodes: the cameras named by an accepted track of at least two measurements, and the ends of the extra edges
 *     in use. itertools.combinations of one camera adds nothing (gtsfm_data.py:259), so a camera seen only in
 *     one-measurement tracks is in no component. A camera with d_cam_valid 0 that a track names is a node and counts
 *     in its component's size, as in the reference, whose graph is built from the tracks alone; it is never kept. A
 *     measurement whose image index is outside [0, n_img) is in no camera: it joins nothing and its track is not kept.
 *   Graph edges: all cameras of one accepted track are joined; the two ends of each extra edge are joined.
 *   Selected component: the one with the most nodes; among equals, the one whose first contributing item has the
 *     smallest index, where track t has index t and extra edge e has index n_tracks + e. That is what
 *     max(nx.connected_components(G), key=len) returns for a graph built by add_edges_from over the tracks in ascending
 *     order and then the extra edges: networkx keeps nodes in insertion order and yields the components in the order of
 *     their first node, and max keeps the first maximum. Verified against networkx 3.4.2 (tests/test_multi_view.py).
 *     gtsfm_rotavg_shonan's rule for equal components (the lowest camera index) is another one, on purpose: there the
 *     reference's graph is built from a dict of pairs.
 *   No edge at all: the result is empty (gtsfm_data.py:265-266), whatever the tracks.
 * Outputs (caller-owned): d_cam_keep[n_img] bytes: the camera is valid and lies in the selected component;
 * d_track_keep[n_tracks] bytes: the track is accepted and every one of its inlier measurements is in a kept camera
 * (from_selected_cameras, :299-315; an accepted one-measurement track in a kept camera is kept); d_track_len[n_tracks]
 * int32: the inlier count of a kept track, else 0 (the reference's 3d_tracks_length); d_stats[6] int64 = { components,
 * cameras kept, tracks kept, measurements kept, accepted tracks, valid cameras }. Entries of tracks past the count in
 * use are 0.
 * Integers only: a lock-free union-find over the cameras with one lane per measurement, per-root sizes and first items
 * by integer atomicAdd / atomicMin, one workgroup that reduces the roots to the winner. The outputs depend on the
 * input set alone and are byte-identical from launch to launch. Nothing allocates or synchronises.
 * Workspace: 17 bytes per camera and 8 per track. n_tracks, n_meas or n_img == 0 returns GTSFM_OK with zeroed outputs
 * and launches no kernel. A negative size, n_tracks + n_extra or n_meas + n_extra >= 2^31 - 1 or a NULL required
 * pointer returns GTSFM_ERR_ARG; a workspace smaller than the query's answer returns GTSFM_ERR_CAPACITY.
 * ---------------------------------------------------------------------------------------------- */
/* 0 for an empty shape (a size <= 0) or an unsupported one (n_tracks >= 2^31 - 1). */
size_t gtsfm_assemble_ba_input_workspace_bytes(long long n_tracks, int n_img);

int gtsfm_assemble_ba_input(const int* d_track_offsets, const int* d_track_img, long long n_tracks,
                            const long long* d_n_tracks, long long n_meas, const uint8_t* d_track_valid,
                            const uint8_t* d_meas_inlier, const uint8_t* d_cam_valid, int n_img,
                            const int* d_extra_edges, int n_extra, void* d_workspace, size_t workspace_bytes,
                            uint8_t* d_cam_keep, uint8_t* d_track_keep, int* d_track_len, long long* d_stats,
                            void* stream);

/* ----------------------------------------------------------------------------------------------
 * Dense multi-view stereo around a depth estimator (gtsfm/densify/). The depth network is gtsfm_patchmatchnet_* below;
 * these calls choose its inputs and turn its depth and confidence maps into a point cloud. GTSFM_HIP_ABI_VERSION stays
 * 407 with gtsfm_mvs_* added: new symbols only.
 *
 * Conventions shared by the five blocks below. A camera is wRc[9] (row-major, camera to world), wtc[3] (its centre)
 * and intrinsics (f, u0, v0), all float64: X_cam = wRc' (X - wtc), u = f x / z + u0, v = f y / z + v0. Pixel (x, y)
 * is column x of row y, at integer coordinates, as in the reference's meshgrid. "View" means pm_i, the dense index of
 * a valid camera (below); per-view arrays are indexed by pm_i.
 * ---------------------------------------------------------------------------------------------- */

/* Source views and depth ranges: gtsfm/densify/patchmatchnet_data.py:78-162 select_src_views_depth_ranges (a triple
 * Python loop over tracks and measurement pairs with GTSAM calls) and :55-63 (the pm_i maps), with
 * gtsfm/densify/mvs_utils.py:21-50 and :96-123.
 *
 * Inputs: the track CSR d_track_offsets[n_tracks + 1] (ascending) and d_track_img[n_meas]; d_point[n_tracks][3];
 * d_track_keep[n_tracks] and d_meas_inlier[n_meas] bytes, NULL = all; d_wRc, d_wtc per image; d_cam_keep[n_img] bytes,
 * NULL = all; max_num_views >= 1 (the reference's num_views, 5).
 * Valid cameras are the kept ones, numbered densely in ascending image index: pm_i. d_img_to_pm[n_img] holds pm_i or
 * -1, d_pm_to_img[n_img] the image of pm_i = 0 .. n_valid - 1 and -1 after them. A measurement counts when its track
 * is kept and lies inside [0, n_meas], its inlier byte is set and its image is a valid camera.
 * Pair score: for every kept track, every unordered pair of its counting measurements in two different valid cameras
 *   a, b adds piecewise_gaussian(theta) to score[a][b] and score[b][a]. theta, in degrees and fp64, is the angle at the
 *   3D point between the rays to the two camera centres: both rays normalised, the dot product clipped to [-1, 1],
 *   acos, times 180 / pi. The Gaussian is exp(-(theta - 5)^2 / (2 sigma^2)) with sigma 1 for theta <= 5 and 10 above.
 *   Each term is added as llround(score 2^40) with a 64-bit integer atomic, so the matrix is the same bytes from launch
 *   to launch: d_scores[n_img][n_img] int64 with row stride n_img, pm-indexed, of which the leading n_valid x n_valid
 *   block is used; divide by 2^40. The diagonal is 0 and never chosen (the reference holds -inf there). A term that is
 *   not a number (the point at a camera centre) is skipped. Two measurements of one track in the same camera add
 *   nothing (the reference would add to the diagonal).
 * Source views: V = min(max_num_views, n_valid); row r of d_src_views[n_img][max_num_views - 1] holds the V - 1
 *   other views of highest score, descending, and -1 after them; rows from n_valid on are -1. Equal scores go to the
 *   lower pm_i. This rule is ours: the reference's np.argsort(-scores) is not stable, so among ties, and zero scores
 *   tie often, its order is unspecified. A zero-score view is still chosen when nothing better exists, as in the
 *   reference.
 * Depth range: the depths of camera r are the third component of wRc' (X - wtc), fp64, over its counting
 *   measurements. d_depth_range[n_img][2] = (P1, P99) of them with np.percentile's default linear interpolation: virtual
 *   index (n - 1) q, g its fraction, a + (b - a) g for g < 0.5 and b - (b - a) (1 - g) otherwise. Any count works: the
 *   order statistics come from a radix select over the list in global memory, not from a sort. A valid camera with no
 *   counting measurement gets (NaN, NaN) and counts in d_stats[2]; the reference would raise there. Rows from n_valid
 *   on are 0.
 * d_stats[4] int64 = { n_valid, V - 1, valid cameras without a depth, score terms added (one per pair) }.
 * The caller reads n_valid from d_stats to slice the outputs; the call itself neither allocates nor synchronises.
 * Workspace: 12 bytes per image and 8 per measurement. n_tracks, n_meas or n_img == 0 returns GTSFM_OK with every
 * output zeroed (n_valid 0) and launches no kernel. A negative size, n_tracks or n_meas >= 2^31 - 1, n_img > 46340
 * (n_img^2 must fit an int), max_num_views < 1 or > 65536 or a NULL required pointer: GTSFM_ERR_ARG; a short workspace:
 * GTSFM_ERR_CAPACITY. */
/* 0 for an empty or unsupported shape. */
size_t gtsfm_mvs_select_views_workspace_bytes(long long n_tracks, long long n_meas, int n_img);

int gtsfm_mvs_select_views(const int* d_track_offsets, const int* d_track_img, long long n_tracks, long long n_meas,
                           const double* d_point, const uint8_t* d_track_keep, const uint8_t* d_meas_inlier,
                           const double* d_wRc, const double* d_wtc, const uint8_t* d_cam_keep, int n_img,
                           int max_num_views, void* d_workspace, size_t workspace_bytes, int* d_img_to_pm,
                           int* d_pm_to_img, long long* d_scores, int* d_src_views, double* d_depth_range,
                           long long* d_stats, void* stream);

/* Depth filtering and fusion: gtsfm/densify/mvs_patchmatchnet.py:201-371 filter_depth and :374-437
 * compute_filtered_reprojection_error over thirdparty/patchmatchnet/eval.py:11-76 reproject_with_depth and :79-125
 * check_geometric_consistency (per (reference, source) pair two full-frame cv2.remap reprojections on the host).
 *
 * Inputs: d_depth and d_confidence [n_views][height][width] float32; cameras per view; d_src_views[n_views][n_src]
 * int32 (an entry outside [0, n_views) is no source); the reference's thresholds are pixel_thresh 1.0, depth_thresh
 * 0.01, min_confidence 0.8, min_consistent_views 1.
 * Per (pixel (x, y) of view r with depth d_ref, source s), geometry in fp64:
 *   X_r = ((x - u0_r) / f_r d_ref, (y - v0_r) / f_r d_ref, d_ref); X_s = wRc_s' ((wRc_r X_r + wtc_r) - wtc_s);
 *   (u_s, v_s) its projection. The source depth is sampled bilinearly at (float32(u_s), float32(v_s)) in float32,
 *   ((v00 (1 - ax)) (1 - ay) + (v10 ax) (1 - ay)) + ((v01 (1 - ax)) ay + (v11 ax) ay), with a constant-0 border: a tap
 *   outside the map is 0, so samples within one pixel of the border blend with 0 and samples further out (or not finite)
 *   are 0. The sample is back-projected with the unrounded (u_s, v_s), brought to the frame of r the same way and
 *   projected: d_reproj = float32(z), (u', v') = float32 of the projection.
 *   dist = sqrt((u' - x)^2 + (v' - y)^2) in fp64 on the float32 values; rel = |d_reproj - d_ref| / d_ref in float32.
 *   Consistent iff d_ref is finite and > 0, dist < pixel_thresh and rel < float32(depth_thresh). (numpy compares its
 *   float32 arrays with the Python thresholds in float32; so does min_confidence below.)
 *   Stated deviation: cv2.remap additionally quantises the fractional sample position to 1/32 pixel and blends with
 *   its own rounding; here the weights are the float32 fractions themselves.
 * Per pixel: geo_sum = consistent sources; fused = float32((float32 sum of the consistent d_reproj in source order,
 *   then + d_ref) / (geo_sum + 1), the division in fp64); geo = d_ref finite and > 0 and geo_sum >=
 *   min_consistent_views; conf = confidence > float32(min_confidence); joint = geo and conf; d_fused is 0 where joint is
 *   false. Stated deviation: the reference has no test of d_ref in geo. It changes nothing for min_consistent_views
 *   >= 1, where such a pixel has geo_sum = 0; for min_consistent_views <= 0 the reference passes (0 + d_ref) / 1 on as
 *   the fused depth, a NaN or a point at or behind the camera, and here the pixel is dropped.
 * Outputs: d_fused[n_views][height][width] float32; d_mask, one byte per pixel: bit 0 geo, bit 1 conf, bit 2 joint;
 * d_counts[n_views][4] int64 = { geo pixels, conf pixels, joint pixels (the view's point count), reprojection errors
 * counted }: the reference's three ratios times height * width; d_err[n_views][3] float64 = { sum, min, max } of dist
 * over every source with dist < pixel_thresh at a joint pixel (min = max = 0 without one). The sum is accumulated as
 * llround(dist 2^24) in 64-bit integers, hence pixel_thresh <= 1024. Everything is byte-identical from launch to launch.
 * Workspace: 24 bytes per view. n_views == 0 returns GTSFM_OK and touches nothing; height or width == 0 zeroes d_counts
 * and d_err; neither launches a kernel. A negative size, n_views > 65535, height * width >= 2^31 - 256, a threshold
 * that is not a number, pixel_thresh outside [0, 1024] or a NULL required pointer: GTSFM_ERR_ARG; a short workspace:
 * GTSFM_ERR_CAPACITY. */
size_t gtsfm_mvs_fuse_depth_workspace_bytes(int n_views, int height, int width);

int gtsfm_mvs_fuse_depth(const float* d_depth, const float* d_confidence, int n_views, int height, int width,
                         const double* d_wRc, const double* d_wtc, const double* d_intrinsics, const int* d_src_views,
                         int n_src, double pixel_thresh, double depth_thresh, double min_confidence,
                         int min_consistent_views, void* d_workspace, size_t workspace_bytes, float* d_fused,
                         uint8_t* d_mask, long long* d_counts, double* d_err, void* stream);

/* The point cloud of the joint pixels: gtsfm/densify/mvs_patchmatchnet.py:325-357 (per view a boolean gather, a
 * back-projection and a colour cast, then two concatenations on the host).
 * A pixel is a point iff bit 2 of d_mask is set. d_view_offset[n_views + 1] int64 is the exclusive scan of the per-view
 * point counts, taken on the device. Point k of view r, in row-major pixel order, goes to row d_view_offset[r] + k:
 * views ascending, then row-major, the reference's concatenation order. d_points[capacity][3] float64 = wRc_r X_r +
 * wtc_r with X_r from d_fused as above; d_colors[capacity][3] uint8 from d_images[n_images][image_height][image_width]
 * [3] uint8, image d_view_image[r] (NULL = r; an index outside [0, n_images) gives black), pixel (x, y): the reference's
 * ((float32(c) / 255) * 255).astype(uint8), evaluated in float32 and truncated (with a correctly rounded division that
 * is c itself for all 256 values; the rule is evaluated all the same).
 * image_height >= height and image_width >= width: the maps cover the top-left corner of the image, the reference's
 * crop to multiples of 8. Rows at or past capacity are not written; d_view_offset[n_views] is the full count either
 * way, so capacity == 0 only counts. Workspace: 12 bytes per 256 pixels of every view and 8 per view. An empty shape
 * zeroes d_view_offset and launches no kernel; errors as for gtsfm_mvs_fuse_depth, and for an image smaller than the
 * maps. */
size_t gtsfm_mvs_gather_points_workspace_bytes(int n_views, int height, int width);

int gtsfm_mvs_gather_points(const float* d_fused, const uint8_t* d_mask, int n_views, int height, int width,
                            const double* d_wRc, const double* d_wtc, const double* d_intrinsics,
                            const uint8_t* d_images, const int* d_view_image, int n_images, int image_height,
                            int image_width, long long capacity, void* d_workspace, size_t workspace_bytes,
                            double* d_points, uint8_t* d_colors, long long* d_view_offset, void* stream);

/* The statistics behind the voxel size: gtsfm/densify/mvs_utils.py:148-190 estimate_voxel_scales and
 * estimate_minimum_voxel_size (gtsfm/utils/ellipsoid.py center_point_cloud and get_right_singular_vectors).
 * d_stats[18] float64 = { mean[3], scatter[9] (row-major, sum of the outer products of the centred points divided by
 * n_points - 1; all 0 for n_points < 2), min bound[3], max bound[3] }. Two passes in fp64 with a fixed grid of
 * workgroups and fixed-order sums: the same bytes from launch to launch. The voxel size is 0.02 sqrt(smallest
 * eigenvalue of the scatter), taken by the caller. n_points == 0 zeroes d_stats and launches no kernel. Workspace: at
 * most 72 KiB. n_points < 0 or a NULL pointer: GTSFM_ERR_ARG; a short workspace: GTSFM_ERR_CAPACITY. */
size_t gtsfm_mvs_voxel_stats_workspace_bytes(long long n_points);

int gtsfm_mvs_voxel_stats(const double* d_points, long long n_points, void* d_workspace, size_t workspace_bytes,
                          double* d_stats, void* stream);

/* Voxel downsampling: gtsfm/densify/mvs_utils.py:193-221 downsample_point_cloud (Open3D voxel_down_sample).
 * gtsfm_mvs_voxel_keys: per axis the voxel index floor((p - (min_bound - voxel_size / 2)) / voxel_size), Open3D's
 * rule, with min_bound read from the d_stats of gtsfm_mvs_voxel_stats; clamped to [0, 2^21 - 1] and packed as
 * x << 42 | y << 21 | z into d_keys[n_points] int64. voxel_size must be > 0 (a size <= 0 means "return the cloud
 * unchanged", the caller's business).
 * The caller orders the keys with a stable sort and passes the sorted keys and the permutation (int64 indices into the
 * input). gtsfm_mvs_voxel_downsample: one output row per distinct key, in ascending key order (Open3D's own order is
 * that of its hash map and unspecified): d_out_points = the mean of the voxel's points, summed in fp64 in sorted order
 * (ascending input index within a voxel); d_out_colors = the mean of the 0-255 values, truncated to uint8 (integer sum,
 * integer division); d_out_keys, d_out_count (points per voxel); d_n_voxels[1] the number of rows. Every output array
 * has n_points rows, zero past the voxel count. n_points == 0 zeroes d_n_voxels and launches no kernel. An extent of
 * 2^21 voxels or more along an axis is the caller's to refuse (gtsfm_amd.densify.mvs_utils does): the clamp would
 * merge everything past it into the last voxel, whose one lane would then add all those points. Workspace: 8 bytes
 * per point and 12 per 256 points. A negative size or a NULL pointer: GTSFM_ERR_ARG; a short workspace: GTSFM_ERR_CAPACITY. */
int gtsfm_mvs_voxel_keys(const double* d_points, long long n_points, const double* d_stats, double voxel_size,
                         long long* d_keys, void* stream);

size_t gtsfm_mvs_voxel_downsample_workspace_bytes(long long n_points);

int gtsfm_mvs_voxel_downsample(const double* d_points, const uint8_t* d_colors, const long long* d_sorted_keys,
                               const long long* d_perm, long long n_points, void* d_workspace, size_t workspace_bytes,
                               double* d_out_points, uint8_t* d_out_colors, long long* d_out_keys, int* d_out_count,
                               long long* d_n_voxels, void* stream);

/* ----------------------------------------------------------------------------------------------
 * PatchmatchNet: the depth network of the dense-MVS stage, eval mode, fp32, batched over reference views.
 * Replaces the model call of MVSPatchmatchNet.densify (gtsfm/densify/mvs_patchmatchnet.py:95-175, BATCH_SIZE 1, one
 * FeatureNet pass per (reference, source) use) and the network itself: thirdparty/patchmatchnet/models/net.py:15-330
 * (FeatureNet, Refinement, PatchmatchNet.forward), patchmatch.py:19-983 (initialisation, propagation, evaluation, the
 * three 1x1x1 nets) and module.py:134-213 (differentiable_warping, depth_regression); the per-stage projection
 * matrices of gtsfm/densify/patchmatchnet_data.py:208-227 are formed inside. GTSFM_HIP_ABI_VERSION stays 407: new
 * symbols only.
 *
 * Every view of the batch is a reference view once; its sources are d_src_views[view][n_src], rows of the same batch
 * (an index outside [0, n_views) is skipped: the view's result is that of a row holding only its valid sources, in
 * row order, bit for bit). A view whose row holds no valid source has no matching cost (the reference's weighted mean
 * is 0 / 0): its depth and confidence are NaN everywhere, so the confidence passes no `> threshold` test, and the other
 * views of the batch are not affected. Features are computed once per view.
 * d_images [n_views][H][W][3] uint8 RGB; H and W multiples of 8, at least 16. Cameras as for gtsfm_mvs_*: d_wRc
 * [n_views][9], d_wtc [n_views][3], d_intrinsics [n_views][3] = (f, u0, v0), float64; stage s uses the first two rows
 * of K divided by 2^s, and src_proj ref_proj^-1 is formed in fp64 from the poses (no matrix inverse) and rounded to fp32
 * once. d_depth_range [n_views][2] float64 = (min, max). d_init_uniform [n_views][48][H/8][W/8] float32 in [0, 1): the
 * random initialisation's numbers (torch.rand in the reference), an input so that a run can be repeated.
 * config: NULL, or the reference's constants (interval scales 0.005 / 0.0125 / 0.025, propagation ranges 6 / 4 / 2,
 * iterations 1 / 2 / 2, samples 8 / 8 / 16, propagate neighbours 0 / 8 / 16, evaluate neighbours 9 / 9 / 9, groups
 * 4 / 8 / 8, each indexed by stage - 1); anything else is GTSFM_ERR_ARG.
 * Outputs: d_depth_out and d_confidence_out [n_views][H][W] float32 (refined_depth["stage_0"] and
 * photometric_confidence). Optional, NULL = not wanted: d_features_out, the channels-last feature maps of every view,
 * stage 3 [n][H/8][W/8][64], then stage 2 [n][H/4][W/4][32], then stage 1 [n][H/2][W/2][16]; d_iter_depth_out, the depth
 * after each of the five patchmatch iterations: two [n][H/8][W/8] maps, two [n][H/4][W/4], one [n][H/2][W/2].
 *
 * d_weights: gtsfm_patchmatchnet_weights_floats() floats, BatchNorm (eps 1e-5) folded into the layer before it. A
 * convolution is W[ky][kx][ci][co] followed by bias[co] (zeros where the layer has none); a 1x1x1 net with G groups is
 * W0[G][16], b0[16], W1[16][8], b1[8], W2[8], b2[1]. In order: feature.conv0 .. conv10; output1, inner1, inner2,
 * output2, output3; for stage 3, 2, 1: evaluation.pixel_wise_net (stage 3 only), evaluation.similarity_net, propa_conv
 * (stages 3 and 2), eval_conv, feature_weight_net; upsample_net.conv0, conv1, conv2, deconv (+ bn; the transposed
 * convolution's weight[ci][co][ky][kx] stored as W[ky][kx][ci][co]), conv3, res.
 * Workspace: about 120 bytes per pixel of the batch plus 4 n_src bytes per stage-3 pixel; the query returns 0 for a
 * shape the call refuses. A NULL required pointer or a refused shape: GTSFM_ERR_ARG; a short workspace:
 * GTSFM_ERR_CAPACITY.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    double interval_scale[3];
    int propagation_range[3], iterations[3], num_samples[3], propagate_neighbors[3], evaluate_neighbors[3], groups[3];
} gtsfm_patchmatchnet_config;

size_t gtsfm_patchmatchnet_weights_floats(void);

size_t gtsfm_patchmatchnet_workspace_bytes(int n_views, int n_src, int height, int width);

int gtsfm_patchmatchnet_batched(const uint8_t* d_images, int n_views, int height, int width, const double* d_wRc,
                                const double* d_wtc, const double* d_intrinsics, const int* d_src_views, int n_src,
                                const double* d_depth_range, const float* d_weights, const float* d_init_uniform,
                                const gtsfm_patchmatchnet_config* config, void* d_workspace, size_t workspace_bytes,
                                float* d_depth_out, float* d_confidence_out, float* d_features_out,
                                float* d_iter_depth_out, void* stream);

/* Measurement hook, as gtsfm_match_set_kernel_events: events[6] are hipEvent_t recorded on the call's stream before
 * FeatureNet, before stage 3, stage 2, stage 1, Refinement, and at the end. NULL switches it off. Not thread-safe. */
int gtsfm_patchmatchnet_set_phase_events(void* const* events);

#ifdef __cplusplus
}
#endif

#endif /* GTSFM_HIP_H_ */
