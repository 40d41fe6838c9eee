// What the two two-view verifiers share (ransac.hip: essential matrix, fundamental.hip: fundamental matrix): the
// sampling hash, the iteration bound, the 3 x 3 decomposition, recoverPose and the putative gather kernel.
#pragma once
#include <math.h>

#include "common.hpp"

// No FMA contraction: every fused multiply-add is an explicit __builtin_fma() that the oracle performs in the same
// place. The pragma is file-scope and carries into the includer; both includers set it themselves as well.
#pragma clang fp contract(off)

namespace {

// sampling hash (identical to the oracle's)
__device__ __forceinline__ uint64_t sm_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Cyclic Jacobi eigen-decomposition, the same rotation sequence as oracle/ransac.c jacobi_eig. N = 3: fully
// unrolled, register resident (redundant per lane).
// Not to be merged with fundamental.hip's fm_jacobi, which follows oracle/fundamental.c's sequence instead.
template <int N>
__device__ __forceinline__ void jacobi_eig_reg(double (&a)[N * N], double (&w)[N], double (&V)[N * N]) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int j = 0; j < N; ++j) V[i * N + j] = (i == j) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int j = i + 1; j < N; ++j) off += a[i * N + j] * a[i * N + j];
        if (off < 1e-30) break;
#pragma unroll
        for (int p = 0; p < N; ++p)
#pragma unroll
            for (int q = p + 1; q < N; ++q) {
                const double apq = a[p * N + q];
                if (fabs(apq) < 1e-300) continue;
                const double app = a[p * N + p], aqq = a[q * N + q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double akp = a[k * N + p], akq = a[k * N + q];
                    a[k * N + p] = c * akp - s * akq;
                    a[k * N + q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double apk = a[p * N + k], aqk = a[q * N + k];
                    a[p * N + k] = c * apk - s * aqk;
                    a[q * N + k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double vkp = V[k * N + p], vkq = V[k * N + q];
                    V[k * N + p] = c * vkp - s * vkq;
                    V[k * N + q] = s * vkp + c * vkq;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = a[i * N + i];
}

__device__ void svd3(const double* E, double* U, double* s, double* V) {
    double ata[9], w[3], Vt[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc += E[k * 3 + i] * E[k * 3 + j];
            ata[i * 3 + j] = acc;
        }
    jacobi_eig_reg<3>(ata, w, Vt);
    // descending order of w (selection by comparisons, same result as the oracle's index sort)
    int o0 = 0, o1 = 1, o2 = 2;
    if (w[o1] > w[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (w[o2] > w[o0]) { const int t = o0; o0 = o2; o2 = t; }
    if (w[o2] > w[o1]) { const int t = o1; o1 = o2; o2 = t; }
    const int order[3] = {o0, o1, o2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int oc = order[c];
        const double wc = oc == 0 ? w[0] : oc == 1 ? w[1] : w[2];
        s[c] = sqrt(fmax(wc, 0.0));
#pragma unroll
        for (int r = 0; r < 3; ++r) V[r * 3 + c] = oc == 0 ? Vt[r * 3] : oc == 1 ? Vt[r * 3 + 1] : Vt[r * 3 + 2];
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        double u[3], nrm = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            u[r] = E[r * 3 + 0] * V[0 * 3 + c] + E[r * 3 + 1] * V[1 * 3 + c] + E[r * 3 + 2] * V[2 * 3 + c];
            nrm += u[r] * u[r];
        }
        nrm = sqrt(nrm);
#pragma unroll
        for (int r = 0; r < 3; ++r) U[r * 3 + c] = nrm > 0 ? u[r] / nrm : (r == c ? 1.0 : 0.0);
    }
    U[2] = U[3] * U[7] - U[6] * U[4];
    U[5] = U[6] * U[1] - U[0] * U[7];
    U[8] = U[0] * U[4] - U[3] * U[1];
    const double v0 = V[3] * V[7] - V[6] * V[4], v1 = V[6] * V[1] - V[0] * V[7], v2 = V[0] * V[4] - V[3] * V[1];
    V[2] = v0;
    V[5] = v1;
    V[8] = v2;
}

__device__ __forceinline__ double det3(const double* m) {
    return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

__device__ int wave_cheirality(const double* R, const double* t, const double2* x1, const double2* x2,
                               const uint8_t* mask, int M, int lane) {
    int good = 0;
    for (int i = lane; i < M; i += 64) {
        if (!mask[i]) continue;
        const double p0 = x1[i].x, p1 = x1[i].y, q0 = x2[i].x, q1 = x2[i].y;
        const double a0 = R[0] * p0 + R[1] * p1 + R[2];
        const double a1 = R[3] * p0 + R[4] * p1 + R[5];
        const double a2 = R[6] * p0 + R[7] * p1 + R[8];
        const double aa = a0 * a0 + a1 * a1 + a2 * a2;
        const double aq = a0 * q0 + a1 * q1 + a2;
        const double qq = q0 * q0 + q1 * q1 + 1.0;
        const double at = a0 * t[0] + a1 * t[1] + a2 * t[2];
        const double qt = q0 * t[0] + q1 * t[1] + t[2];
        const double det = aa * qq - aq * aq;
        if (fabs(det) < 1e-18) continue;
        const double l1 = (-at * qq + aq * qt) / det;
        const double z2 = l1 * a2 + t[2];
        good += (l1 > 0.0 && l1 < 50.0 && z2 > 0.0 && z2 < 50.0) ? 1 : 0;
    }
    for (int m = 32; m >= 1; m >>= 1) good += __shfl_xor(good, m);
    return good;
}

// recoverPose (oracle/ransac.c oracle_recover_pose) of E on the masked K-normalised correspondences: decomposition
// (redundant per lane), then the wave's cheirality vote over the four (R, t); the first of the most voted wins. The
// caller makes `mask` visible to the whole wave before the call and stores R (9), t (3) from one lane after it.
__device__ __forceinline__ void recover_pose(const double* E, const double2* x1, const double2* x2,
                                             const uint8_t* mask, int M, int lane, double* R, double* t) {
    double U[9], s[3], V[9];
    svd3(E, U, s, V);
    if (det3(U) < 0)
        for (int k = 0; k < 9; ++k) U[k] = -U[k];
    if (det3(V) < 0)
        for (int k = 0; k < 9; ++k) V[k] = -V[k];
    double R1[9], R2[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double uw0 = -U[r * 3 + 1], uw1 = U[r * 3 + 0], uw2 = U[r * 3 + 2];
            const double uwt0 = U[r * 3 + 1], uwt1 = -U[r * 3 + 0], uwt2 = U[r * 3 + 2];
            R1[r * 3 + c] = uw0 * V[c * 3 + 0] + uw1 * V[c * 3 + 1] + uw2 * V[c * 3 + 2];
            R2[r * 3 + c] = uwt0 * V[c * 3 + 0] + uwt1 * V[c * 3 + 1] + uwt2 * V[c * 3 + 2];
        }
    const double tp[3] = {U[2], U[5], U[8]};
    const double tn[3] = {-U[2], -U[5], -U[8]};
    const int g1 = wave_cheirality(R1, tp, x1, x2, mask, M, lane);
    const int g2 = wave_cheirality(R2, tp, x1, x2, mask, M, lane);
    const int g3 = wave_cheirality(R1, tn, x1, x2, mask, M, lane);
    const int g4 = wave_cheirality(R2, tn, x1, x2, mask, M, lane);
    const double* Rs;
    const double* ts;
    if (g1 >= g2 && g1 >= g3 && g1 >= g4) { Rs = R1; ts = tp; }
    else if (g2 >= g1 && g2 >= g3 && g2 >= g4) { Rs = R2; ts = tp; }
    else if (g3 >= g1 && g3 >= g2 && g3 >= g4) { Rs = R1; ts = tn; }
    else { Rs = R2; ts = tn; }
    for (int k = 0; k < 9; ++k) R[k] = Rs[k];
    for (int k = 0; k < 3; ++k) t[k] = ts[k];
}

// Iterations still needed for confidence p at outlier ratio ep (OpenCV RANSACUpdateNumIters), at most max_iters.
__device__ __attribute__((noinline)) int update_num_iters(double p, double ep, int model_points, int max_iters) {
    p = fmax(p, 0.0); p = fmin(p, 1.0);
    ep = fmax(ep, 0.0); ep = fmin(ep, 1.0);
    double num = fmax(1.0 - p, 2.2250738585072014e-308);
    double denom = 1.0 - pow(1.0 - ep, (double)model_points);
    if (denom < 2.2250738585072014e-308) return 0;
    num = log(num);
    denom = log(denom);
    return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)llround(num / denom);
}

// Gather + normalise the putatives of every pair: x = (uv - (u0, v0)) / f per image (utils/features.py:40-50) into
// x1n, x2n (fp64, what the refits and recoverPose read), and the float4 (x1, y1, x2, y2) that the estimation reads:
// the normalised coordinates rounded to fp32 (E path), or with kPixelPts the pixel coordinates as they are (F path).
template <bool kPixelPts>
__global__ void gather_putatives_kernel(const float* __restrict__ kp_xy, const double* __restrict__ intr, int kmax,
                                        const int* __restrict__ pairs, const uint32_t* __restrict__ match_idx,
                                        const int* __restrict__ match_count, int mcap, double2* __restrict__ x1n,
                                        double2* __restrict__ x2n, float4* __restrict__ pts) {
    const int p = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int M = match_count[p];
    if (i >= M) return;
    const int i1 = pairs[2 * p], i2 = pairs[2 * p + 1];
    const uint32_t a = match_idx[((size_t)p * mcap + i) * 2], b = match_idx[((size_t)p * mcap + i) * 2 + 1];
    const double f1 = intr[3 * i1], u1 = intr[3 * i1 + 1], v1 = intr[3 * i1 + 2];
    const double f2 = intr[3 * i2], u2 = intr[3 * i2 + 1], v2 = intr[3 * i2 + 2];
    const float* k1 = kp_xy + ((size_t)i1 * kmax + a) * 2;
    const float* k2 = kp_xy + ((size_t)i2 * kmax + b) * 2;
    const size_t o = (size_t)p * mcap + i;
    // the pixel float4 goes out ahead of the divisions, so its registers are free while the quotients are live
    if (kPixelPts) pts[o] = make_float4(k1[0], k1[1], k2[0], k2[1]);
    const double2 n1 = make_double2(((double)k1[0] - u1) / f1, ((double)k1[1] - v1) / f1);
    const double2 n2 = make_double2(((double)k2[0] - u2) / f2, ((double)k2[1] - v2) / f2);
    x1n[o] = n1;
    x2n[o] = n2;
    if (!kPixelPts) pts[o] = make_float4((float)n1.x, (float)n1.y, (float)n2.x, (float)n2.y);
}

}  // namespace
