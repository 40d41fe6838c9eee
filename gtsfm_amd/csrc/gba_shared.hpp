// What the two global bundle adjustments (gba.hip: fixed calibration, gba_calib.hip: refined calibration) share beyond
// se3.hpp, reduce.hpp, csr.hpp and lm.hpp: the pose prior's residual, the Cholesky inverse of a small symmetric positive
// definite block (the block-Jacobi preconditioner) and the csr.hpp source that groups factor measurements by camera.
// Sets no fp-contract pragma: include it after the includer's own (see se3.hpp).
#pragma once
#include <math.h>

#include "common.hpp"
#include "se3.hpp"

namespace {

constexpr double kPointPriorW = 100.0;  // PriorFactorPoint3 sigma 0.1

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

}  // namespace
