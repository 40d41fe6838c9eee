// Small fp64 geometry shared by the back-end solvers (ba2.hip, triangulate.hip, gba.hip, transavg.hip): 3 x 3 helpers,
// SO(3) / SE(3) exponential and logarithm, the pinhole projection with its Jacobians, 3 x 3 inverse and Cholesky
// solve, and the Huber pair. The arithmetic is oracle/ba2.c's, operation for operation.
//
// Floating-point contraction: this header sets no `#pragma clang fp contract`, and must not include a header that does
// (twoview.hpp). A file-scope pragma covers everything that follows it in the translation unit, so every .hip file
// includes this header AFTER its own pragma, if it has one. ba2.hip has none and contracts; every other includer sets
// contract(off) first and does not. The same rule holds for reduce.hpp, csr.hpp and lm.hpp.
#pragma once
#include <math.h>

#include "common.hpp"

namespace {

constexpr double kHuberK = 1.345;

struct Pose {
    double R[9];  // wRc row-major
    double t[3];  // wtc
};

__device__ __forceinline__ void skew3(const double* w, double* S) {
    S[0] = 0; S[1] = -w[2]; S[2] = w[1];
    S[3] = w[2]; S[4] = 0; S[5] = -w[0];
    S[6] = -w[1]; S[7] = w[0]; S[8] = 0;
}

__device__ __forceinline__ void mm3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

__device__ __forceinline__ void mtv3(const double* A, const double* v, double* o) {
#pragma unroll
    for (int j = 0; j < 3; ++j) o[j] = A[j] * v[0] + A[3 + j] * v[1] + A[6 + j] * v[2];
}

__device__ __forceinline__ void mv3(const double* A, const double* v, double* o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = A[3 * i] * v[0] + A[3 * i + 1] * v[1] + A[3 * i + 2] * v[2];
}

__device__ void so3_exp(const double* w, double* R) {
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double W[9], W2[9];
    skew3(w, W);
    mm3(W, W, W2);
    double a, b;
    if (th2 < 1e-16) {
        a = 1.0 - th2 / 6.0;
        b = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0 ? 1.0 : 0.0) + a * W[k] + b * W2[k];
}

__device__ void so3_log(const double* R, double* w) {
    double c = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    c = fmin(1.0, fmax(-1.0, c));
    const double th = acos(c);
    const double v[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    if (th < 1e-8) {
        for (int k = 0; k < 3; ++k) w[k] = 0.5 * v[k];
    } else if (3.14159265358979323846 - th < 1e-6) {
        const int i = (R[0] >= R[4] && R[0] >= R[8]) ? 0 : (R[4] >= R[8] ? 1 : 2);
        double ax[3];
        ax[i] = sqrt(fmax(0.0, (R[4 * i] + 1.0) * 0.5));
        for (int j = 0; j < 3; ++j)
            if (j != i) ax[j] = (R[3 * i + j] + R[3 * j + i]) / (4.0 * ax[i]);
        const double n = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
        for (int k = 0; k < 3; ++k) w[k] = th * ax[k] / n;
    } else {
        const double s = th / (2.0 * sin(th));
        for (int k = 0; k < 3; ++k) w[k] = s * v[k];
    }
}

__device__ void pose_retract(const Pose& X, const double* xi, Pose& o) {
    double dR[9], tv[3], W[9], W2[9];
    so3_exp(xi, dR);
    const double* w = xi;
    const double* v = xi + 3;
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    skew3(w, W);
    mm3(W, W, W2);
    double a, b;
    if (th2 < 1e-16) {
        a = 0.5 - th2 / 24.0;
        b = 1.0 / 6.0 - th2 / 120.0;
    } else {
        const double th = sqrt(th2);
        a = (1.0 - cos(th)) / th2;
        b = (th - sin(th)) / (th2 * th);
    }
    for (int i = 0; i < 3; ++i)
        tv[i] = v[i] + a * (W[3 * i] * v[0] + W[3 * i + 1] * v[1] + W[3 * i + 2] * v[2]) +
                b * (W2[3 * i] * v[0] + W2[3 * i + 1] * v[1] + W2[3 * i + 2] * v[2]);
    mm3(X.R, dR, o.R);
    double Rt[3];
    mv3(X.R, tv, Rt);
    for (int i = 0; i < 3; ++i) o.t[i] = X.t[i] + Rt[i];
}

__device__ void pose_log(const Pose& T, double* xi) {
    double w[3];
    so3_log(T.R, w);
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    xi[0] = w[0]; xi[1] = w[1]; xi[2] = w[2];
    if (th < 1e-10) {
        for (int k = 0; k < 3; ++k) xi[3 + k] = T.t[k];
        return;
    }
    double W[9], Wt[3], WWt[3];
    const double wn[3] = {w[0] / th, w[1] / th, w[2] / th};
    skew3(wn, W);
    mv3(W, T.t, Wt);
    mv3(W, Wt, WWt);
    const double tn = tan(0.5 * th);
    for (int k = 0; k < 3; ++k) xi[3 + k] = T.t[k] - (0.5 * th) * Wt[k] + (1.0 - th / (2.0 * tn)) * WWt[k];
}

// K = (f, cx, cy); pc is the point in the camera frame; false when it is not in front (z <= 0)
__device__ __forceinline__ bool project(const Pose& X, const double* K, const double* p, double* pc, double* uv) {
    const double d[3] = {p[0] - X.t[0], p[1] - X.t[1], p[2] - X.t[2]};
    mtv3(X.R, d, pc);
    if (pc[2] <= 0.0) return false;
    uv[0] = K[1] + K[0] * (pc[0] / pc[2]);
    uv[1] = K[2] + K[0] * (pc[1] / pc[2]);
    return true;
}

// d uv / d p (Jp, 2 x 3) and d uv / d pose (Jx, 2 x 6, rotation first) at a point in front of the camera
__device__ __forceinline__ void project_jac(const Pose& X, const double* K, const double* pc, double* Jp, double* Jx) {
    const double iz = 1.0 / pc[2], xn = pc[0] * iz, yn = pc[1] * iz, f = K[0];
    const double D[6] = {f * iz, 0.0, -f * xn * iz, 0.0, f * iz, -f * yn * iz};
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
}

__device__ __forceinline__ double huber_loss(double d) {
    return d <= kHuberK ? 0.5 * d * d : kHuberK * d - 0.5 * kHuberK * kHuberK;
}
__device__ __forceinline__ double huber_weight(double d) { return d <= kHuberK ? 1.0 : kHuberK / d; }

// inverse by cofactors; false when the determinant is zero or not finite
__device__ bool inv3(const double* A, double* I) {
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
    const double id = 1.0 / det;
    I[0] = c00 * id;
    I[1] = (A[2] * A[7] - A[1] * A[8]) * id;
    I[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    I[3] = c01 * id;
    I[4] = (A[0] * A[8] - A[2] * A[6]) * id;
    I[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    I[6] = c02 * id;
    I[7] = (A[1] * A[6] - A[0] * A[7]) * id;
    I[8] = (A[0] * A[4] - A[1] * A[3]) * id;
    return true;
}

// solves a x = b in place by Cholesky (the lower triangle of a is read, b becomes x); false when a is not positive
// definite
__device__ __forceinline__ bool chol3_solve(double* a, double* b) {
    for (int j = 0; j < 3; ++j) {
        double s = a[4 * j];
        for (int k = 0; k < j; ++k) s -= a[3 * j + k] * a[3 * j + k];
        if (!(s > 0.0)) return false;
        const double d = sqrt(s);
        a[4 * j] = d;
        for (int i = j + 1; i < 3; ++i) {
            double v = a[3 * i + j];
            for (int k = 0; k < j; ++k) v -= a[3 * i + k] * a[3 * j + k];
            a[3 * i + j] = v / d;
        }
    }
    for (int i = 0; i < 3; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= a[3 * i + k] * b[k];
        b[i] = v / a[4 * i];
    }
    for (int i = 2; i >= 0; --i) {
        double v = b[i];
        for (int k = i + 1; k < 3; ++k) v -= a[3 * k + i] * b[k];
        b[i] = v / a[4 * i];
    }
    return true;
}

}  // namespace
