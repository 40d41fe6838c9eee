// Rotation averaging, Shonan: the Riemannian staircase on St(p, 3)^n with an optimality certificate.
//
// Reference: gtsfm/averaging/rotation/shonan.py (ShonanRotationAveraging on GTSAM's ShonanAveraging3) and "Shonan
// Rotation Averaging" (arXiv 2008.02737). The semantics are stated in include/gtsfm_hip.h.
//
// The cost tr(Y Q Y') is quadratic in the lifted variable, so the gradient, the Hessian-vector product and the
// certificate's operator are all Out = V Q with Q the 3n x 3n connection Laplacian: ra_matvec, the hot kernel. Q is a
// node-major list of half-edges in ascending edge index (the stable counting sort of csr.hpp), each entry a
// neighbour, a 3 x 3 block (aRb' on the a side, aRb on the b side) and kappa, 80 + 4 bytes. One wave owns one node: its
// 64 lanes are (slice, row) pairs, floor(64 / p) slices of p rows; a lane walks the half-edges slice, slice + slices,
// ... of the node's list for its row of V and the slices are added in a fixed tree in LDS, so a hub camera's list is
// split over a wave and two calls give the same bytes. V is [n][p][3]; p = 1 is the certificate's matvec.
// The LM / PCG / Lanczos control flow is host code, as in gba.hip and transavg.hip; every reduction is one workgroup
// summing in a fixed order. fp64, no FMA contraction, no floating-point atomics.
#include <limits.h>
#include <math.h>

#include "twoview.hpp"  // sm_mix, jacobi_eig_reg, svd3, det3

#pragma clang fp contract(off)

#include "csr.hpp"
#include "reduce.hpp"  // uf_find, uf_unite

namespace {

constexpr int kPMax = 30;
constexpr int kRedBlock = 1024;
constexpr int kChunksMax = 256;
constexpr int kLanczosMax = 128;  // basis vectors per cycle
constexpr int kEntry = 10;        // doubles per half-edge: block[9], kappa
// LevenbergMarquardtParams::CeresDefaults
constexpr double kLambdaInitial = 1e-4;
constexpr double kLambdaFactor = 2.0;
constexpr double kLambdaUpper = 1e32;
constexpr double kLambdaLower = 1e-16;
constexpr double kMinFidelity = 1e-3;
constexpr double kAlphaMin = 1e-2;  // initializeWithDescent's smallest step

enum { I_NKEPT = 0, I_NEG, I_COUNT = 4 };
enum { S_DOT = 0, S_RZ, S_RR, S_NEG, S_GX, S_XQ, S_XDX, S_ALPHA, S_BETA, S_D2, S_COUNT = 16 };

struct Args {
    const int* edges;       // [E][2] (a, b)
    const double* aRb;      // [E][9]
    const double* kappa;    // [E] or NULL
    const uint8_t* evalid;  // [E] or NULL
    const double* init;     // [n_img][9] or NULL
    int E, n_img;
    CsrChunks chunks;
    uint64_t seed;
    uint8_t* use;    // [E]
    int* parent;     // [n_img]
    int* cnt;        // [n_img]
    uint8_t* hase;   // [n_img]
    uint8_t* keep;   // [n_img]
    int* newidx;     // [n_img]
    int* old;        // [n_img]
    int* icnt;       // [I_COUNT]
    int* rkey;       // [E][2]
    int* node_off;   // [n_img + 1]
    int* hist;       // [chunks][n_img]
    int* nbr;        // [2 E]
    double* blk;     // [2 E][kEntry]
    double* D;       // [n_img]: 2 * sum of kappa
    double* Lam;     // [n_img][9]
    double* scal;    // [S_COUNT]
};

// ------------------------------------------------------------------ setup: edges, components, remap, half-edge lists
// The components are reduce.hpp's union-find: a component's root is its lowest camera index.
__global__ void ra_init(Args a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < I_COUNT) a.icnt[i] = 0;
    if (i >= a.n_img) return;
    a.parent[i] = i;
    a.cnt[i] = 0;
    a.hase[i] = 0;
}

__global__ void ra_edge_use(Args a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    const int u = a.edges[2 * e], v = a.edges[2 * e + 1];
    bool ok = (!a.evalid || a.evalid[e]) && u >= 0 && u < a.n_img && v >= 0 && v < a.n_img && u != v;
    if (ok)
        for (int k = 0; k < 9; ++k) ok = ok && isfinite(a.aRb[9 * (size_t)e + k]);
    if (ok && a.kappa) ok = isfinite(a.kappa[e]) && a.kappa[e] > 0.0;
    a.use[e] = ok;
    if (!ok) return;
    a.hase[u] = 1;
    a.hase[v] = 1;
    uf_unite(a.parent, u, v);
}

__global__ void ra_comp_count(Args a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n_img || !a.hase[i]) return;
    atomicAdd(a.cnt + uf_find(a.parent, i), 1);
}

// the largest component (first maximum: the one holding the lowest camera index) and the consecutive remap
__global__ void ra_select(Args a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int best = -1, best_cnt = 0;
    for (int i = 0; i < a.n_img; ++i)
        if (a.cnt[i] > best_cnt) { best_cnt = a.cnt[i]; best = i; }
    int run = 0;
    for (int i = 0; i < a.n_img; ++i) {
        const bool k = best >= 0 && a.hase[i] && uf_find(a.parent, i) == best;
        a.keep[i] = k;
        a.newidx[i] = k ? run : -1;
        if (k) a.old[run++] = i;
    }
    a.icnt[I_NKEPT] = run;
}

__global__ void ra_edge_remap(Args a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    bool ok = a.use[e];
    if (ok) ok = a.keep[a.edges[2 * e]];
    a.use[e] = ok;
    a.rkey[2 * e] = ok ? a.newidx[a.edges[2 * e]] : -1;
    a.rkey[2 * e + 1] = ok ? a.newidx[a.edges[2 * e + 1]] : -1;
}

// csr.hpp source. Half-edge of edge (a, b, R, kappa): at a the neighbour b with block R', at b the neighbour a with
// block R, so that (V Q)_i = sum_h kappa_h (V_i - V_nbr(h) block_h)
struct HalfEdges {
    static constexpr int kKeys = 2;
    const uint8_t* use;
    const int* rkey;
    const double* aRb;
    const double* kappa;
    int* nbr;
    double* blk;
    __device__ bool keys(long long m, int* k) const {
        if (!use[m]) return false;
        k[0] = rkey[2 * m];
        k[1] = rkey[2 * m + 1];
        return true;
    }
    __device__ void put(long long m, const int* k, const size_t* slot) const {
        const double* R = aRb + 9 * (size_t)m;
        const double kap = kappa ? kappa[m] : 1.0;
        nbr[slot[0]] = k[1];
        nbr[slot[1]] = k[0];
        double* ba = blk + slot[0] * kEntry;
        double* bb = blk + slot[1] * kEntry;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                ba[3 * r + c] = R[3 * c + r];
                bb[3 * r + c] = R[3 * r + c];
            }
        ba[9] = kap;
        bb[9] = kap;
    }
};

__global__ void ra_degree(Args a, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int h = a.node_off[i]; h < a.node_off[i + 1]; ++h) d += a.blk[(size_t)h * kEntry + 9];
    a.D[i] = 2.0 * d;
}

// ------------------------------------------------------------------ the hot kernel: Out = V Q
__global__ __launch_bounds__(256) void ra_matvec(const int* __restrict__ node_off, const int* __restrict__ nbr,
                                                 const double* __restrict__ blk, const double* __restrict__ V,
                                                 double* __restrict__ out, int n, int p) {
    __shared__ double part[4][64][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int node = blockIdx.x * 4 + wave;
    const int ns = 64 / p;
    const int s = lane / p, r = lane - s * p;
    const bool live = node < n && s < ns;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    if (live) {
        const int b = node_off[node], e = node_off[node + 1];
        const double* yi = V + ((size_t)node * p + r) * 3;
        const double y0 = yi[0], y1 = yi[1], y2 = yi[2];
        for (int h = b + s; h < e; h += ns) {
            const double* m = blk + (size_t)h * kEntry;
            const double* yj = V + ((size_t)nbr[h] * p + r) * 3;
            const double z0 = yj[0], z1 = yj[1], z2 = yj[2], k = m[9];
            a0 += k * (y0 - (z0 * m[0] + z1 * m[3] + z2 * m[6]));
            a1 += k * (y1 - (z0 * m[1] + z1 * m[4] + z2 * m[7]));
            a2 += k * (y2 - (z0 * m[2] + z1 * m[5] + z2 * m[8]));
        }
    }
    part[wave][lane][0] = a0;
    part[wave][lane][1] = a1;
    part[wave][lane][2] = a2;
    __syncthreads();
    int width = 1;
    while (width < ns) width <<= 1;
    for (int st = width >> 1; st >= 1; st >>= 1) {
        if (live && s < st && s + st < ns) {
            part[wave][lane][0] += part[wave][lane + st * p][0];
            part[wave][lane][1] += part[wave][lane + st * p][1];
            part[wave][lane][2] += part[wave][lane + st * p][2];
        }
        __syncthreads();
    }
    if (live && s == 0) {
        double* o = out + ((size_t)node * p + r) * 3;
        o[0] = part[wave][lane][0];
        o[1] = part[wave][lane][1];
        o[2] = part[wave][lane][2];
    }
}

// ------------------------------------------------------------------ per-node kernels on [n][p][3]
// M (3 x 3) += u' v for 3-vectors u, v
__device__ __forceinline__ void outer_add(double* M, const double* u, const double* v) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] += u[i] * v[j];
}

// o = u M for a 3-vector u
__device__ __forceinline__ void row_mul(const double* u, const double* M, double* o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = u[0] * M[c] + u[1] * M[3 + c] + u[2] * M[6 + c];
}

__device__ __forceinline__ void symmetrise(double* M) {
    const double a = 0.5 * (M[1] + M[3]), b = 0.5 * (M[2] + M[6]), c = 0.5 * (M[5] + M[7]);
    M[1] = M[3] = a;
    M[2] = M[6] = b;
    M[5] = M[7] = c;
}

// (A'A)^-1/2 for the polar factor; a singular A gives non-finite entries, which the cost then reports
__device__ void inv_sqrt3(double* ata, double* Mi) {
    double w[3], V[9];
    jacobi_eig_reg<3>(reinterpret_cast<double(&)[9]>(*ata), w, V);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            Mi[3 * i + j] = V[3 * i] * V[3 * j] / sqrt(w[0]) + V[3 * i + 1] * V[3 * j + 1] / sqrt(w[1]) +
                            V[3 * i + 2] * V[3 * j + 2] / sqrt(w[2]);
}

// Lam_i = sym(Y_i' G_i), g = 2 (G - Y Lam)
__global__ void ra_lambda_grad(const double* Y, const double* G, double* Lam, double* g, int n, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* y = Y + (size_t)i * p * 3;
    const double* gq = G + (size_t)i * p * 3;
    double L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < p; ++r) outer_add(L, y + 3 * r, gq + 3 * r);
    symmetrise(L);
    for (int k = 0; k < 9; ++k) Lam[9 * (size_t)i + k] = L[k];
    if (!g) return;
    for (int r = 0; r < p; ++r) {
        double t[3];
        row_mul(y + 3 * r, L, t);
        for (int c = 0; c < 3; ++c) g[((size_t)i * p + r) * 3 + c] = 2.0 * (gq[3 * r + c] - t[c]);
    }
}

// q holds V Q on entry: q = 2 Proj_Y(V Q - V Lam) + lambda D V
__global__ void ra_hess(const double* Y, const double* Lam, const double* V, double* q, const double* D, double lambda,
                        int n, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* y = Y + (size_t)i * p * 3;
    const double* v = V + (size_t)i * p * 3;
    double* qi = q + (size_t)i * p * 3;
    const double* L = Lam + 9 * (size_t)i;
    double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < p; ++r) {
        double t[3], w[3];
        row_mul(v + 3 * r, L, t);
        for (int c = 0; c < 3; ++c) w[c] = qi[3 * r + c] - t[c];
        outer_add(S, y + 3 * r, w);
    }
    symmetrise(S);
    const double ld = lambda * D[i];
    for (int r = 0; r < p; ++r) {
        double t[3], u[3];
        row_mul(v + 3 * r, L, t);
        row_mul(y + 3 * r, S, u);
        for (int c = 0; c < 3; ++c) qi[3 * r + c] = 2.0 * ((qi[3 * r + c] - t[c]) - u[c]) + ld * v[3 * r + c];
    }
}

// Yn_i = polar factor of Y_i + X_i (X may be NULL)
__global__ void ra_retract(const double* Y, const double* X, double* Yn, int n, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* y = Y + (size_t)i * p * 3;
    const double* x = X ? X + (size_t)i * p * 3 : nullptr;
    double ata[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Mi[9];
    for (int r = 0; r < p; ++r) {
        double t[3];
        for (int c = 0; c < 3; ++c) t[c] = y[3 * r + c] + (x ? x[3 * r + c] : 0.0);
        outer_add(ata, t, t);
    }
    inv_sqrt3(ata, Mi);
    for (int r = 0; r < p; ++r) {
        double t[3], o[3];
        for (int c = 0; c < 3; ++c) t[c] = y[3 * r + c] + (x ? x[3 * r + c] : 0.0);
        row_mul(t, Mi, o);
        for (int c = 0; c < 3; ++c) Yn[((size_t)i * p + r) * 3 + c] = o[c];
    }
}

// Yn_i ((p + 1) x 3) = polar factor of [Y_i; alpha v_i]
__global__ void ra_lift(const double* Y, const double* v, double alpha, double* Yn, int n, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* y = Y + (size_t)i * p * 3;
    double last[3], ata[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Mi[9];
    for (int c = 0; c < 3; ++c) last[c] = alpha * v[3 * (size_t)i + c];
    for (int r = 0; r < p; ++r) outer_add(ata, y + 3 * r, y + 3 * r);
    outer_add(ata, last, last);
    inv_sqrt3(ata, Mi);
    for (int r = 0; r <= p; ++r) {
        double o[3];
        row_mul(r < p ? y + 3 * r : last, Mi, o);
        for (int c = 0; c < 3; ++c) Yn[((size_t)i * (p + 1) + r) * 3 + c] = o[c];
    }
}

// the initial point at level p: [wRi_init; 0] or the seeded rotation, through the polar factor
__global__ void ra_start(Args a, double* Y, double* tmp, int n, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int cam = a.old[i];
    double R[9];
    if (a.init) {
        for (int k = 0; k < 9; ++k) R[k] = a.init[9 * (size_t)cam + k];
    } else {
        const uint64_t base = sm_mix(a.seed ^ sm_mix((uint64_t)(uint32_t)cam));
        double A[9], ata[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Mi[9];
        for (int k = 0; k < 9; ++k) A[k] = 2.0 * ((double)(sm_mix(base + (uint64_t)k) >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
        for (int r = 0; r < 3; ++r) outer_add(ata, A + 3 * r, A + 3 * r);
        inv_sqrt3(ata, Mi);
        for (int r = 0; r < 3; ++r) row_mul(A + 3 * r, Mi, R + 3 * r);
        if (det3(R) < 0.0) { R[2] = -R[2]; R[5] = -R[5]; R[8] = -R[8]; }
    }
    double* t = tmp + (size_t)i * p * 3;
    for (int k = 0; k < 3 * p; ++k) t[k] = k < 9 ? R[k] : 0.0;
}

// ------------------------------------------------------------------ one-workgroup reductions, fixed order
__device__ double block_sum(double v, double* sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = kRedBlock / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

__device__ double block_dot(const double* a, const double* b, size_t N, double* sh) {
    double acc = 0.0;
    for (size_t k = threadIdx.x; k < N; k += kRedBlock) acc += a[k] * b[k];
    return block_sum(acc, sh);
}

__global__ __launch_bounds__(kRedBlock) void ra_dot(const double* a, const double* b, size_t N, double* dst) {
    __shared__ double sh[kRedBlock];
    const double d = block_dot(a, b, N, sh);
    if (threadIdx.x == 0) *dst = d;
}

// x = 0, r = -g, pv = r / (D (1 + lambda)); rz, rr
__global__ __launch_bounds__(kRedBlock) void ra_pcg_init(const double* g, const double* D, double lambda, double* x,
                                                         double* r, double* pv, size_t N, int p3, double* scal) {
    __shared__ double sh[kRedBlock];
    double rz = 0.0, rr = 0.0;
    for (size_t k = threadIdx.x; k < N; k += kRedBlock) {
        const double rk = -g[k], z = rk / (D[k / p3] * (1.0 + lambda));
        x[k] = 0.0;
        r[k] = rk;
        pv[k] = z;
        rz += rk * z;
        rr += rk * rk;
    }
    rz = block_sum(rz, sh);
    rr = block_sum(rr, sh);
    if (threadIdx.x == 0) { scal[S_RZ] = rz; scal[S_RR] = rr; scal[S_NEG] = 0.0; }
}

// one conjugate-gradient step; on non-positive curvature: x = pv when first, and nothing else changes
__global__ __launch_bounds__(kRedBlock) void ra_pcg_step(const double* D, double lambda, double* x, double* r,
                                                         double* pv, const double* q, size_t N, int p3, int first,
                                                         double* scal) {
    __shared__ double sh[kRedBlock];
    const double pq = block_dot(pv, q, N, sh);
    const double rz = scal[S_RZ];
    if (!(pq > 0.0)) {
        if (first)
            for (size_t k = threadIdx.x; k < N; k += kRedBlock) x[k] = pv[k];
        if (threadIdx.x == 0) scal[S_NEG] = 1.0;
        return;
    }
    const double alpha = rz / pq;
    double rz2 = 0.0, rr = 0.0;
    for (size_t k = threadIdx.x; k < N; k += kRedBlock) {
        x[k] = x[k] + alpha * pv[k];
        const double rk = r[k] - alpha * q[k];
        r[k] = rk;
        const double z = rk / (D[k / p3] * (1.0 + lambda));
        rz2 += rk * z;
        rr += rk * rk;
    }
    rz2 = block_sum(rz2, sh);
    rr = block_sum(rr, sh);
    const double beta = rz2 / rz;
    for (size_t k = threadIdx.x; k < N; k += kRedBlock)
        pv[k] = r[k] / (D[k / p3] * (1.0 + lambda)) + beta * pv[k];
    __syncthreads();
    if (threadIdx.x == 0) { scal[S_RZ] = rz2; scal[S_RR] = rr; }
}

// <g, x>, <x, q>, sum_i D_i |x_i|^2
__global__ __launch_bounds__(kRedBlock) void ra_model(const double* g, const double* x, const double* q, const double* D,
                                                      size_t N, int p3, double* scal) {
    __shared__ double sh[kRedBlock];
    double gx = 0.0, xq = 0.0, xdx = 0.0;
    for (size_t k = threadIdx.x; k < N; k += kRedBlock) {
        gx += g[k] * x[k];
        xq += x[k] * q[k];
        xdx += D[k / p3] * (x[k] * x[k]);
    }
    gx = block_sum(gx, sh);
    xq = block_sum(xq, sh);
    xdx = block_sum(xdx, sh);
    if (threadIdx.x == 0) { scal[S_GX] = gx; scal[S_XQ] = xq; scal[S_XDX] = xdx; }
}

// ------------------------------------------------------------------ the certificate: Lanczos on S = Q - blockdiag(Lam)
__global__ void ra_lz_seed(Args a, double* w, int n, int salt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t base = sm_mix(a.seed ^ sm_mix((uint64_t)(uint32_t)a.old[i]));
    for (int c = 0; c < 3; ++c)
        w[3 * (size_t)i + c] = 2.0 * ((double)(sm_mix(base + (uint64_t)(16 + 3 * salt + c)) >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
}

// w_i -= v_i Lam_i (w holds v Q)
__global__ void ra_sub_lambda(const double* Lam, const double* v, double* w, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double t[3];
    row_mul(v + 3 * (size_t)i, Lam + 9 * (size_t)i, t);
    for (int c = 0; c < 3; ++c) w[3 * (size_t)i + c] -= t[c];
}

// c[j] = <V_j, w>, one workgroup per basis vector
__global__ __launch_bounds__(kRedBlock) void ra_lz_dots(const double* V, const double* w, size_t N, double* c,
                                                        double* alpha_dst) {
    __shared__ double sh[kRedBlock];
    const double d = block_dot(V + (size_t)blockIdx.x * N, w, N, sh);
    if (threadIdx.x == 0) {
        c[blockIdx.x] = d;
        if (alpha_dst && blockIdx.x == gridDim.x - 1) *alpha_dst = d;
    }
}

// w -= sum_j c[j] V_j, j ascending
__global__ void ra_lz_sub(const double* V, double* w, size_t N, const double* c, int nv) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    double acc = w[k];
    for (int j = 0; j < nv; ++j) acc -= c[j] * V[(size_t)j * N + k];
    w[k] = acc;
}

// dst = w / |w|, *norm = |w|
__global__ __launch_bounds__(kRedBlock) void ra_normalise(const double* w, double* dst, size_t N, double* norm) {
    __shared__ double sh[kRedBlock];
    const double nn = sqrt(block_dot(w, w, N, sh));
    for (size_t k = threadIdx.x; k < N; k += kRedBlock) dst[k] = w[k] / nn;
    if (threadIdx.x == 0) *norm = nn;
}

struct Coef { double s[kLanczosMax]; };

// v = sum_j s[j] V_j, j ascending
__global__ void ra_lz_combine(const double* V, double* v, size_t N, Coef s, int nv) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= N) return;
    double acc = 0.0;
    for (int j = 0; j < nv; ++j) acc += s.s[j] * V[(size_t)j * N + k];
    v[k] = acc;
}

// |w - theta v|
__global__ __launch_bounds__(kRedBlock) void ra_resid(const double* w, const double* v, double theta, size_t N,
                                                      double* dst) {
    __shared__ double sh[kRedBlock];
    double acc = 0.0;
    for (size_t k = threadIdx.x; k < N; k += kRedBlock) {
        const double d = w[k] - theta * v[k];
        acc += d * d;
    }
    acc = block_sum(acc, sh);
    if (threadIdx.x == 0) *dst = sqrt(acc);
}

// ------------------------------------------------------------------ rounding
// M[a][b] = sum_i Y_i[a] . Y_i[b], i ascending: the p x p Gram matrix of the p x 3n matrix Y
__global__ void ra_gram(const double* Y, double* M, int n, int p) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p * p) return;
    const int ra = t / p, rb = t - ra * p;
    double acc = 0.0;
    for (int i = 0; i < n; ++i) {
        const double* u = Y + ((size_t)i * p + ra) * 3;
        const double* v = Y + ((size_t)i * p + rb) * 3;
        acc += u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    }
    M[t] = acc;
}

struct Basis { double U[3 * kPMax]; };  // U[k][r]: direction k, row r

__global__ void ra_round_blocks(const double* Y, Basis u, double* B, int* icnt, int n, int p) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double b[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = 0; r < p; ++r) {
        const double* y = Y + ((size_t)i * p + r) * 3;
        for (int k = 0; k < 3; ++k)
            for (int c = 0; c < 3; ++c) b[3 * k + c] += u.U[k * kPMax + r] * y[c];
    }
    for (int k = 0; k < 9; ++k) B[9 * (size_t)i + k] = b[k];
    if (det3(b) < 0.0) atomicAdd(icnt + I_NEG, 1);
}

__global__ void ra_round_out(Args a, const double* B, double* wRi, uint8_t* rot_valid, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double b[9], U[9], s[3], V[9], R[9];
    for (int k = 0; k < 9; ++k) b[k] = B[9 * (size_t)i + k];
    if (2 * a.icnt[I_NEG] > n) { b[6] = -b[6]; b[7] = -b[7]; b[8] = -b[8]; }
    // svd3 completes U and V by cross products, so both are proper rotations and U V' is the closest rotation to b
    // whatever the sign of det(b): the flip of the smallest direction is already in their third columns
    svd3(b, U, s, V);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + U[3 * r + 2] * V[3 * c + 2];
    const int cam = a.old[i];
    for (int k = 0; k < 9; ++k) wRi[9 * (size_t)cam + k] = R[k];
    rot_valid[cam] = 1;
}

// ------------------------------------------------------------------ host helpers
// cyclic Jacobi on a dense symmetric n x n matrix (row-major, destroyed); eigenvalues w, eigenvectors the columns of V
void host_jacobi(double* A, int n, double* w, double* V) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) V[i * n + j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < n; ++i) {
            diag += A[i * n + i] * A[i * n + i];
            for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
        }
        if (off <= 1e-32 * diag || off == 0.0) break;
        for (int p = 0; p < n; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A[p * n + q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < n; ++k) {
                    const double akp = A[k * n + p], akq = A[k * n + q];
                    A[k * n + p] = c * akp - s * akq;
                    A[k * n + q] = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {
                    const double apk = A[p * n + k], aqk = A[q * n + k];
                    A[p * n + k] = c * apk - s * aqk;
                    A[q * n + k] = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = V[k * n + p], vkq = V[k * n + q];
                    V[k * n + p] = c * vkp - s * vkq;
                    V[k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < n; ++i) w[i] = A[i * n + i];
}

struct Layout {
    size_t use, parent, cnt, hase, keep, newidx, old, icnt, rkey, node_off, hist, nbr, blk, D, Lam, scal, vec, basis, lw,
        lv, lc, gram, B, total;
    CsrChunks chunks;
};

constexpr int kVecs = 9;  // Y, Yn, G, Gn, g, x, r, pv, q

Layout layout(int E, int n_img, int p_max) {
    Layout L;
    L.chunks = csr_chunks(E, kChunksMax);
    WsCarver w;
    const size_t e = (size_t)E, n = (size_t)n_img, d = sizeof(double);
    L.use = w.take(e);
    L.parent = w.take(n * 4);
    L.cnt = w.take(n * 4);
    L.hase = w.take(n);
    L.keep = w.take(n);
    L.newidx = w.take(n * 4);
    L.old = w.take(n * 4);
    L.icnt = w.take(I_COUNT * 4);
    L.rkey = w.take(e * 8);
    L.node_off = w.take((n + 1) * 4);
    L.hist = w.take(csr_hist_bytes(L.chunks, n));
    L.nbr = w.take(2 * e * 4);
    L.blk = w.take(2 * e * kEntry * d);
    L.D = w.take(n * d);
    L.Lam = w.take(n * 9 * d);
    L.scal = w.take(S_COUNT * d);
    L.vec = w.take((size_t)kVecs * n * p_max * 3 * d);
    L.basis = w.take((size_t)(kLanczosMax + 1) * n * 3 * d);
    L.lw = w.take(n * 3 * d);
    L.lv = w.take(n * 3 * d);
    L.lc = w.take((kLanczosMax + 1) * d);
    L.gram = w.take((size_t)kPMax * kPMax * d);
    L.B = w.take(n * 9 * d);
    L.total = w.o;
    return L;
}

bool sizes_ok(int n_edges, int n_img, int p_max) {
    return n_edges > 0 && n_edges < (1 << 30) && n_img > 0 && n_img <= (1 << 20) && p_max >= 3 && p_max <= kPMax;
}

}  // namespace

extern "C" {

size_t gtsfm_rotavg_workspace_bytes(int n_edges, int n_img, int p_max) {
    if (!sizes_ok(n_edges, n_img, p_max)) return 0;
    return layout(n_edges, n_img, p_max).total;
}

int gtsfm_rotavg_shonan(const int* d_edges, const double* d_aRb, const double* d_kappa, const uint8_t* d_edge_valid,
                        int n_edges, int n_img, const double* d_wRi_init, uint64_t seed, int p_min, int p_max,
                        double optimality_threshold, double grad_rel_tol, int max_iterations, double pcg_rel_tol,
                        int pcg_max_iter, double eig_tol, int eig_max_steps, void* d_workspace, size_t workspace_bytes,
                        double* d_wRi, uint8_t* d_rot_valid, double* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (p_min < 3 || p_max < p_min || !sizes_ok(n_edges, n_img, p_max) || !d_edges || !d_aRb || !d_workspace || !d_wRi ||
        !d_rot_valid || !d_stats || !isfinite(optimality_threshold) || !(grad_rel_tol > 0) || max_iterations <= 0 ||
        !(pcg_rel_tol > 0) || pcg_max_iter <= 0 || !(eig_tol > 0) || eig_max_steps <= 0)
        return GTSFM_ERR_ARG;
    const Layout L = layout(n_edges, n_img, p_max);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    Args a;
    a.edges = d_edges; a.aRb = d_aRb; a.kappa = d_kappa; a.evalid = d_edge_valid; a.init = d_wRi_init;
    a.E = n_edges; a.n_img = n_img; a.chunks = L.chunks; a.seed = seed;
    a.use = ws + L.use; a.parent = (int*)(ws + L.parent); a.cnt = (int*)(ws + L.cnt); a.hase = ws + L.hase;
    a.keep = ws + L.keep; a.newidx = (int*)(ws + L.newidx); a.old = (int*)(ws + L.old); a.icnt = (int*)(ws + L.icnt);
    a.rkey = (int*)(ws + L.rkey); a.node_off = (int*)(ws + L.node_off); a.hist = (int*)(ws + L.hist);
    a.nbr = (int*)(ws + L.nbr); a.blk = (double*)(ws + L.blk); a.D = (double*)(ws + L.D);
    a.Lam = (double*)(ws + L.Lam); a.scal = (double*)(ws + L.scal);
    double* vec = (double*)(ws + L.vec);
    const size_t vstride = (size_t)n_img * p_max * 3;
    double *Y = vec, *Yn = vec + vstride, *G = vec + 2 * vstride, *Gn = vec + 3 * vstride, *g = vec + 4 * vstride,
           *x = vec + 5 * vstride, *r = vec + 6 * vstride, *pv = vec + 7 * vstride, *q = vec + 8 * vstride;
    double* basis = (double*)(ws + L.basis);
    double* lw = (double*)(ws + L.lw);
    double* lv = (double*)(ws + L.lv);
    double* lc = (double*)(ws + L.lc);
    double* gram = (double*)(ws + L.gram);
    double* Bk = (double*)(ws + L.B);

    const unsigned B = 256;
    const unsigned gE = blocks_for(n_edges, B), gI = blocks_for(n_img, B);
    int icnt[I_COUNT];
    double scal[S_COUNT];
    auto read_scal = [&]() { return read_back(scal, a.scal, S_COUNT, stream); };
    int rc;
    GTSFM_CHECK_HIP(hipMemsetAsync(d_wRi, 0, (size_t)n_img * 9 * sizeof(double), stream));
    GTSFM_CHECK_HIP(hipMemsetAsync(d_rot_valid, 0, (size_t)n_img, stream));
    hipLaunchKernelGGL(ra_init, dim3(gI), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(ra_edge_use, dim3(gE), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(ra_comp_count, dim3(gI), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(ra_select, dim3(1), dim3(64), 0, stream, a);
    hipLaunchKernelGGL(ra_edge_remap, dim3(gE), dim3(B), 0, stream, a);
    if ((rc = csr_build(HalfEdges{a.use, a.rkey, a.aRb, a.kappa, a.nbr, a.blk}, n_edges, n_img, a.chunks, a.hist,
                        a.node_off, stream)) != GTSFM_OK)
        return rc;
    GTSFM_CHECK_HIP(hipMemcpyAsync(icnt, a.icnt, sizeof(icnt), hipMemcpyDeviceToHost, stream));
    int half_edges = 0;
    GTSFM_CHECK_HIP(hipMemcpyAsync(&half_edges, a.node_off + n_img, sizeof(int), hipMemcpyDeviceToHost, stream));
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    const int n = icnt[I_NKEPT];
    double stats[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n == 0) {
        stats[11] = 1.0;
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_stats, stats, sizeof(stats), hipMemcpyHostToDevice, stream));
        GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
        return GTSFM_OK;
    }
    const unsigned gN = blocks_for(n, B), gW = blocks_for(n, 4);
    auto matvec = [&](const double* V, double* out, int p) {
        hipLaunchKernelGGL(ra_matvec, dim3(gW), dim3(256), 0, stream, a.node_off, a.nbr, a.blk, V, out, n, p);
    };
    // cost tr(V Q V') = <V, V Q>, with V Q left in `out`
    auto cost = [&](const double* V, double* out, int p, double* f) -> int {
        matvec(V, out, p);
        hipLaunchKernelGGL(ra_dot, dim3(1), dim3(kRedBlock), 0, stream, V, out, (size_t)n * p * 3, a.scal + S_DOT);
        GTSFM_CHECK_HIP(hipGetLastError());
        int rc2 = read_scal();
        *f = scal[S_DOT];
        return rc2;
    };
    hipLaunchKernelGGL(ra_degree, dim3(gN), dim3(B), 0, stream, a, n);
    hipLaunchKernelGGL(ra_dot, dim3(1), dim3(kRedBlock), 0, stream, a.D, a.D, (size_t)n, a.scal + S_D2);
    int p = p_min;
    hipLaunchKernelGGL(ra_start, dim3(gN), dim3(B), 0, stream, a, Y, Yn, n, p);
    hipLaunchKernelGGL(ra_retract, dim3(gN), dim3(B), 0, stream, Yn, (const double*)nullptr, Y, n, p);
    double f = 0.0;
    if ((rc = cost(Y, G, p, &f)) != GTSFM_OK) return rc;
    const double G0 = sqrt(3.0 * scal[S_D2]), f0 = f;
    long long outer = 0, pcg_total = 0, cap_hits = 0, lz_steps = 0;
    double status = 2.0, theta = 0.0, resid = 0.0;
    bool bad = !isfinite(f);

    while (!bad) {
        // ---- Riemannian LM at level p; Y, G = Y Q and f are current
        const size_t N = (size_t)n * p * 3;
        const int p3 = p * 3;
        double lambda = kLambdaInitial, nu = kLambdaFactor;
        for (int it = 0; it < max_iterations && !bad; ++it) {
            hipLaunchKernelGGL(ra_lambda_grad, dim3(gN), dim3(B), 0, stream, Y, G, a.Lam, g, n, p);
            hipLaunchKernelGGL(ra_dot, dim3(1), dim3(kRedBlock), 0, stream, g, g, N, a.scal + S_DOT);
            GTSFM_CHECK_HIP(hipGetLastError());
            if ((rc = read_scal()) != GTSFM_OK) return rc;
            if (!isfinite(scal[S_DOT])) { bad = true; break; }
            if (sqrt(scal[S_DOT]) <= grad_rel_tol * G0) break;
            bool accepted = false;
            while (lambda <= kLambdaUpper) {
                hipLaunchKernelGGL(ra_pcg_init, dim3(1), dim3(kRedBlock), 0, stream, g, a.D, lambda, x, r, pv, N, p3,
                                   a.scal);
                GTSFM_CHECK_HIP(hipGetLastError());
                if ((rc = read_scal()) != GTSFM_OK) return rc;
                const double bb = scal[S_RR];
                double rr = bb;
                int k = 0;
                while (!(sqrt(rr) <= pcg_rel_tol * sqrt(bb))) {
                    if (k >= pcg_max_iter) {
                        ++cap_hits;
                        break;
                    }
                    matvec(pv, q, p);
                    hipLaunchKernelGGL(ra_hess, dim3(gN), dim3(B), 0, stream, Y, a.Lam, pv, q, a.D, lambda, n, p);
                    hipLaunchKernelGGL(ra_pcg_step, dim3(1), dim3(kRedBlock), 0, stream, a.D, lambda, x, r, pv, q, N, p3,
                                       k == 0 ? 1 : 0, a.scal);
                    GTSFM_CHECK_HIP(hipGetLastError());
                    if ((rc = read_scal()) != GTSFM_OK) return rc;
                    ++k;
                    if (scal[S_NEG] != 0.0) break;
                    rr = scal[S_RR];
                }
                pcg_total += k;
                matvec(x, q, p);
                hipLaunchKernelGGL(ra_hess, dim3(gN), dim3(B), 0, stream, Y, a.Lam, x, q, a.D, lambda, n, p);
                hipLaunchKernelGGL(ra_model, dim3(1), dim3(kRedBlock), 0, stream, g, x, q, a.D, N, p3, a.scal);
                hipLaunchKernelGGL(ra_retract, dim3(gN), dim3(B), 0, stream, Y, x, Yn, n, p);
                double fn = 0.0;
                if ((rc = cost(Yn, Gn, p, &fn)) != GTSFM_OK) return rc;
                if (!isfinite(fn)) { bad = true; break; }
                const double model = -scal[S_GX] - 0.5 * (scal[S_XQ] - lambda * scal[S_XDX]);
                const double rho = model > 0.0 ? (f - fn) / model : -1.0;
                if (rho > kMinFidelity && fn < f) {
                    double* t = Y; Y = Yn; Yn = t;
                    t = G; G = Gn; Gn = t;
                    f = fn;
                    const double c = 2.0 * rho - 1.0;
                    double shrink = 1.0 - c * c * c;
                    if (shrink < 1.0 / 3.0) shrink = 1.0 / 3.0;
                    lambda *= shrink;
                    if (lambda < kLambdaLower) lambda = kLambdaLower;
                    nu = kLambdaFactor;
                    ++outer;
                    accepted = true;
                    break;
                }
                lambda *= nu;
                nu *= 2.0;
            }
            if (!accepted) break;
        }
        if (bad) break;

        // ---- certificate: the smallest eigenpair of S = Q - blockdiag(Lam) by Lanczos with full reorthogonalisation
        hipLaunchKernelGGL(ra_lambda_grad, dim3(gN), dim3(B), 0, stream, Y, G, a.Lam, (double*)nullptr, n, p);
        const size_t N3 = (size_t)n * 3;
        const unsigned g3 = blocks_for(N3, B);
        const int m = (size_t)kLanczosMax < N3 ? kLanczosMax : (int)N3;
        auto apply_S = [&](const double* v, double* w) {
            matvec(v, w, 1);
            hipLaunchKernelGGL(ra_sub_lambda, dim3(gN), dim3(B), 0, stream, a.Lam, v, w, n);
        };
        hipLaunchKernelGGL(ra_lz_seed, dim3(gN), dim3(B), 0, stream, a, lw, n, p);
        hipLaunchKernelGGL(ra_normalise, dim3(1), dim3(kRedBlock), 0, stream, lw, basis, N3, a.scal + S_BETA);
        double al[kLanczosMax], be[kLanczosMax];
        static thread_local double T[kLanczosMax * kLanczosMax], TV[kLanczosMax * kLanczosMax], tw[kLanczosMax];
        bool done = false;
        while (!done) {
            int k = 0;
            double scale = 0.0;
            bool restart = false;
            while (!restart && !done) {
                double* vk = basis + (size_t)k * N3;
                apply_S(vk, lw);
                for (int pass = 0; pass < 2; ++pass) {
                    hipLaunchKernelGGL(ra_lz_dots, dim3(k + 1), dim3(kRedBlock), 0, stream, basis, lw, N3, lc,
                                       pass == 0 ? a.scal + S_ALPHA : (double*)nullptr);
                    hipLaunchKernelGGL(ra_lz_sub, dim3(g3), dim3(B), 0, stream, basis, lw, N3, lc, k + 1);
                }
                hipLaunchKernelGGL(ra_normalise, dim3(1), dim3(kRedBlock), 0, stream, lw, basis + (size_t)(k + 1) * N3, N3,
                                   a.scal + S_BETA);
                GTSFM_CHECK_HIP(hipGetLastError());
                if ((rc = read_scal()) != GTSFM_OK) return rc;
                al[k] = scal[S_ALPHA];
                be[k] = scal[S_BETA];
                if (!isfinite(al[k]) || !isfinite(be[k])) { bad = true; done = true; break; }
                if (fabs(al[k]) > scale) scale = fabs(al[k]);
                const bool breakdown = !(be[k] > 1e-12 * (scale > 1.0 ? scale : 1.0));
                if (!breakdown && be[k] > scale) scale = be[k];
                ++k;
                ++lz_steps;
                const bool capped = lz_steps >= eig_max_steps;
                if (!(breakdown || capped || k == m || k == 16 || k == 32 || k == 64)) continue;
                for (int i = 0; i < k * k; ++i) T[i] = 0.0;
                for (int i = 0; i < k; ++i) {
                    T[i * k + i] = al[i];
                    if (i + 1 < k) T[i * k + i + 1] = T[(i + 1) * k + i] = be[i];
                }
                host_jacobi(T, k, tw, TV);
                int lo = 0;
                for (int i = 1; i < k; ++i)
                    if (tw[i] < tw[lo]) lo = i;
                const double est = fabs(be[k - 1] * TV[(k - 1) * k + lo]);
                if (!(breakdown || capped || k == m || est <= eig_tol)) continue;
                Coef s;
                for (int i = 0; i < k; ++i) s.s[i] = TV[i * k + lo];
                hipLaunchKernelGGL(ra_lz_combine, dim3(g3), dim3(B), 0, stream, basis, lv, N3, s, k);
                hipLaunchKernelGGL(ra_normalise, dim3(1), dim3(kRedBlock), 0, stream, lv, lv, N3, a.scal + S_BETA);
                apply_S(lv, lw);
                hipLaunchKernelGGL(ra_dot, dim3(1), dim3(kRedBlock), 0, stream, lv, lw, N3, a.scal + S_DOT);
                GTSFM_CHECK_HIP(hipGetLastError());
                if ((rc = read_scal()) != GTSFM_OK) return rc;
                theta = scal[S_DOT];  // the Rayleigh quotient of the normalised Ritz vector
                hipLaunchKernelGGL(ra_resid, dim3(1), dim3(kRedBlock), 0, stream, lw, lv, theta, N3, a.scal + S_DOT);
                GTSFM_CHECK_HIP(hipGetLastError());
                if ((rc = read_scal()) != GTSFM_OK) return rc;
                resid = scal[S_DOT];
                if (resid <= eig_tol || capped) {
                    done = true;
                } else {
                    GTSFM_CHECK_HIP(hipMemcpyAsync(basis, lv, N3 * sizeof(double), hipMemcpyDeviceToDevice, stream));
                    restart = true;
                }
            }
        }
        if (bad) break;
        if (theta > optimality_threshold) {
            status = 0.0;
            break;
        }
        if (p >= p_max) break;

        // ---- lift to p + 1 along e_{p+1} v', halving the step from max(1024 alphaMin, 0.1 / |theta|)
        double alpha = 1024.0 * kAlphaMin;
        if (0.1 / fabs(theta) > alpha) alpha = 0.1 / fabs(theta);
        for (;;) {
            hipLaunchKernelGGL(ra_lift, dim3(gN), dim3(B), 0, stream, Y, lv, alpha, Yn, n, p);
            double ft = 0.0;
            if ((rc = cost(Yn, Gn, p + 1, &ft)) != GTSFM_OK) return rc;
            if (!isfinite(ft)) { bad = true; break; }
            if (ft < f || alpha / 2.0 < kAlphaMin) {
                f = ft;
                break;
            }
            alpha /= 2.0;
        }
        double* t = Y; Y = Yn; Yn = t;
        t = G; G = Gn; Gn = t;
        ++p;
    }

    if (bad) {
        status = 3.0;
    } else {
        // ---- rounding: the three dominant directions of Y, the sign, the closest rotations
        hipLaunchKernelGGL(ra_gram, dim3(blocks_for((size_t)p * p, B)), dim3(B), 0, stream, Y, gram, n, p);
        double M[kPMax * kPMax], MV[kPMax * kPMax], mw[kPMax];
        GTSFM_CHECK_HIP(hipMemcpyAsync(M, gram, (size_t)p * p * sizeof(double), hipMemcpyDeviceToHost, stream));
        GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
        host_jacobi(M, p, mw, MV);
        Basis u;
        bool taken[kPMax] = {false};
        for (int k = 0; k < 3; ++k) {
            int hi = -1;
            for (int i = 0; i < p; ++i)
                if (!taken[i] && (hi < 0 || mw[i] > mw[hi])) hi = i;
            taken[hi] = true;
            for (int rr = 0; rr < kPMax; ++rr) u.U[k * kPMax + rr] = rr < p ? MV[rr * p + hi] : 0.0;
        }
        hipLaunchKernelGGL(ra_round_blocks, dim3(gN), dim3(B), 0, stream, Y, u, Bk, a.icnt, n, p);
        hipLaunchKernelGGL(ra_round_out, dim3(gN), dim3(B), 0, stream, a, Bk, d_wRi, d_rot_valid, n);
        GTSFM_CHECK_HIP(hipGetLastError());
    }
    stats[0] = f0; stats[1] = f; stats[2] = (double)p; stats[3] = theta; stats[4] = resid; stats[5] = (double)outer;
    stats[6] = (double)pcg_total; stats[7] = (double)cap_hits; stats[8] = (double)lz_steps;
    stats[9] = bad ? 0.0 : (double)n; stats[10] = (double)(half_edges / 2); stats[11] = status;
    GTSFM_CHECK_HIP(hipMemcpyAsync(d_stats, stats, sizeof(stats), hipMemcpyHostToDevice, stream));
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    return GTSFM_OK;
}

}  // extern "C"
