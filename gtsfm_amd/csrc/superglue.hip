// SuperGlue matcher on gfx950: thirdparty/SuperGluePretrainedNetwork/models/superglue.py:228-283 as driven by
// gtsfm/frontend/matcher/superglue_matcher.py:43-111 (20 Sinkhorn iterations, match threshold 0.2), batched over
// image pairs.
//
//   keypoint normalisation + MLP encoder (with eval BatchNorm) -> 18 x {self, cross} attentional propagation
//   (4-head attention d = 256, MLP 512 -> 512 -> 256, residual) -> final projection -> scores / 16
//   -> log-space optimal transport with a dustbin -> mutual argmax + threshold.
//
// Layout: every (pair, side) owns a kmax x C row-major (point-major) feature block, so each 1x1 Conv1d is a
// batched GEMM  Y[n][co] = sum_ci X[n][ci] W^T[ci][co]  on the bf16 matrix cores at near-fp32 accuracy (three-plane
// split, six products: sg_gemm3_kernel). Differences from the fp32 torch reference come from: summation order; the
// three dropped plane products (each below 2^-23 |a b|); exp taken as v_exp_f32 of x log2(e) in the attention and
// Sinkhorn kernels (the product's rounding gives a relative error of about |x| 2^-24). tests/test_superglue_gpu.py
// bounds the result: log-assignment within 2e-3 of the reference module, matches equal up to near-ties. Heads
// are stored head-major (channel h * 64 + d; the reference's view(b, 64, 4, n) interleaves them as 4 d + h — the
// host packs the q/k/v/merge weights accordingly). Attention is one fused kernel (online softmax on the same split
// products): the K1 x K2 probability matrix never reaches HBM. The Sinkhorn matrix (K1 + 1) x (K2 + 1) does, once
// per pair.
#include "sg_kernels.hpp"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ packed weights (include/gtsfm_hip.h)
// GEMM weights are W^T[cin][cout] row-major. Encoder layers: W^T (cin_pad x cout), bias, bn_scale, bn_shift
// (the last encoder layer has no BN). GNN layer: Wqkv^T (256 x 768, columns [q | k | v], head-major), bqkv,
// Wm^T (256 x 256, rows head-major), bm, W1^T (512 x 512: rows 0..255 act on x, 256..511 on the message), b1,
// bn1 scale, bn1 shift, W2^T (512 x 256), b2. Then final_proj W^T (256 x 256), bias, and bin_score (1 float).
constexpr int kEncIn[5] = {16, 32, 64, 128, 256};  // cin (the 3 encoder inputs zero-padded to 16)
constexpr int kEncOut[5] = {32, 64, 128, 256, 256};

__host__ __device__ constexpr size_t enc_floats(int i) {
    return (size_t)kEncIn[i] * kEncOut[i] + kEncOut[i] + (i < 4 ? 2 * kEncOut[i] : 0);
}
__host__ __device__ constexpr size_t enc_total() {
    size_t o = 0;
    for (int i = 0; i < 5; ++i) o += enc_floats(i);
    return o;
}
constexpr size_t kLayerFloats = (size_t)256 * 768 + 768 + 256 * 256 + 256 + 512 * 512 + 512 * 3 + 512 * 256 + 256;
__host__ __device__ constexpr size_t sg_weights_floats(int n_layers) {
    return enc_total() + (size_t)n_layers * kLayerFloats + 256 * 256 + 256 + 1;
}

// ------------------------------------------------------------------ encoder input and descriptor init
// superglue.py:64-71 normalize_keypoints: (kpts - size / 2) / (max(W, H) * 0.7), size = (W, H); the encoder input is
// (x_n, y_n, score) (:79-81), zero-padded to 16 channels. X <- descriptors (rows >= count zeroed).
__global__ void sg_prepare_kernel(const float* __restrict__ kp, const float* __restrict__ scores,
                                  const float* __restrict__ desc, const int* __restrict__ counts,
                                  const int* __restrict__ hw, const int* __restrict__ pairs, int kmax,
                                  float* __restrict__ enc_in /*(2P, kmax, 16)*/, float* __restrict__ X,
                                  int* __restrict__ side_counts) {
    const int zs = blockIdx.y;
    const int img = pairs[zs];
    const int n = counts[img];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && threadIdx.x == 0) side_counts[zs] = n;
    if (i >= kmax) return;
    float* e = enc_in + ((long)zs * kmax + i) * 16;
    float* x = X + ((long)zs * kmax + i) * kD;
    const float* d = desc + ((long)img * kmax + i) * kD;
    if (i < n) {
        const float W = (float)hw[2 * img + 1], H = (float)hw[2 * img];
        const float scaling = fmaxf(W, H) * 0.7f;
        e[0] = (kp[((long)img * kmax + i) * 2] - W / 2.0f) / scaling;
        e[1] = (kp[((long)img * kmax + i) * 2 + 1] - H / 2.0f) / scaling;
        e[2] = scores[(long)img * kmax + i];
        for (int c = 0; c < kD; ++c) x[c] = d[c];
    } else {
        e[0] = e[1] = e[2] = 0.0f;
        for (int c = 0; c < kD; ++c) x[c] = 0.0f;
    }
    for (int c = 3; c < 16; ++c) e[c] = 0.0f;
}

// ------------------------------------------------------------------ log-space optimal transport
// superglue.py:114-145 with iters = 20: couplings [[S, alpha], [alpha, alpha]], norm = -log(m + n),
// log_mu = [norm] * m + [log(n) + norm], log_nu = [norm] * n + [log(m) + norm],
// u = log_mu - logsumexp(Z + v, 2), v = log_nu - logsumexp(Z + u, 1); result Z + u + v - norm.
__global__ void sk_init_kernel(float* __restrict__ Z, const int* __restrict__ side_counts, int kmax,
                               const float* __restrict__ bin_score, float* __restrict__ u, float* __restrict__ v) {
    const int p = blockIdx.y;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const long ld = kmax + 1;
    float* Zp = Z + (long)p * ld * ld;
    const float alpha = bin_score[0];
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) Zp[(long)t * ld + n] = alpha;
    if (t < n) Zp[(long)m * ld + t] = alpha;
    if (t == 0) Zp[(long)m * ld + n] = alpha;
    if (t <= m) u[(long)p * ld + t] = 0.0f;
    if (t <= n) v[(long)p * ld + t] = 0.0f;
}

// exp(x) = 2^(x log2 e) on v_exp_f32 (1 ulp; arguments <= 0 here)
__device__ __forceinline__ float sk_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

// online log-sum-exp over four values at a time: one running-max update and no divergent branch per element, and the
// four loads behind it are issued together (the passes stream Z from HBM: 8.3 GB each on the C5 slice)
__device__ __forceinline__ void lse_push4(const float (&x)[4], float& mx, float& s) {
    const float nm = fmaxf(fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3])), mx);
    if (nm == -INFINITY) return;  // nothing seen yet (padding lanes)
    s = s * sk_exp(mx - nm) + ((sk_exp(x[0] - nm) + sk_exp(x[1] - nm)) + (sk_exp(x[2] - nm) + sk_exp(x[3] - nm)));
    mx = nm;
}

__device__ __forceinline__ void lse_merge(float& mx, float& s, float mo, float so) {
    if (mo > mx) {
        s = s * sk_exp(mx - mo) + so;
        mx = mo;
    } else if (so > 0.0f) {
        s = s + so * sk_exp(mo - mx);
    }
}

__device__ __forceinline__ float sk_norm(int m, int n) { return -logf((float)m + (float)n); }

// u[i] for rows 0..m: one wave per row
__global__ __launch_bounds__(256) void sk_rows_kernel(const float* __restrict__ Z, const int* __restrict__ side_counts,
                                                      int kmax, float* __restrict__ u, const float* __restrict__ v) {
    const int p = blockIdx.y;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i > m) return;
    const long ld = kmax + 1;
    const float* row = Z + (long)p * ld * ld + (long)i * ld;
    const float* vp = v + (long)p * ld;
    float mx = -INFINITY, s = 0.0f;
    for (int j0 = lane; j0 <= n; j0 += 256) {
        float x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + 64 * k;
            x[k] = j <= n ? row[j] + vp[j] : -INFINITY;
        }
        lse_push4(x, mx, s);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const float mo = __shfl_xor(mx, o), so = __shfl_xor(s, o);
        lse_merge(mx, s, mo, so);
    }
    if (lane == 0) {
        const float norm = sk_norm(m, n);
        const float log_mu = i < m ? norm : logf((float)n) + norm;
        u[(long)p * ld + i] = log_mu - (logf(s) + mx);
    }
}

// v[j] for columns 0..n: 64 columns x 4 row groups per workgroup
__global__ __launch_bounds__(256) void sk_cols_kernel(const float* __restrict__ Z, const int* __restrict__ side_counts,
                                                      int kmax, const float* __restrict__ u, float* __restrict__ v) {
    __shared__ float pm[4][64], ps[4][64];
    const int p = blockIdx.y;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    if (blockIdx.x * 64 > n) return;
    const long ld = kmax + 1;
    const float* Zp = Z + (long)p * ld * ld;
    const float* up = u + (long)p * ld;
    float mx = -INFINITY, s = 0.0f;
    if (j <= n)
        for (int i0 = g; i0 <= m; i0 += 16) {
            float x[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = i0 + 4 * k;
                x[k] = i <= m ? Zp[(long)i * ld + j] + up[i] : -INFINITY;
            }
            lse_push4(x, mx, s);
        }
    pm[g][c] = mx;
    ps[g][c] = s;
    __syncthreads();
    if (g == 0 && j <= n) {
        for (int o = 1; o < 4; ++o) lse_merge(mx, s, pm[o][c], ps[o][c]);
        const float norm = sk_norm(m, n);
        const float log_nu = j < n ? norm : logf((float)m) + norm;
        v[(long)p * ld + j] = log_nu - (logf(s) + mx);
    }
}

// One pass over Z per Sinkhorn iteration (kmax <= kSkFusedMaxK): a 64-lane workgroup takes kSkRows rows of one pair,
// lane l holding columns l + 64 k. Per row: u_i = log_mu - logsumexp_j(Z_ij + v_j) (sk_rows_kernel's grouping and
// order, so u is unchanged given v), then, from the same registers, each column's running log-sum-exp of Z_ij + u_i
// over the workgroup's rows; the partials (max, scaled sum) go to `part` and sk_vmerge_kernel turns them into v.
// Z is read once per iteration instead of twice; the column sums run in another order than sk_cols_kernel's, so v
// differs from the two-pass form in the last bits (the log-assignment tolerance of tests/test_superglue_gpu.py).
constexpr int kSkRows = 64, kSkNC = 33, kSkFusedMaxK = 64 * kSkNC - 1;
__host__ __device__ constexpr int sk_row_blocks(int kmax) { return (kmax + 1 + kSkRows - 1) / kSkRows; }

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2))) void sk_pass_kernel(const float* __restrict__ Z, const int* __restrict__ side_counts,
                                                     int kmax, float* __restrict__ u, const float* __restrict__ v,
                                                     float2* __restrict__ part) {
    const int p = blockIdx.y, rb = blockIdx.x, lane = threadIdx.x;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const int i0 = rb * kSkRows;
    const long ld = kmax + 1;
    float2* pp = part + ((long)p * sk_row_blocks(kmax) + rb) * ld;
    if (i0 > m) {  // a block wholly past the rows: an empty partial for every column
        for (int j = lane; j <= n; j += 64) pp[j] = make_float2(-INFINITY, 0.0f);
        return;
    }
    const float* Zp = Z + (long)p * ld * ld;
    __shared__ float vj[kSkNC * 64];  // v of the lane's columns (LDS: registers hold the row, its prefetch and partials)
    float cm[kSkNC], cs[kSkNC];
#pragma unroll
    for (int k = 0; k < kSkNC; ++k) {
        const int j = lane + 64 * k;
        vj[64 * k + lane] = j <= n ? v[(long)p * ld + j] : 0.0f;
        cm[k] = -INFINITY;
        cs[k] = 0.0f;
    }
    const float norm = sk_norm(m, n);
    const int i1 = min(m, i0 + kSkRows - 1);
    // row i + 1's loads are issued before row i is reduced (a wave's rows are a dependent sequence otherwise)
    float xn[kSkNC];
    auto load_row = [&](int i) {
        const float* row = Zp + (long)min(i, i1) * ld;
#pragma unroll
        for (int k = 0; k < kSkNC; ++k) {
            const int j = lane + 64 * k;
            xn[k] = j <= n ? row[j] : -INFINITY;
        }
    };
    load_row(i0);
    for (int i = i0; i <= i1; ++i) {
        float x[kSkNC];
#pragma unroll
        for (int k = 0; k < kSkNC; ++k) x[k] = xn[k];
        load_row(i + 1);
        float mx = -INFINITY, s = 0.0f;
#pragma unroll
        for (int k0 = 0; k0 < kSkNC; k0 += 4) {
            float y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) y[q] = k0 + q < kSkNC ? x[k0 + q] + vj[64 * (k0 + q) + lane] : -INFINITY;
            lse_push4(y, mx, s);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float mo = __shfl_xor(mx, o), so = __shfl_xor(s, o);
            lse_merge(mx, s, mo, so);
        }
        const float log_mu = i < m ? norm : logf((float)n) + norm;
        const float ui = log_mu - (logf(s) + mx);
        if (lane == 0) u[(long)p * ld + i] = ui;
#pragma unroll
        for (int k = 0; k < kSkNC; ++k) {
            const float y = x[k] + ui;
            const float nm = fmaxf(cm[k], y);
            if (nm != -INFINITY) {
                cs[k] = cs[k] * sk_exp(cm[k] - nm) + sk_exp(y - nm);
                cm[k] = nm;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kSkNC; ++k) {
        const int j = lane + 64 * k;
        if (j <= n) pp[j] = make_float2(cm[k], cs[k]);
    }
}

// v_j = log_nu - logsumexp over the row blocks' partials of column j (sk_pass_kernel)
__global__ __launch_bounds__(256) void sk_vmerge_kernel(const float2* __restrict__ part,
                                                        const int* __restrict__ side_counts, int kmax,
                                                        float* __restrict__ v) {
    const int p = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    if (j > n) return;
    const long ld = kmax + 1;
    const int nrb = sk_row_blocks(kmax), used = m / kSkRows + 1;
    const float2* pp = part + (long)p * nrb * ld + j;
    float mx = -INFINITY, s = 0.0f;
    for (int r = 0; r < used; ++r) {
        const float2 q = pp[(long)r * ld];
        lse_merge(mx, s, q.x, q.y);
    }
    const float norm = sk_norm(m, n);
    const float log_nu = j < n ? norm : logf((float)m) + norm;
    v[(long)p * ld + j] = log_nu - (logf(s) + mx);
}

// the final scores ((Z + u) + v) - norm (assign_rowmax_kernel / assign_colmax_kernel, sg_kernels.hpp)
struct SkScore {
    float norm;
    __device__ __forceinline__ SkScore(int m, int n) : norm(sk_norm(m, n)) {}
    __device__ __forceinline__ float operator()(float z, float ui, float vj) const { return ((z + ui) + vj) - norm; }
};

// final log-assignment of one pair ((Z + u) + v) - norm, rows 0..m, columns 0..n (ld = kmax + 1), NaN elsewhere
__global__ __launch_bounds__(256) void sk_final_kernel(const float* __restrict__ Z, const int* __restrict__ side_counts,
                                                       int kmax, const float* __restrict__ u,
                                                       const float* __restrict__ v, int p, float* __restrict__ out) {
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const long ld = kmax + 1;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= ld * ld) return;
    const int i = (int)(e / ld), j = (int)(e % ld);
    out[e] = (i <= m && j <= n) ? ((Z[(long)p * ld * ld + e] + u[(long)p * ld + i]) + v[(long)p * ld + j]) -
                                      sk_norm(m, n)
                                : __builtin_nanf("");
}

// ------------------------------------------------------------------ host-side orchestration
struct SgLayout {
    size_t enc_in, X, T1, T2, qkv, kvp, att, msg, hid, Z, u, v, part, max0, idx0, idx1, cnt, wsplit, total;
};

// bf16 planes of one GNN layer's four weight matrices (Wqkv, Wm, W1, W2), reused by the final projection
constexpr size_t kSplitElems = (size_t)256 * 768 + 256 * 256 + 512 * 512 + 512 * 256;

__host__ SgLayout sg_layout(int P, int kmax) {
    SgLayout L{};
    const size_t S = (size_t)2 * P * kmax;
    const size_t ld = (size_t)kmax + 1;
    WsCarver c;
    L.enc_in = c.take(S * 16 * 4);
    L.X = c.take(S * kD * 4);
    L.T1 = c.take(S * kD * 4);
    L.T2 = c.take(S * kD * 4);
    L.qkv = c.take(S * kD * 4);  // q only: keys and values go straight to the bf16 planes (kvp)
    L.kvp = c.take(S * 2 * kD * 3 * sizeof(__bf16));  // key and value planes of the current layer
    L.att = c.take(S * kD * 4);
    L.msg = c.take(S * kD * 4);
    L.hid = c.take(S * 512 * 4);
    L.Z = c.take((size_t)P * ld * ld * 4);
    L.u = c.take((size_t)P * ld * 4);
    L.v = c.take((size_t)P * ld * 4);
    L.part = c.take((size_t)P * sk_row_blocks(kmax) * ld * sizeof(float2));  // Sinkhorn column partials
    L.max0 = c.take((size_t)P * kmax * 4);
    L.idx0 = c.take((size_t)P * kmax * 4);
    L.idx1 = c.take((size_t)P * kmax * 4);
    L.cnt = c.take((size_t)2 * P * 4);
    L.wsplit = c.take(kSplitElems * 3 * sizeof(__bf16));
    L.total = c.o;
    return L;
}

}  // namespace

extern "C" {

size_t gtsfm_superglue_weights_floats(int n_layers) { return n_layers > 0 ? sg_weights_floats(n_layers) : 0; }

size_t gtsfm_superglue_workspace_bytes(int n_pairs, int kmax) {
    if (n_pairs <= 0 || kmax <= 0) return 0;
    return sg_layout(n_pairs, (kmax + 63) / 64 * 64).total;
}

int gtsfm_superglue_batched(const float* d_kp, const float* d_scores, const float* d_desc, const int* d_counts,
                            const int* d_image_hw, int n_img, int kmax, const int* d_pairs, int n_pairs,
                            const float* d_weights, int n_layers, int sinkhorn_iters, float match_threshold,
                            void* d_workspace, size_t workspace_bytes, uint32_t* d_out_idx, int* d_out_count,
                            float* d_out_mscores, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_pairs == 0) return GTSFM_OK;
    if (!d_kp || !d_scores || !d_desc || !d_counts || !d_image_hw || !d_pairs || !d_weights || !d_workspace ||
        !d_out_idx || !d_out_count || n_img <= 0 || kmax <= 0 || n_pairs < 0 || n_layers <= 0 || sinkhorn_iters < 0 ||
        kmax % 64 != 0)
        return GTSFM_ERR_ARG;
    const SgLayout L = sg_layout(n_pairs, kmax);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    float* enc_in = (float*)(ws + L.enc_in);
    float* X = (float*)(ws + L.X);
    float* T1 = (float*)(ws + L.T1);
    float* T2 = (float*)(ws + L.T2);
    float* qkv = (float*)(ws + L.qkv);
    __bf16* kvp = (__bf16*)(ws + L.kvp);
    const long kv_batch = (long)2 * 3 * kD * kmax;
    float* att = (float*)(ws + L.att);
    float* msg = (float*)(ws + L.msg);
    float* hid = (float*)(ws + L.hid);
    float* Z = (float*)(ws + L.Z);
    float* u = (float*)(ws + L.u);
    float* v = (float*)(ws + L.v);
    float* max0 = (float*)(ws + L.max0);
    int* idx0 = (int*)(ws + L.idx0);
    int* idx1 = (int*)(ws + L.idx1);
    int* side_counts = (int*)(ws + L.cnt);
    __bf16* wsp = (__bf16*)(ws + L.wsplit);
    __bf16* Pqkv = wsp;                        // [3][768][256]
    __bf16* Pm = Pqkv + 3 * (size_t)768 * 256;  // [3][256][256]
    __bf16* P1 = Pm + 3 * (size_t)256 * 256;    // [3][512][512]
    __bf16* P2 = P1 + 3 * (size_t)512 * 512;    // [3][256][512]
    const int S = 2 * n_pairs;
    hipLaunchKernelGGL(sg_prepare_kernel, dim3((kmax + 255) / 256, S), dim3(256), 0, stream, d_kp, d_scores, d_desc,
                       d_counts, d_image_hw, d_pairs, kmax, enc_in, X, side_counts);
    GTSFM_CHECK_HIP(hipGetLastError());
    // keypoint encoder (superglue.py:74-81): MLP [3, 32, 64, 128, 256, 256], BN + ReLU between layers; desc += enc
    const float* w = d_weights;
    {
        const float* in = enc_in;
        int cin = 16;
        float* bufs[2] = {T1, T2};
        for (int i = 0; i < 5; ++i) {
            const float* W = w;
            const float* bias = W + (size_t)kEncIn[i] * kEncOut[i];
            const int co = kEncOut[i];
            GemmArgs g = side_gemm(in, cin, W, kEncIn[i], co, bias, i < 4 ? bufs[i & 1] : X, i < 4 ? co : kD, kmax);
            if (i < 4) {
                g.bn_scale = bias + co;
                g.bn_shift = bias + 2 * co;
                g.relu = 1;
            } else {
                g.residual = 1;  // desc0 + kenc(...)
            }
            GTSFM_CHECK_HIP(run_gemm(g, S, stream));
            in = bufs[i & 1];
            cin = co;
            w += enc_floats(i);
        }
    }
    // attentional GNN (superglue.py:104-121): layer l is 'self' for even l, 'cross' for odd l
    for (int l = 0; l < n_layers; ++l) {
        const float* Wqkv = w;
        const float* bqkv = Wqkv + 256 * 768;
        const float* Wm = bqkv + 768;
        const float* bm = Wm + 256 * 256;
        const float* W1 = bm + 256;
        const float* b1 = W1 + 512 * 512;
        const float* s1 = b1 + 512;
        const float* h1 = s1 + 512;
        const float* W2 = h1 + 512;
        const float* b2 = W2 + 512 * 256;
        w += kLayerFloats;
        GTSFM_CHECK_HIP(split_weights(SplitJobs{{{Wqkv, Pqkv, kD, 768}, {Wm, Pm, kD, kD}, {W1, P1, 512, 512},
                                                 {W2, P2, 512, kD}}},
                                      stream));
        Gemm3Args gq = side_gemm3(X, kD, Pqkv, kD, 768, bqkv, qkv, kD, kmax);  // C = q (columns < 256), ldc 256
        gq.kv = kvp;
        gq.kv_batch = kv_batch;
        GTSFM_CHECK_HIP(run_gemm3(gq, S, stream));
        hipLaunchKernelGGL(sg_attention3_kernel, dim3((kmax + kAttnQ - 1) / kAttnQ, kHeads, S), dim3(kAttnThreads), 0,
                           stream, qkv, kvp, kv_batch, side_counts, kmax, l & 1, att);
        GTSFM_CHECK_HIP(hipGetLastError());
        GTSFM_CHECK_HIP(run_gemm3(side_gemm3(att, kD, Pm, kD, kD, bm, msg, kD, kmax), S, stream));
        Gemm3Args g1 = side_gemm3(X, kD, P1, 512, 512, b1, hid, 512, kmax);
        g1.Ksplit = kD;  // cat([x, message])
        g1.A2 = msg;
        g1.lda2 = kD;
        g1.a2_batch = (long)kmax * kD;
        g1.bn_scale = s1;
        g1.bn_shift = h1;
        g1.relu = 1;
        GTSFM_CHECK_HIP(run_gemm3(g1, S, stream));
        Gemm3Args g2 = side_gemm3(hid, 512, P2, 512, kD, b2, X, kD, kmax);
        g2.residual = 1;  // desc + delta
        GTSFM_CHECK_HIP(run_gemm3(g2, S, stream));
    }
    // final projection, scores = mdesc0^T mdesc1 / 16 into the coupling matrix interior
    const float* Wf = w;
    const float* bf = Wf + 256 * 256;
    const float* bin = bf + 256;
    GTSFM_CHECK_HIP(split_weights(SplitJobs{{{Wf, Pm, kD, kD}, {}, {}, {}}}, stream));
    GTSFM_CHECK_HIP(run_gemm3(side_gemm3(X, kD, Pm, kD, kD, bf, T1, kD, kmax), S, stream));
    const long ld = kmax + 1;
    {
        Gemm3Args g{};
        g.A = T1; g.lda = kD; g.a_batch = (long)2 * kmax * kD;
        g.Ksplit = kD;
        g.Bt = T1 + (long)kmax * kD; g.ldb = kD; g.b_batch = (long)2 * kmax * kD;
        g.alpha = 1.0f / 16.0f;
        g.C = Z; g.ldc = ld; g.c_batch = ld * ld;
        g.M = kmax; g.N = kmax; g.K = kD;
        g.m_lim = side_counts; g.n_lim = side_counts; g.lim_stride = 2;
        GTSFM_CHECK_HIP(run_gemm3(g, n_pairs, stream));
    }
    hipLaunchKernelGGL(sk_init_kernel, dim3((kmax + 256) / 256, n_pairs), dim3(256), 0, stream, Z, side_counts, kmax,
                       bin, u, v);
    // Sinkhorn: one pass over Z per iteration (sk_pass_kernel + sk_vmerge_kernel) for kmax <= 2048 (33 columns per
    // lane), else two passes (sk_rows_kernel, sk_cols_kernel). C5 slice match stage 860 -> 826 ms per step, 532
    // -> 555 pairs/s (profiles/r06m_*). Round 5's one-pass form (a workgroup's 8 rows of Z in LDS, 65 KB, phases in
    // series) ran 7.35 ms per iteration against 2.09 + 2.01 ms for the two passes; this one keeps the rows and the
    // column partials in registers (one 64-lane wave per 64 rows, the next row prefetched) and needs no LDS for Z.
    const char* sk_env = getenv("GTSFM_SG_SINKHORN_TWO_PASS");  // test hook: the two-pass form below
    if (kmax <= kSkFusedMaxK && !(sk_env && sk_env[0] == '1')) {
        float2* part = (float2*)(ws + L.part);
        for (int it = 0; it < sinkhorn_iters; ++it) {
            hipLaunchKernelGGL(sk_pass_kernel, dim3(sk_row_blocks(kmax), n_pairs), dim3(64), 0, stream, Z,
                               side_counts, kmax, u, (const float*)v, part);
            hipLaunchKernelGGL(sk_vmerge_kernel, dim3((kmax + 256) / 256, n_pairs), dim3(256), 0, stream,
                               (const float2*)part, side_counts, kmax, v);
        }
    } else {
        for (int it = 0; it < sinkhorn_iters; ++it) {
            hipLaunchKernelGGL(sk_rows_kernel, dim3((kmax + 4) / 4, n_pairs), dim3(256), 0, stream, Z, side_counts,
                               kmax, u, (const float*)v);
            hipLaunchKernelGGL(sk_cols_kernel, dim3((kmax + 64) / 64, n_pairs), dim3(256), 0, stream, Z, side_counts,
                               kmax, (const float*)u, v);
        }
    }
    GTSFM_CHECK_HIP(run_assign_argmax<SkScore>(Z, side_counts, kmax, n_pairs, u, v, max0, idx0, idx1, stream));
    hipLaunchKernelGGL(sg_emit_kernel, dim3(n_pairs), dim3(256), 0, stream, side_counts, kmax, max0, idx0, idx1,
                       match_threshold, d_out_idx, d_out_count, d_out_mscores);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

int gtsfm_superglue_log_assignment(const void* d_workspace, size_t workspace_bytes, int n_pairs, int kmax, int pair,
                                   float* d_out, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!d_workspace || !d_out || n_pairs <= 0 || pair < 0 || pair >= n_pairs || kmax <= 0 || kmax % 64 != 0)
        return GTSFM_ERR_ARG;
    const SgLayout L = sg_layout(n_pairs, kmax);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    const unsigned char* ws = (const unsigned char*)d_workspace;
    const long ld = kmax + 1;
    hipLaunchKernelGGL(sk_final_kernel, dim3((unsigned)((ld * ld + 255) / 256)), dim3(256), 0, stream,
                       (const float*)(ws + L.Z), (const int*)(ws + L.cnt), kmax, (const float*)(ws + L.u),
                       (const float*)(ws + L.v), pair, d_out);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // extern "C"
