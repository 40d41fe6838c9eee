// LightGlue matcher on gfx950 at SuperPoint's width (d = 256, 4 heads of 64, 9 layers of one self and one cross
// block), as gtsfm/frontend/matcher/lightglue_matcher.py:24-93 drives it, batched over image pairs. The arithmetic is
// the one DESIGN.md restates (the LightGlue source is not part of the reference checkout): rotary position encoding,
// shared-projection bidirectional cross attention, LayerNorm + GELU feed-forward, double-softmax assignment with
// matchability, and adaptive depth (every pair leaves the network at its own layer). Point pruning is not built.
//
// Shared with superglue.hip (sg_kernels.hpp): the fp32-accurate split-bf16 GEMM, its weight splitter, the fused
// attention kernel and the match emission. New here: the position encoding, the q/k/v packing with the rotary step,
// the LayerNorm + GELU row kernel, the confidence / stop kernel and the assignment's log-sum-exp kernels (its argmax
// read-out is sg_kernels.hpp's, with LgScore).
//
// Layout: every (pair, side) owns a kmax x C row-major block, as in superglue.hip. Adaptive depth without a host
// read-back: `live[side]` holds the side's keypoint count while its pair is in the network and 0 afterwards. Every
// GEMM takes it as its row limit and the attention kernel as its query / key count, so the workgroups of a stopped
// pair return at once and its features stay what they were at its exit layer.
#include "sg_kernels.hpp"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------ packed weights (include/gtsfm_hip.h)
// Wr (32 x 2), then per layer: the self block, the cross block, the assignment and the token-confidence head.
// GEMM weights are W^T[cin][cout] row-major.
// self:  Wqkv^T (256 x 768, columns [q | k | v], each head-major h * 64 + e), bqkv, Wout^T (256 x 256), bout,
//        W1^T (512 x 512: rows 0..255 act on x, 256..511 on the message), b1, LayerNorm weight, LayerNorm bias,
//        W2^T (512 x 256), b2
// cross: Wqkv^T (256 x 512, columns [qk | v]), bias, then as the self block
// tail:  final_proj W^T (256 x 256), bias, matchability w (256), token w (256), matchability b, token b, 0, 0
constexpr size_t kFfnFloats = (size_t)256 * 256 + 256 + 512 * 512 + 3 * 512 + 512 * 256 + 256;
constexpr size_t kSelfFloats = (size_t)256 * 768 + 768 + kFfnFloats;
constexpr size_t kCrossFloats = (size_t)256 * 512 + 512 + kFfnFloats;
constexpr size_t kTailFloats = (size_t)256 * 256 + 256 + 256 + 256 + 4;
constexpr size_t kLgLayerFloats = kSelfFloats + kCrossFloats + kTailFloats;
constexpr size_t kLgHead = 64;
__host__ __device__ constexpr size_t lg_weights_floats(int n_layers) { return kLgHead + n_layers * kLgLayerFloats; }
__host__ __device__ constexpr size_t lg_tail(int layer) {
    return kLgHead + layer * kLgLayerFloats + kSelfFloats + kCrossFloats;
}
constexpr int kMaxLayers = 16;

// log(sigmoid(z)) = min(z, 0) - log1p(exp(-|z|))
__device__ __forceinline__ float log_sigmoid(float z) { return fminf(z, 0.0f) - log1pf(expf(-fabsf(z))); }

// ------------------------------------------------------------------ inputs and position encoding
// One wave per keypoint row. X <- descriptors (rows past the count zeroed); p = (kpt - size / 2) / (max(W, H) / 2)
// with the side's own image size; theta_j = Wr[j] . p for j < 32; pe row = [cos theta | sin theta] (frequency j
// serves channels 2 j and 2 j + 1 of every head and layer). Accurate cosf / sinf. A pair with an empty side never
// enters the network (live = 0).
__global__ __launch_bounds__(256) void lg_prepare_kernel(const float* __restrict__ kp, const float* __restrict__ desc,
                                                         const int* __restrict__ counts, const int* __restrict__ hw,
                                                         const int* __restrict__ pairs, int kmax, int n_layers,
                                                         const float* __restrict__ Wr, float* __restrict__ X,
                                                         float* __restrict__ pe, int* __restrict__ side_counts,
                                                         int* __restrict__ live, int* __restrict__ exit_layer) {
    const int zs = blockIdx.y;
    const int img = pairs[zs], other = pairs[zs ^ 1];
    const int n = counts[img];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        side_counts[zs] = n;
        live[zs] = (n > 0 && counts[other] > 0) ? n : 0;
        if ((zs & 1) == 0) exit_layer[zs >> 1] = n_layers - 1;
    }
    if (i >= kmax) return;
    float* x = X + ((long)zs * kmax + i) * kD;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) v = *(const f32x4*)(desc + ((long)img * kmax + i) * kD + 4 * lane);
    *(f32x4*)(x + 4 * lane) = v;
    if (lane < 32) {
        float c = 1.0f, s = 0.0f;
        if (i < n) {
            const float W = (float)hw[2 * img + 1], H = (float)hw[2 * img];
            const float half = fmaxf(W, H) / 2.0f;
            const float px = (kp[((long)img * kmax + i) * 2] - W / 2.0f) / half;
            const float py = (kp[((long)img * kmax + i) * 2 + 1] - H / 2.0f) / half;
            const float th = Wr[2 * lane] * px + Wr[2 * lane + 1] * py;
            c = cosf(th);
            s = sinf(th);
        }
        pe[((long)zs * kmax + i) * 64 + lane] = c;
        pe[((long)zs * kmax + i) * 64 + 32 + lane] = s;
    }
}

// ------------------------------------------------------------------ q / k / v packing
// The projection GEMM leaves P[side][row][ld] fp32 (self: ld 768 = [q | k | v]; cross: ld 512 = [qk | v]). One
// workgroup takes 64 rows of one (side, head) and writes what sg_attention3_kernel reads: the query as fp32
// (side, kmax, 256), the key as bf16 planes [3][head][kmax][64], the value as transposed planes [3][head][64][kmax].
// Self blocks rotate q and k first: t'[2 j] = t[2 j] cos_j - t[2 j + 1] sin_j, t'[2 j + 1] = t[2 j + 1] cos_j +
// t[2 j] sin_j. Cross blocks write qk as the query and as the key. Rows past the side's count are written as zeros
// (the attention kernel loads values eight keys at a time, past the count too).
__global__ __launch_bounds__(256) void lg_pack_kernel(const float* __restrict__ P, int ld, int self,
                                                      const float* __restrict__ pe, const int* __restrict__ live,
                                                      int kmax, float* __restrict__ q, __bf16* __restrict__ kv,
                                                      long kv_batch) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    __shared__ float tile[64][65];
    const int zs = blockIdx.z, h = blockIdx.y, r0 = blockIdx.x * 64;
    const int n = live[zs];
    if (n == 0) return;
    const int tid = threadIdx.x, d = tid & 63;
    const float* Pz = P + (long)zs * kmax * ld;
    const int koff = self ? kD : 0, voff = self ? 2 * kD : kD;
    __bf16* kbase = kv + zs * kv_batch;
    __bf16* vbase = kbase + (long)3 * kD * kmax;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {
        const int row = r0 + (tid >> 6) + 4 * it;
        const float* pr = Pz + (long)row * ld + h * kHd;
        float qv = 0.0f, kvv = 0.0f, vv = 0.0f;
        if (row < n) {
            qv = pr[d];
            kvv = pr[koff + d];
            vv = pr[voff + d];
            if (self) {
                const float c = pe[((long)zs * kmax + row) * 64 + (d >> 1)];
                const float s = pe[((long)zs * kmax + row) * 64 + 32 + (d >> 1)];
                const float qp = pr[d ^ 1], kp2 = pr[koff + (d ^ 1)];
                qv = (d & 1) ? qv * c + qp * s : qv * c - qp * s;
                kvv = (d & 1) ? kvv * c + kp2 * s : kvv * c - kp2 * s;
            }
        }
        q[((long)zs * kmax + row) * kD + h * kHd + d] = qv;
        __bf16 pl[3];
        split3(kvv, pl[0], pl[1], pl[2]);
#pragma unroll
        for (int p = 0; p < 3; ++p) kbase[(((long)p * kHeads + h) * kmax + row) * kHd + d] = pl[p];
        tile[(tid >> 6) + 4 * it][d] = vv;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int item = tid + 256 * it;
        const int dd = item >> 4, kg = item & 15;
        bf16x4 pl[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            __bf16 a, b, c;
            split3(tile[4 * kg + e][dd], a, b, c);
            pl[0][e] = a;
            pl[1][e] = b;
            pl[2][e] = c;
        }
#pragma unroll
        for (int p = 0; p < 3; ++p)
            *(bf16x4*)(vbase + (((long)p * kHeads + h) * kHd + dd) * kmax + r0 + 4 * kg) = pl[p];
    }
}

// ------------------------------------------------------------------ LayerNorm(512) + exact GELU, in place
// One wave per row (eight values per lane), two-pass variance in fp32 (biased, eps 1e-5), erff.
__global__ __launch_bounds__(256) void lg_ln_gelu_kernel(float* __restrict__ hid, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta,
                                                         const int* __restrict__ live, int kmax) {
    const int zs = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= live[zs]) return;
    float* row = hid + ((long)zs * kmax + i) * 512;
    f32x4 a = *(const f32x4*)(row + 4 * lane), b = *(const f32x4*)(row + 256 + 4 * lane);
    const float mean = wave_sum(((a[0] + a[1]) + (a[2] + a[3])) + ((b[0] + b[1]) + (b[2] + b[3]))) / 512.0f;
    a = a - mean;
    b = b - mean;
    const float var = wave_sum(((a[0] * a[0] + a[1] * a[1]) + (a[2] * a[2] + a[3] * a[3])) +
                               ((b[0] * b[0] + b[1] * b[1]) + (b[2] * b[2] + b[3] * b[3]))) / 512.0f;
    const float inv = 1.0f / sqrtf(var + 1e-5f);
    const f32x4 ga = *(const f32x4*)(gamma + 4 * lane), gb = *(const f32x4*)(gamma + 256 + 4 * lane);
    const f32x4 ba = *(const f32x4*)(beta + 4 * lane), bb = *(const f32x4*)(beta + 256 + 4 * lane);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float ya = a[e] * inv * ga[e] + ba[e], yb = b[e] * inv * gb[e] + bb[e];
        a[e] = 0.5f * ya * (1.0f + erff(ya * 0.70710678118654752f));
        b[e] = 0.5f * yb * (1.0f + erff(yb * 0.70710678118654752f));
    }
    *(f32x4*)(row + 4 * lane) = a;
    *(f32x4*)(row + 256 + 4 * lane) = b;
}

// w . x + b of one 256-D row, over the wave
__device__ __forceinline__ float row_dot(const float* __restrict__ x, const float* __restrict__ w, int lane) {
    const f32x4 a = *(const f32x4*)(x + 4 * lane), b = *(const f32x4*)(w + 4 * lane);
    return wave_sum((a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]));
}

// ------------------------------------------------------------------ token confidence and the stop decision
// After layer `layer` (not the last): c = sigmoid(w . x + b) for every keypoint of both sides; the pair stops if
// 1 - #{c < tau} / (n0 + n1) > depth_confidence. One workgroup per pair; a stopped pair's live counts become 0.
__global__ __launch_bounds__(256) void lg_confidence_kernel(const float* __restrict__ X, const float* __restrict__ wt,
                                                            const float* __restrict__ bt, float tau, float conf,
                                                            int layer, int kmax, int* __restrict__ live,
                                                            int* __restrict__ exit_layer) {
    __shared__ int below[4];
    const int p = blockIdx.x;
    const int n0 = live[2 * p], n1 = live[2 * p + 1];
    if (n0 == 0 || n1 == 0) return;  // (uniform over the workgroup) stopped earlier, or never ran
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float b = bt[0];
    int cnt = 0;
    for (int r = wave; r < n0 + n1; r += 4) {
        const int side = r < n0 ? 0 : 1, i = r < n0 ? r : r - n0;
        const float t = row_dot(X + ((long)(2 * p + side) * kmax + i) * kD, wt, lane) + b;
        const float c = 1.0f / (1.0f + expf(-t));
        cnt += c < tau ? 1 : 0;
    }
    if (lane == 0) below[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = below[0] + below[1] + below[2] + below[3];
        const float ratio = 1.0f - (float)total / (float)(n0 + n1);
        if (ratio > conf) {
            exit_layer[p] = layer;
            live[2 * p] = 0;
            live[2 * p + 1] = 0;
        }
    }
}

// ------------------------------------------------------------------ assignment
// lims[layer][side] = the side's count if its pair left the network at `layer` (and ran at all), else 0: the row
// limit of that layer's final projection.
__global__ void lg_lims_kernel(const int* __restrict__ side_counts, const int* __restrict__ exit_layer, int S,
                               int n_layers, int* __restrict__ lims) {
    const int zs = blockIdx.x * blockDim.x + threadIdx.x;
    if (zs >= S) return;
    const bool ran = side_counts[zs] > 0 && side_counts[zs ^ 1] > 0;
    const int e = exit_layer[zs >> 1];
    for (int l = 0; l < n_layers; ++l) lims[l * S + zs] = (ran && e == l) ? side_counts[zs] : 0;
}

// matchability z = wm . x + bm with the pair's exit layer's weights: lsp = logsigmoid(z), lsn = logsigmoid(-z)
__global__ __launch_bounds__(256) void lg_matchability_kernel(const float* __restrict__ X,
                                                              const float* __restrict__ weights,
                                                              const int* __restrict__ side_counts,
                                                              const int* __restrict__ exit_layer, int kmax,
                                                              float* __restrict__ lsp, float* __restrict__ lsn) {
    const int zs = blockIdx.y, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= side_counts[zs] || side_counts[zs ^ 1] == 0) return;
    const float* tail = weights + lg_tail(exit_layer[zs >> 1]) + 256 * 256 + 256;
    const float z = row_dot(X + ((long)zs * kmax + i) * kD, tail, lane) + tail[512];
    if (lane == 0) {
        lsp[(long)zs * kmax + i] = log_sigmoid(z);
        lsn[(long)zs * kmax + i] = log_sigmoid(-z);
    }
}

// u[i] = logsigmoid(z0[i]) - logsumexp_j S[i][j]: one wave per row, lane l takes columns l + 64 k, four per step
constexpr int kLseChunk = 256;
__global__ __launch_bounds__(256) void lg_rowlse_kernel(const float* __restrict__ Z,
                                                        const int* __restrict__ side_counts, int kmax,
                                                        const float* __restrict__ lsp, float* __restrict__ u) {
    const int p = blockIdx.y;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= m || n == 0) return;
    const long ld = kmax + 1;
    const float* row = Z + (long)p * ld * ld + (long)i * ld;
    float mx = -INFINITY;
    for (int j0 = lane; j0 < n; j0 += kLseChunk) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + 64 * k < n) mx = fmaxf(mx, row[j0 + 64 * k]);
    }
    mx = wave_max(mx);
    float s = 0.0f;
    for (int j0 = lane; j0 < n; j0 += kLseChunk) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (j0 + 64 * k < n) s = s + expf(row[j0 + 64 * k] - mx);
    }
    s = wave_sum(s);
    if (lane == 0) u[(long)p * ld + i] = lsp[(long)(2 * p) * kmax + i] - (mx + logf(s));
}

// v[j] = logsigmoid(z1[j]) - logsumexp_i S[i][j]: 64 columns x 4 row groups per workgroup, four rows per step
constexpr int kColRows = 16;
__global__ __launch_bounds__(256) void lg_collse_kernel(const float* __restrict__ Z,
                                                        const int* __restrict__ side_counts, int kmax,
                                                        const float* __restrict__ lsp, float* __restrict__ v) {
    __shared__ float red[4][64];
    const int p = blockIdx.y;
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    if (blockIdx.x * 64 >= n || m == 0) return;
    const long ld = kmax + 1;
    const float* Zp = Z + (long)p * ld * ld;
    float mx = -INFINITY;
    if (j < n)
        for (int i0 = g; i0 < m; i0 += kColRows) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + 4 * k < m) mx = fmaxf(mx, Zp[(long)(i0 + 4 * k) * ld + j]);
        }
    red[g][c] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0][c], red[1][c]), fmaxf(red[2][c], red[3][c]));
    __syncthreads();
    float s = 0.0f;
    if (j < n)
        for (int i0 = g; i0 < m; i0 += kColRows) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (i0 + 4 * k < m) s = s + expf(Zp[(long)(i0 + 4 * k) * ld + j] - mx);
        }
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && j < n) {
        s = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
        v[(long)p * ld + j] = lsp[(long)(2 * p + 1) * kmax + j] - (mx + logf(s));
    }
}

// the log-assignment of (i, j): log_softmax_j S + log_softmax_i S + logsigmoid(z0[i]) + logsigmoid(z1[j])
// (assign_rowmax_kernel / assign_colmax_kernel, sg_kernels.hpp)
struct LgScore {
    __device__ __forceinline__ LgScore(int, int) {}
    __device__ __forceinline__ float operator()(float s, float ui, float vj) const { return (s + ui) + (s + vj); }
};

// one pair's (m + 1) x (n + 1) log-assignment with its dustbin column / row, NaN elsewhere (ld = kmax + 1)
__global__ __launch_bounds__(256) void lg_final_kernel(const float* __restrict__ Z, const int* __restrict__ side_counts,
                                                       int kmax, const float* __restrict__ u,
                                                       const float* __restrict__ v, const float* __restrict__ lsn,
                                                       int p, float* __restrict__ out) {
    const int m = side_counts[2 * p], n = side_counts[2 * p + 1];
    const long ld = kmax + 1;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= ld * ld) return;
    const int i = (int)(e / ld), j = (int)(e % ld);
    float r = __builtin_nanf("");
    if (m > 0 && n > 0 && i <= m && j <= n) {
        if (i < m && j < n) r = LgScore(m, n)(Z[(long)p * ld * ld + e], u[(long)p * ld + i], v[(long)p * ld + j]);
        else if (i < m) r = lsn[(long)(2 * p) * kmax + i];
        else if (j < n) r = lsn[(long)(2 * p + 1) * kmax + j];
        else r = 0.0f;
    }
    out[e] = r;
}

// ------------------------------------------------------------------ host-side orchestration
struct LgLayout {
    size_t X, pe, proj, q, kvp, att, msg, hid, Z, u, v, lsp, lsn, max0, idx0, idx1, cnt, live, exit_layer, lims, wsplit,
        total;
};

// bf16 planes of one block's four weight matrices (Wqkv, Wout, W1, W2), reused by the final projections
constexpr size_t kLgSplitElems = (size_t)256 * 768 + 256 * 256 + 512 * 512 + 512 * 256;

__host__ LgLayout lg_layout(int P, int kmax) {
    LgLayout L{};
    const size_t S = (size_t)2 * P * kmax;
    const size_t ld = (size_t)kmax + 1;
    WsCarver c;
    L.X = c.take(S * kD * 4);
    L.pe = c.take(S * 64 * 4);
    L.proj = c.take(S * 768 * 4);  // the q/k/v projection; later the final projection (ld 256)
    L.q = c.take(S * kD * 4);
    L.kvp = c.take(S * 2 * kD * 3 * sizeof(__bf16));
    L.att = c.take(S * kD * 4);
    L.msg = c.take(S * kD * 4);
    L.hid = c.take(S * 512 * 4);
    L.Z = c.take((size_t)P * ld * ld * 4);
    L.u = c.take((size_t)P * ld * 4);
    L.v = c.take((size_t)P * ld * 4);
    L.lsp = c.take(S * 4);
    L.lsn = c.take(S * 4);
    L.max0 = c.take((size_t)P * kmax * 4);
    L.idx0 = c.take((size_t)P * kmax * 4);
    L.idx1 = c.take((size_t)P * kmax * 4);
    L.cnt = c.take((size_t)2 * P * 4);
    L.live = c.take((size_t)2 * P * 4);
    L.exit_layer = c.take((size_t)P * 4);
    L.lims = c.take((size_t)kMaxLayers * 2 * P * 4);
    L.wsplit = c.take(kLgSplitElems * 3 * sizeof(__bf16));
    L.total = c.o;
    return L;
}

struct LgFfn {
    const float *Wo, *bo, *W1, *b1, *g, *b, *W2, *b2;
};
// the part of a block after its projection: Wout, bout, W1, b1, LayerNorm weight, LayerNorm bias, W2, b2
LgFfn lg_ffn(const float* w) {
    LgFfn f;
    f.Wo = w;
    f.bo = f.Wo + 256 * 256;
    f.W1 = f.bo + 256;
    f.b1 = f.W1 + 512 * 512;
    f.g = f.b1 + 512;
    f.b = f.g + 512;
    f.W2 = f.b + 512;
    f.b2 = f.W2 + 512 * 256;
    return f;
}

}  // namespace

extern "C" {

size_t gtsfm_lightglue_weights_floats(int n_layers) {
    return n_layers > 0 && n_layers <= kMaxLayers ? lg_weights_floats(n_layers) : 0;
}

size_t gtsfm_lightglue_workspace_bytes(int n_pairs, int kmax) {
    if (n_pairs <= 0 || kmax <= 0) return 0;
    return lg_layout(n_pairs, (kmax + 63) / 64 * 64).total;
}

int gtsfm_lightglue_batched(const float* d_kp, const float* d_desc, const int* d_counts, const int* d_image_hw,
                            int n_img, int kmax, const int* d_pairs, int n_pairs, const float* d_weights, int n_layers,
                            float depth_confidence, float filter_threshold, void* d_workspace, size_t workspace_bytes,
                            uint32_t* d_out_idx, int* d_out_count, float* d_out_mscores, int* d_out_exit_layer,
                            void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_pairs == 0) return GTSFM_OK;
    if (!d_kp || !d_desc || !d_counts || !d_image_hw || !d_pairs || !d_weights || !d_workspace || !d_out_idx ||
        !d_out_count || n_img <= 0 || kmax <= 0 || n_pairs < 0 || n_layers <= 0 || n_layers > kMaxLayers ||
        kmax % 64 != 0)
        return GTSFM_ERR_ARG;
    const LgLayout L = lg_layout(n_pairs, kmax);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    float* X = (float*)(ws + L.X);
    float* pe = (float*)(ws + L.pe);
    float* proj = (float*)(ws + L.proj);
    float* q = (float*)(ws + L.q);
    __bf16* kvp = (__bf16*)(ws + L.kvp);
    const long kv_batch = (long)2 * 3 * kD * kmax;
    float* att = (float*)(ws + L.att);
    float* msg = (float*)(ws + L.msg);
    float* hid = (float*)(ws + L.hid);
    float* Z = (float*)(ws + L.Z);
    float* u = (float*)(ws + L.u);
    float* v = (float*)(ws + L.v);
    float* lsp = (float*)(ws + L.lsp);
    float* lsn = (float*)(ws + L.lsn);
    float* max0 = (float*)(ws + L.max0);
    int* idx0 = (int*)(ws + L.idx0);
    int* idx1 = (int*)(ws + L.idx1);
    int* side_counts = (int*)(ws + L.cnt);
    int* live = (int*)(ws + L.live);
    int* exit_layer = (int*)(ws + L.exit_layer);
    int* lims = (int*)(ws + L.lims);
    __bf16* wsp = (__bf16*)(ws + L.wsplit);
    __bf16* Pqkv = wsp;                         // [3][768 or 512][256]
    __bf16* Po = Pqkv + 3 * (size_t)768 * 256;  // [3][256][256]
    __bf16* P1 = Po + 3 * (size_t)256 * 256;    // [3][512][512]
    __bf16* P2 = P1 + 3 * (size_t)512 * 512;    // [3][256][512]
    const int S = 2 * n_pairs;
    const bool stopping = depth_confidence > 0.0f;
    hipLaunchKernelGGL(lg_prepare_kernel, dim3(kmax / 4, S), dim3(256), 0, stream, d_kp, d_desc, d_counts, d_image_hw,
                       d_pairs, kmax, n_layers, d_weights, X, pe, side_counts, live, exit_layer);
    GTSFM_CHECK_HIP(hipGetLastError());
    for (int l = 0; l < n_layers; ++l) {
        const float* wl = d_weights + kLgHead + (size_t)l * kLgLayerFloats;
        for (int cross = 0; cross < 2; ++cross) {
            const int nproj = cross ? 512 : 768;
            const float* Wp = cross ? wl + kSelfFloats : wl;
            const float* bp = Wp + (size_t)256 * nproj;
            const LgFfn f = lg_ffn(bp + nproj);
            GTSFM_CHECK_HIP(split_weights(SplitJobs{{{Wp, Pqkv, kD, nproj}, {f.Wo, Po, kD, kD}, {f.W1, P1, 512, 512},
                                                     {f.W2, P2, 512, kD}}},
                                          stream));
            Gemm3Args gp = side_gemm3(X, kD, Pqkv, kD, nproj, bp, proj, nproj, kmax);
            gp.m_lim = live;
            gp.lim_stride = 1;
            GTSFM_CHECK_HIP(run_gemm3(gp, S, stream));
            hipLaunchKernelGGL(lg_pack_kernel, dim3(kmax / 64, kHeads, S), dim3(256), 0, stream, (const float*)proj,
                               nproj, cross ? 0 : 1, (const float*)pe, (const int*)live, kmax, q, kvp, kv_batch);
            hipLaunchKernelGGL(sg_attention3_kernel, dim3((kmax + kAttnQ - 1) / kAttnQ, kHeads, S), dim3(kAttnThreads),
                               0, stream, (const float*)q, (const __bf16*)kvp, kv_batch, (const int*)live, kmax, cross,
                               att);
            GTSFM_CHECK_HIP(hipGetLastError());
            Gemm3Args go = side_gemm3(att, kD, Po, kD, kD, f.bo, msg, kD, kmax);
            go.m_lim = live;
            go.lim_stride = 1;
            GTSFM_CHECK_HIP(run_gemm3(go, S, stream));
            Gemm3Args g1 = side_gemm3(X, kD, P1, 512, 512, f.b1, hid, 512, kmax);
            g1.Ksplit = kD;  // cat([x, message])
            g1.A2 = msg;
            g1.lda2 = kD;
            g1.a2_batch = (long)kmax * kD;
            g1.m_lim = live;
            g1.lim_stride = 1;
            GTSFM_CHECK_HIP(run_gemm3(g1, S, stream));
            hipLaunchKernelGGL(lg_ln_gelu_kernel, dim3(kmax / 4, S), dim3(256), 0, stream, hid, f.g, f.b,
                               (const int*)live, kmax);
            Gemm3Args g2 = side_gemm3(hid, 512, P2, 512, kD, f.b2, X, kD, kmax);
            g2.residual = 1;  // x + FFN([x | message])
            g2.m_lim = live;
            g2.lim_stride = 1;
            GTSFM_CHECK_HIP(run_gemm3(g2, S, stream));
        }
        if (stopping && l + 1 < n_layers) {
            const float* tail = d_weights + lg_tail(l);
            float tau = 0.8f + 0.1f * expf(-4.0f * (float)l / (float)n_layers);
            tau = tau < 0.0f ? 0.0f : (tau > 1.0f ? 1.0f : tau);
            hipLaunchKernelGGL(lg_confidence_kernel, dim3(n_pairs), dim3(256), 0, stream, (const float*)X,
                               tail + 256 * 256 + 512, tail + 256 * 256 + 768 + 1, tau, depth_confidence, l, kmax,
                               live, exit_layer);
            GTSFM_CHECK_HIP(hipGetLastError());
        }
    }
    // assignment with the weights of the layer each pair stopped at: one final projection per layer over the pairs
    // that left there (every other pair's workgroups return at once), md = (Wf x + b) / 256^(1/4)
    hipLaunchKernelGGL(lg_lims_kernel, dim3((S + 255) / 256), dim3(256), 0, stream, (const int*)side_counts,
                       (const int*)exit_layer, S, n_layers, lims);
    GTSFM_CHECK_HIP(hipGetLastError());
    float* md = proj;
    for (int l = stopping ? 0 : n_layers - 1; l < n_layers; ++l) {
        const float* tail = d_weights + lg_tail(l);
        GTSFM_CHECK_HIP(split_weights(SplitJobs{{{tail, Po, kD, kD}, {}, {}, {}}}, stream));
        Gemm3Args gf = side_gemm3(X, kD, Po, kD, kD, tail + 256 * 256, md, kD, kmax);
        gf.alpha = 0.25f;
        gf.m_lim = lims + (size_t)l * S;
        gf.lim_stride = 1;
        GTSFM_CHECK_HIP(run_gemm3(gf, S, stream));
    }
    hipLaunchKernelGGL(lg_matchability_kernel, dim3(kmax / 4, S), dim3(256), 0, stream, (const float*)X, d_weights,
                       (const int*)side_counts, (const int*)exit_layer, kmax, lsp, lsn);
    GTSFM_CHECK_HIP(hipGetLastError());
    const long ld = kmax + 1;
    {
        Gemm3Args g{};
        g.A = md; g.lda = kD; g.a_batch = (long)2 * kmax * kD;
        g.Ksplit = kD;
        g.Bt = md + (long)kmax * kD; g.ldb = kD; g.b_batch = (long)2 * kmax * kD;
        g.alpha = 1.0f;
        g.C = Z; g.ldc = ld; g.c_batch = ld * ld;
        g.M = kmax; g.N = kmax; g.K = kD;
        g.m_lim = side_counts; g.n_lim = side_counts; g.lim_stride = 2;
        GTSFM_CHECK_HIP(run_gemm3(g, n_pairs, stream));
    }
    hipLaunchKernelGGL(lg_rowlse_kernel, dim3(kmax / 4, n_pairs), dim3(256), 0, stream, (const float*)Z,
                       (const int*)side_counts, kmax, (const float*)lsp, u);
    hipLaunchKernelGGL(lg_collse_kernel, dim3(kmax / 64, n_pairs), dim3(256), 0, stream, (const float*)Z,
                       (const int*)side_counts, kmax, (const float*)lsp, v);
    GTSFM_CHECK_HIP(hipGetLastError());
    GTSFM_CHECK_HIP(run_assign_argmax<LgScore>(Z, side_counts, kmax, n_pairs, u, v, max0, idx0, idx1, stream));
    hipLaunchKernelGGL(sg_emit_kernel, dim3(n_pairs), dim3(256), 0, stream, (const int*)side_counts, kmax,
                       (const float*)max0, (const int*)idx0, (const int*)idx1, filter_threshold, d_out_idx,
                       d_out_count, d_out_mscores);
    GTSFM_CHECK_HIP(hipGetLastError());
    if (d_out_exit_layer)
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_out_exit_layer, exit_layer, (size_t)n_pairs * sizeof(int),
                                       hipMemcpyDeviceToDevice, stream));
    return GTSFM_OK;
}

int gtsfm_lightglue_log_assignment(const void* d_workspace, size_t workspace_bytes, int n_pairs, int kmax, int pair,
                                   float* d_out, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!d_workspace || !d_out || n_pairs <= 0 || pair < 0 || pair >= n_pairs || kmax <= 0 || kmax % 64 != 0)
        return GTSFM_ERR_ARG;
    const LgLayout L = lg_layout(n_pairs, kmax);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    const unsigned char* ws = (const unsigned char*)d_workspace;
    const long ld = kmax + 1;
    hipLaunchKernelGGL(lg_final_kernel, dim3((unsigned)((ld * ld + 255) / 256)), dim3(256), 0, stream,
                       (const float*)(ws + L.Z), (const int*)(ws + L.cnt), kmax, (const float*)(ws + L.u),
                       (const float*)(ws + L.v), (const float*)(ws + L.lsn), pair, d_out);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // extern "C"
