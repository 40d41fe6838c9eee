// PatchmatchNet depth estimation (eval mode, the reference's fixed configuration), batched over reference views:
// thirdparty/patchmatchnet/models/net.py (FeatureNet, Refinement, PatchmatchNet.forward), patchmatch.py (the three
// PatchMatch stages) and module.py:134-194 (differentiable_warping). All arithmetic is fp32; activations are
// channels-last, so a bilinear tap of a C-channel feature is one contiguous read. The blob layout is documented next to
// gtsfm_patchmatchnet_weights_floats in gtsfm_hip.h.
#include "common.hpp"

namespace {

constexpr int kInitBins = 48;
constexpr int kEvalNb = 9;
constexpr int kMlpHidden0 = 16, kMlpHidden1 = 8;

struct StageCfg {
    int C, G, dil, iters, Ns, Np;
    float scale;
};
// index 0 = stage 1 (half resolution) ... 2 = stage 3 (eighth resolution)
const StageCfg kStage[3] = {{16, 4, 6, 1, 8, 0, 0.005f}, {32, 8, 4, 2, 8, 8, 0.0125f}, {64, 8, 2, 2, 16, 16, 0.025f}};

constexpr size_t conv_floats(int k, int cin, int cout) { return (size_t)k * k * cin * cout + cout; }
constexpr size_t mlp_floats(int g) { return (size_t)g * kMlpHidden0 + kMlpHidden0 + kMlpHidden0 * kMlpHidden1 + kMlpHidden1 + kMlpHidden1 + 1; }

// Offsets (in floats) of every layer in the blob, in the order pack_patchmatchnet_weights writes them.
struct Blob {
    size_t fconv[11], output1, inner1, inner2, output2, output3;
    size_t pixel, sim[3], propa[3], eval[3], fwn[3];  // [stage - 1]
    size_t rconv0, rconv1, rconv2, rdeconv, rconv3, rres, total;
    Blob() {
        static const int fc[11][3] = {{3, 3, 8}, {3, 8, 8}, {5, 8, 16}, {3, 16, 16}, {3, 16, 16}, {5, 16, 32},
                                      {3, 32, 32}, {3, 32, 32}, {5, 32, 64}, {3, 64, 64}, {3, 64, 64}};
        size_t o = 0;
        auto put = [&](size_t n) { size_t at = o; o += n; return at; };
        for (int i = 0; i < 11; ++i) fconv[i] = put(conv_floats(fc[i][0], fc[i][1], fc[i][2]));
        output1 = put(conv_floats(1, 64, 64));
        inner1 = put(conv_floats(1, 32, 64));
        inner2 = put(conv_floats(1, 16, 64));
        output2 = put(conv_floats(1, 64, 32));
        output3 = put(conv_floats(1, 64, 16));
        pixel = 0;
        for (int l = 2; l >= 0; --l) {
            const StageCfg& c = kStage[l];
            if (l == 2) pixel = put(mlp_floats(c.G));
            sim[l] = put(mlp_floats(c.G));
            propa[l] = c.Np ? put(conv_floats(3, c.C, 2 * c.Np)) : 0;
            eval[l] = put(conv_floats(3, c.C, 2 * kEvalNb));
            fwn[l] = put(mlp_floats(c.G));
        }
        rconv0 = put(conv_floats(3, 3, 8));
        rconv1 = put(conv_floats(3, 1, 8));
        rconv2 = put(conv_floats(3, 8, 8));
        rdeconv = put(conv_floats(3, 8, 8));
        rconv3 = put(conv_floats(3, 16, 8));
        rres = put(conv_floats(3, 8, 1));
        total = o;
    }
};

// ---------------------------------------------------------------------------------------------------------------
// Convolutions
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float load_act(const float* p) { return *p; }
__device__ __forceinline__ float load_act(const uint8_t* p) { return (float)*p / 255.0f; }

// Direct fp32 convolution, 16 x 16 output pixels per workgroup, one pixel and all COUT channels per lane. The input
// tile goes through LDS eight channels at a time, one plane per channel so that neighbouring lanes read neighbouring
// words. Weights are W[ky][kx][ci][co] followed by bias[co] (BatchNorm folded in); a lane reads them at wave-uniform
// addresses. Output pixel stride out_c and channel offset out_off let two layers write one concatenated map.
template <int K, int S, int CIN, int COUT, bool RELU, int MAXDIL, typename TIN>
__global__ __launch_bounds__(256) void pm_conv_kernel(const TIN* __restrict__ in, const float* __restrict__ w,
                                                      float* __restrict__ out, int H, int W, int Ho, int Wo, int dil,
                                                      int pad, int out_c, int out_off) {
    constexpr int CCH = CIN < 8 ? CIN : 8;
    constexpr int TMAX = 15 * S + (K - 1) * MAXDIL + 1;
    __shared__ float tile[CCH][TMAX][TMAX + 1];
    const int tin = 15 * S + (K - 1) * dil + 1;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int ox = blockIdx.x * 16 + tx, oy = blockIdx.y * 16 + ty;
    const int ix0 = blockIdx.x * 16 * S - pad, iy0 = blockIdx.y * 16 * S - pad;
    const TIN* inv = in + (size_t)blockIdx.z * H * W * CIN;
    const float* bias = w + (size_t)K * K * CIN * COUT;
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = bias[co];
    for (int c0 = 0; c0 < CIN; c0 += CCH) {
        __syncthreads();
        for (int i = threadIdx.x; i < tin * tin; i += 256) {
            const int r = i / tin, c = i - r * tin;
            const int iy = iy0 + r, ix = ix0 + c;
            const bool ok = iy >= 0 && iy < H && ix >= 0 && ix < W;
            const TIN* p = inv + ((size_t)(ok ? iy : 0) * W + (ok ? ix : 0)) * CIN + c0;
#pragma unroll
            for (int cc = 0; cc < CCH; ++cc) tile[cc][r][c] = ok ? load_act(p + cc) : 0.0f;
        }
        __syncthreads();
#pragma unroll 1
        for (int ky = 0; ky < K; ++ky) {
#pragma unroll 1
            for (int kx = 0; kx < K; ++kx) {
                const float* wp = w + ((size_t)(ky * K + kx) * CIN + c0) * COUT;
#pragma unroll
                for (int cc = 0; cc < CCH; ++cc) {
                    const float x = tile[cc][ty * S + ky * dil][tx * S + kx * dil];
#pragma unroll
                    for (int co = 0; co < COUT; ++co) acc[co] = fmaf(x, wp[cc * COUT + co], acc[co]);
                }
            }
        }
    }
    if (ox < Wo && oy < Ho) {
        float* o = out + (((size_t)blockIdx.z * Ho + oy) * Wo + ox) * out_c + out_off;
#pragma unroll
        for (int co = 0; co < COUT; ++co) o[co] = RELU ? fmaxf(acc[co], 0.0f) : acc[co];
    }
}

template <int K, int S, int CIN, int COUT, bool RELU, int MAXDIL, typename TIN>
int launch_conv(const TIN* in, const float* w, float* out, int n, int H, int W, int dil, int pad, int out_c,
                int out_off, hipStream_t stream) {
    if (dil > MAXDIL) return GTSFM_ERR_ARG;
    const int Ho = (H + 2 * pad - dil * (K - 1) - 1) / S + 1, Wo = (W + 2 * pad - dil * (K - 1) - 1) / S + 1;
    dim3 grid(blocks_for(Wo, 16), blocks_for(Ho, 16), n);
    hipLaunchKernelGGL((pm_conv_kernel<K, S, CIN, COUT, RELU, MAXDIL, TIN>), grid, dim3(256), 0, stream, in, w, out, H,
                       W, Ho, Wo, dil, pad, out_c ? out_c : COUT, out_off);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

// Refinement's ConvTranspose2d (k3, stride 2, pad 1, output_pad 1) + BatchNorm + ReLU, 8 -> 8 channels:
// out[oy][ox] takes in[iy][ix] through tap (ky, kx) where oy = 2 iy - 1 + ky. W[ky][kx][ci][co], then bias.
__global__ __launch_bounds__(256) void pm_deconv_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                        float* __restrict__ out, int n, int h, int wd, int out_c,
                                                        int out_off) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int Ho = 2 * h, Wo = 2 * wd;
    if (idx >= (size_t)n * Ho * Wo) return;
    const int ox = (int)(idx % Wo), oy = (int)((idx / Wo) % Ho), v = (int)(idx / ((size_t)Wo * Ho));
    float acc[8];
#pragma unroll
    for (int co = 0; co < 8; ++co) acc[co] = w[9 * 64 + co];
    for (int ky = 0; ky < 3; ++ky) {
        const int ty = oy + 1 - ky;
        if (ty < 0 || (ty & 1) || (ty >> 1) >= h) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int tx = ox + 1 - kx;
            if (tx < 0 || (tx & 1) || (tx >> 1) >= wd) continue;
            const float* p = in + (((size_t)v * h + (ty >> 1)) * wd + (tx >> 1)) * 8;
            const float* wp = w + (ky * 3 + kx) * 64;
#pragma unroll
            for (int ci = 0; ci < 8; ++ci)
#pragma unroll
                for (int co = 0; co < 8; ++co) acc[co] = fmaf(p[ci], wp[ci * 8 + co], acc[co]);
        }
    }
    float* o = out + idx * out_c + out_off;
#pragma unroll
    for (int co = 0; co < 8; ++co) o[co] = fmaxf(acc[co], 0.0f);
}

// out[v][y][x][c] += bilinear x2 upsample of a[v][y/2..][x/2..][c] (F.interpolate, align_corners=False).
__global__ __launch_bounds__(256) void pm_upsample_add_kernel(const float* __restrict__ a, float* __restrict__ out, int n,
                                                              int h, int w, int C) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int Ho = 2 * h, Wo = 2 * w;
    if (idx >= (size_t)n * Ho * Wo * C) return;
    const int c = (int)(idx % C);
    const size_t pix = idx / C;
    const int ox = (int)(pix % Wo), oy = (int)((pix / Wo) % Ho), v = (int)(pix / ((size_t)Wo * Ho));
    const float sy = fmaxf((oy + 0.5f) * 0.5f - 0.5f, 0.0f), sx = fmaxf((ox + 0.5f) * 0.5f - 0.5f, 0.0f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);
    const float ly = sy - y0, lx = sx - x0;
    const float* av = a + (size_t)v * h * w * C + c;
    const float top = (1.0f - lx) * av[((size_t)y0 * w + x0) * C] + lx * av[((size_t)y0 * w + x1) * C];
    const float bot = (1.0f - lx) * av[((size_t)y1 * w + x0) * C] + lx * av[((size_t)y1 * w + x1) * C];
    out[idx] += (1.0f - ly) * top + ly * bot;
}

// ---------------------------------------------------------------------------------------------------------------
// Patchmatch helpers
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// A position in pixels to grid_sample's source index with the reference's quirk: normalised as x / ((W - 1) / 2) - 1,
// un-normalised as for align_corners=False, clamped to the border.
__device__ __forceinline__ float border_index(float p, int size) {
    const float g = p / ((size - 1) * 0.5f) - 1.0f;
    const float i = ((g + 1.0f) * size - 1.0f) * 0.5f;
    return fminf(fmaxf(i, 0.0f), (float)(size - 1));
}

// Four bilinear taps: pixel offsets (row * W + col) and weights; a tap outside the map has weight 0 and offset 0.
struct Taps {
    int o[4];
    float w[4];
};

__device__ __forceinline__ Taps make_taps(float ix, float iy, int H, int W) {
    Taps t;
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float wx1 = ix - fx, wy1 = iy - fy, wx0 = (fx + 1.0f) - ix, wy0 = (fy + 1.0f) - iy;
    const int xs[4] = {x0, x0 + 1, x0, x0 + 1}, ys[4] = {y0, y0, y0 + 1, y0 + 1};
    const float ws[4] = {wx0 * wy0, wx1 * wy0, wx0 * wy1, wx1 * wy1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ok = xs[k] >= 0 && xs[k] < W && ys[k] >= 0 && ys[k] < H;
        t.o[k] = ok ? ys[k] * W + xs[k] : 0;
        t.w[k] = ok ? ws[k] : 0.0f;
    }
    return t;
}

__device__ __forceinline__ Taps border_taps(float px, float py, int H, int W) {
    return make_taps(border_index(px, W), border_index(py, H), H, W);
}

// The 1x1x1 nets (BatchNorm folded): W0[G][16], b0[16], W1[16][8], b1[8], W2[8], b2. Returns the value before any
// sigmoid.
template <int G>
__device__ __forceinline__ float mlp_eval(const float* __restrict__ m, const float (&x)[G]) {
    float h0[kMlpHidden0], h1[kMlpHidden1];
    const float* b0 = m + G * kMlpHidden0;
#pragma unroll
    for (int o = 0; o < kMlpHidden0; ++o) h0[o] = b0[o];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int o = 0; o < kMlpHidden0; ++o) h0[o] = fmaf(x[g], m[g * kMlpHidden0 + o], h0[o]);
    const float* w1 = b0 + kMlpHidden0;
    const float* b1 = w1 + kMlpHidden0 * kMlpHidden1;
#pragma unroll
    for (int o = 0; o < kMlpHidden1; ++o) h1[o] = b1[o];
#pragma unroll
    for (int i = 0; i < kMlpHidden0; ++i) {
        const float a = fmaxf(h0[i], 0.0f);
#pragma unroll
        for (int o = 0; o < kMlpHidden1; ++o) h1[o] = fmaf(a, w1[i * kMlpHidden1 + o], h1[o]);
    }
    const float* w2 = b1 + kMlpHidden1;
    float y = w2[kMlpHidden1];
#pragma unroll
    for (int i = 0; i < kMlpHidden1; ++i) y = fmaf(fmaxf(h1[i], 0.0f), w2[i], y);
    return y;
}

// Group-wise mean correlation of the reference feature at a pixel with the feature of `map` gathered through taps.
template <int C, int G>
__device__ __forceinline__ void group_correlation(const float* __restrict__ ref, const float* __restrict__ map,
                                                  const Taps& t, float (&sim)[G]) {
    constexpr int CG = C / G;
    const float4* r4 = reinterpret_cast<const float4*>(ref);
    const float4* m4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m4[k] = reinterpret_cast<const float4*>(map + (size_t)t.o[k] * C);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < CG / 4; ++q) {
            const int i = g * (CG / 4) + q;
            const float4 a = m4[0][i], b = m4[1][i], c = m4[2][i], d = m4[3][i], r = r4[i];
            s = fmaf(t.w[0] * a.x + t.w[1] * b.x + t.w[2] * c.x + t.w[3] * d.x, r.x, s);
            s = fmaf(t.w[0] * a.y + t.w[1] * b.y + t.w[2] * c.y + t.w[3] * d.y, r.y, s);
            s = fmaf(t.w[0] * a.z + t.w[1] * b.z + t.w[2] * c.z + t.w[3] * d.z, r.z, s);
            s = fmaf(t.w[0] * a.w + t.w[1] * b.w + t.w[2] * c.w + t.w[3] * d.w, r.w, s);
        }
        sim[g] = s / (float)CG;
    }
}

// differentiable_warping for one pixel and depth: the taps of the source feature (align_corners=True, zero padding).
// pr = rot (9, row-major) and trans (3) of src_proj ref_proj^-1.
__device__ __forceinline__ Taps warp_taps(const float* __restrict__ pr, int x, int y, float depth, int H, int W) {
    const float fx = (float)x, fy = (float)y;
    float px = (pr[0] * fx + pr[1] * fy + pr[2]) * depth + pr[9];
    float py = (pr[3] * fx + pr[4] * fy + pr[5]) * depth + pr[10];
    float pz = (pr[6] * fx + pr[7] * fy + pr[8]) * depth + pr[11];
    if (pz <= 1e-3f) {
        px = (float)W;
        py = (float)H;
        pz = 1.0f;
    }
    const float gx = (px / pz) / ((W - 1) * 0.5f) - 1.0f, gy = (py / pz) / ((H - 1) * 0.5f) - 1.0f;
    const float ix = (gx + 1.0f) * 0.5f * (W - 1), iy = (gy + 1.0f) * 0.5f * (H - 1);
    if (!(ix > -1.0f && ix < (float)W && iy > -1.0f && iy < (float)H)) {  // also catches NaN: nothing is read
        Taps t;
#pragma unroll
        for (int k = 0; k < 4; ++k) t.o[k] = 0, t.w[k] = 0.0f;
        return t;
    }
    return make_taps(ix, iy, H, W);
}

// Ascending bitonic sort of N registers (N a power of two): every index is a compile-time constant.
template <int N>
__device__ __forceinline__ void sort_registers(float (&a)[N]) {
#pragma unroll
    for (int k = 2; k <= N; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float lo = fminf(a[i], a[l]), hi = fmaxf(a[i], a[l]);
                    const bool up = (i & k) == 0;
                    a[i] = up ? lo : hi;
                    a[l] = up ? hi : lo;
                }
            }
}

// ---------------------------------------------------------------------------------------------------------------
// Patchmatch kernels. Per-view maps are [view][pixel], volumes [view][pixel][D], features [view][pixel][C].
// ---------------------------------------------------------------------------------------------------------------

// proj[stage - 1][view][s] = rot (9) and trans (3) of src_proj ref_proj^-1, in fp64 from the poses, rounded once:
// rot = K_s R_s' R_r K_r^-1, trans = K_s R_s' (c_r - c_s), K = diag-plus-offset of (f, u0, v0) with its first two rows
// divided by 2^stage (patchmatchnet_data.py:208-227). An invalid source index leaves zeros.
__global__ void pm_proj_kernel(const double* __restrict__ wRc, const double* __restrict__ wtc,
                               const double* __restrict__ intr, const int* __restrict__ src_views, int n, int S,
                               float* __restrict__ proj) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 3 * n * S) return;
    const int s = idx % S, v = (idx / S) % n, l = idx / (S * n);
    float* o = proj + (size_t)idx * 12;
    const int sv = src_views[v * S + s];
    if (sv < 0 || sv >= n) {
        for (int i = 0; i < 12; ++i) o[i] = 0.0f;
        return;
    }
    const double sc = 1.0 / (double)(2 << l);
    const double* Rr = wRc + 9 * v;
    const double* Rs = wRc + 9 * sv;
    const double fr = intr[3 * v] * sc, ur = intr[3 * v + 1] * sc, vr = intr[3 * v + 2] * sc;
    const double fs = intr[3 * sv] * sc, us = intr[3 * sv + 1] * sc, vs = intr[3 * sv + 2] * sc;
    double M[9], d[3], m[3];  // M = R_s' R_r, d = R_s' (c_r - c_s)
    for (int i = 0; i < 3; ++i) d[i] = wtc[3 * v + i] - wtc[3 * sv + i];
    for (int i = 0; i < 3; ++i) {
        m[i] = Rs[i] * d[0] + Rs[3 + i] * d[1] + Rs[6 + i] * d[2];
        for (int j = 0; j < 3; ++j) M[3 * i + j] = Rs[i] * Rr[j] + Rs[3 + i] * Rr[3 + j] + Rs[6 + i] * Rr[6 + j];
    }
    double A[9];  // K_s M
    for (int j = 0; j < 3; ++j) {
        A[j] = fs * M[j] + us * M[6 + j];
        A[3 + j] = fs * M[3 + j] + vs * M[6 + j];
        A[6 + j] = M[6 + j];
    }
    for (int i = 0; i < 3; ++i) {  // times K_r^-1 = [[1/f, 0, -u/f], [0, 1/f, -v/f], [0, 0, 1]]
        o[3 * i] = (float)(A[3 * i] / fr);
        o[3 * i + 1] = (float)(A[3 * i + 1] / fr);
        o[3 * i + 2] = (float)(A[3 * i + 2] - (A[3 * i] * ur + A[3 * i + 1] * vr) / fr);
    }
    o[9] = (float)(fs * m[0] + us * m[2]);
    o[10] = (float)(fs * m[1] + vs * m[2]);
    o[11] = (float)m[2];
}

__global__ void pm_depth_range_kernel(const double* __restrict__ range, int n, float* __restrict__ out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const float dmin = (float)range[2 * v], dmax = (float)range[2 * v + 1];
    out[4 * v] = dmin;
    out[4 * v + 1] = dmax;
    out[4 * v + 2] = 1.0f / dmin;
    out[4 * v + 3] = 1.0f / dmax;
}

__device__ __forceinline__ void eval_offset(int nb, int dil, int& dy, int& dx) {
    dy = (nb / 3 - 1) * dil;
    dx = (nb % 3 - 1) * dil;
}

// FeatureWeightNet: the 9 evaluation neighbours of the reference feature, group correlation with the centre, the net,
// sigmoid. fw[view][pixel][9].
template <int C, int G>
__global__ __launch_bounds__(256) void pm_feature_weight_kernel(const float* __restrict__ feat,
                                                                const float* __restrict__ eoff,
                                                                const float* __restrict__ net, float* __restrict__ fw,
                                                                int n, int H, int W, int dil) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int P = H * W;
    if (idx >= (size_t)n * P * kEvalNb) return;
    const int nb = (int)(idx % kEvalNb);
    const size_t vp = idx / kEvalNb;
    const int pix = (int)(vp % P), v = (int)(vp / P);
    const int x = pix % W, y = pix / W;
    int dy, dx;
    eval_offset(nb, dil - 1, dy, dx);
    const float* off = eoff + vp * (2 * kEvalNb);
    const Taps t = border_taps((float)x + ((float)dx + off[2 * nb]), (float)y + ((float)dy + off[2 * nb + 1]), H, W);
    float sim[G];
    group_correlation<C, G>(feat + vp * C, feat + (size_t)v * P * C, t, sim);
    fw[idx] = sigmoidf(mlp_eval<G>(net, sim));
}

// Random initialisation on stage 3: 48 inverse-depth bins, one uniform number each. Writes the samples and their
// normalised inverse depth xn = (1/d - 1/max) / (1/min - 1/max).
__global__ __launch_bounds__(256) void pm_init_samples_kernel(const float* __restrict__ uniform,
                                                              const float* __restrict__ range,
                                                              float* __restrict__ samples, float* __restrict__ xn,
                                                              int n, int P) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * P * kInitBins) return;
    const int d = (int)(idx % kInitBins);
    const size_t vp = idx / kInitBins;
    const int pix = (int)(vp % P), v = (int)(vp / P);
    const float inv_min = range[4 * v + 2], inv_max = range[4 * v + 3];
    const float u = uniform[((size_t)v * kInitBins + d) * P + pix];
    const float s = 1.0f / (inv_max + (u + (float)d) / (float)kInitBins * (inv_min - inv_max));
    samples[idx] = s;
    xn[idx] = (1.0f / s - inv_max) / (inv_min - inv_max);
}

// Local perturbation around the previous depth (NS samples in inverse depth, clamped to the view's range) and
// adaptive propagation (NP bilinear, border-padded reads of the neighbours' central sample), sorted ascending.
// `shift` = 1 reads the previous depth from the map of half the size (nearest x2 upsampling between stages).
template <int NS, int NP>
__global__ __launch_bounds__(256) void pm_perturb_kernel(const float* __restrict__ prev, int shift,
                                                         const float* __restrict__ poff,
                                                         const float* __restrict__ range, float scale,
                                                         float* __restrict__ samples, float* __restrict__ xn, int n,
                                                         int H, int W, int dil) {
    const size_t vp = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int P = H * W;
    if (vp >= (size_t)n * P) return;
    const int pix = (int)(vp % P), v = (int)(vp / P);
    const int x = pix % W, y = pix / W;
    const int Wp = W >> shift;
    const float* pv = prev + (size_t)v * (H >> shift) * Wp;
    const float inv_min = range[4 * v + 2], inv_max = range[4 * v + 3];
    const float interval = (inv_min - inv_max) * scale;
    float a[NS + NP];
    const float inv0 = 1.0f / pv[(y >> shift) * Wp + (x >> shift)];
#pragma unroll
    for (int k = 0; k < NS; ++k)
        a[k] = 1.0f / fminf(fmaxf(inv0 + interval * (float)(k - NS / 2), inv_max), inv_min);
    if (NP > 0) {
        const float* off = poff + vp * (2 * NP);
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int ring = i & 7, mul = i < 8 ? dil : 2 * dil;
            const int r3 = ring < 4 ? ring : ring + 1;  // the 3 x 3 ring without its centre
            const int dy = (r3 / 3 - 1) * mul, dx = (r3 % 3 - 1) * mul;
            const Taps t = border_taps((float)x + ((float)dx + off[2 * i]), (float)y + ((float)dy + off[2 * i + 1]), H, W);
            float s = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int qx = t.o[k] % W, qy = t.o[k] / W;
                const float dq = pv[(qy >> shift) * Wp + (qx >> shift)];
                s += t.w[k] * (1.0f / fminf(fmaxf(1.0f / dq, inv_max), inv_min));
            }
            a[NS + i] = s;
        }
        sort_registers<NS + NP>(a);
    }
    float* so = samples + vp * (NS + NP);
    float* xo = xn + vp * (NS + NP);
#pragma unroll
    for (int k = 0; k < NS + NP; ++k) {
        so[k] = a[k];
        xo[k] = (1.0f / a[k] - inv_max) / (inv_min - inv_max);
    }
}

// PixelwiseNet on stage 3's first iteration: per (view, source, pixel) the maximum over the depth samples of
// sigmoid(net(similarity)). vw[view][s][pixel].
template <int C, int G>
__global__ __launch_bounds__(256) void pm_view_weight_kernel(const float* __restrict__ feat,
                                                             const float* __restrict__ samples,
                                                             const float* __restrict__ proj,
                                                             const int* __restrict__ src_views,
                                                             const float* __restrict__ net, float* __restrict__ vw,
                                                             int n, int S, int H, int W, int D) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int P = H * W;
    if (idx >= (size_t)n * S * P) return;
    const int pix = (int)(idx % P), s = (int)((idx / P) % S), v = (int)(idx / ((size_t)P * S));
    const int sv = src_views[v * S + s];
    if (sv < 0 || sv >= n) {
        vw[idx] = 0.0f;
        return;
    }
    const float* pr = proj + ((size_t)v * S + s) * 12;
    const float* ref = feat + ((size_t)v * P + pix) * C;
    const float* src = feat + (size_t)sv * P * C;
    const float* sm = samples + ((size_t)v * P + pix) * D;
    float best = 0.0f;
    for (int d = 0; d < D; ++d) {
        const Taps t = warp_taps(pr, pix % W, pix / W, sm[d], H, W);
        float sim[G];
        group_correlation<C, G>(ref, src, t, sim);
        best = fmaxf(best, sigmoidf(mlp_eval<G>(net, sim)));
    }
    vw[idx] = best;
}

// The matching cost of one patchmatch iteration, one lane per (view, pixel, depth sample): over the source views the
// warp, the 4-tap gather, the group correlation and the view-weighted mean, then SimilarityNet's 1x1x1 convs.
// vw is stage 3's map; vshift = log2 of this stage's size over stage 3's (nearest upsampling). cost[view][pixel][D].
template <int C, int G>
__global__ __launch_bounds__(256) void pm_cost_kernel(const float* __restrict__ feat, const float* __restrict__ samples,
                                                      const float* __restrict__ proj,
                                                      const int* __restrict__ src_views, const float* __restrict__ vw,
                                                      int vshift, const float* __restrict__ net,
                                                      float* __restrict__ cost, int n, int S, int H, int W, int D) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int P = H * W;
    if (idx >= (size_t)n * P * D) return;
    const size_t vp = idx / D;
    const int pix = (int)(vp % P), v = (int)(vp / P);
    const int x = pix % W, y = pix / W;
    const int W3 = W >> vshift, P3 = (H >> vshift) * W3;
    const int pix3 = (y >> vshift) * W3 + (x >> vshift);
    const float depth = samples[idx];
    const float* ref = feat + vp * C;
    float sum[G], wsum = 0.0f;
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = 0.0f;
    for (int s = 0; s < S; ++s) {
        const int sv = src_views[v * S + s];
        if (sv < 0 || sv >= n) continue;
        const Taps t = warp_taps(proj + ((size_t)v * S + s) * 12, x, y, depth, H, W);
        float sim[G];
        group_correlation<C, G>(ref, feat + (size_t)sv * P * C, t, sim);
        const float wv = vw[((size_t)v * S + s) * P3 + pix3];
#pragma unroll
        for (int g = 0; g < G; ++g) sum[g] = fmaf(sim[g], wv, sum[g]);
        wsum += wv;
    }
    // No valid source, or every view weight underflowed: the reference's 0 / 0. mlp_eval's fmaxf would turn that NaN
    // into a finite constant cost (uniform scores, confidence 0.5), so the NaN is written as it is and reaches the
    // view's depth and confidence.
    if (!(wsum > 0.0f)) {
        cost[idx] = __builtin_nanf("");
        return;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] /= wsum;
    cost[idx] = mlp_eval<G>(net, sum);
}

// Adaptive spatial aggregation, softmax over depth and regression, one lane per (view, pixel). For each of the 9
// evaluation neighbours: the bilinear, border-padded cost and normalised inverse depth of every sample, the depth
// weight sigmoid(2 (2 - min(|xn_nb - xn| / scale, 4))) times the feature weight, normalised over the neighbours.
// LAST (stage 1's only iteration): inverse-depth index regression between the first and last sample, and the
// confidence = the four probabilities around the truncated index, written x2 nearest-upsampled.
template <int D, bool LAST>
__global__ __launch_bounds__(256) void pm_aggregate_kernel(const float* __restrict__ cost, const float* __restrict__ xn,
                                                           const float* __restrict__ samples,
                                                           const float* __restrict__ eoff, const float* __restrict__ fw,
                                                           float scale, float* __restrict__ depth_out,
                                                           float* __restrict__ conf_out, int n, int H, int W, int dil) {
    const size_t vp = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int P = H * W;
    if (vp >= (size_t)n * P) return;
    const int pix = (int)(vp % P), v = (int)(vp / P);
    const int x = pix % W, y = pix / W;
    const float* off = eoff + vp * (2 * kEvalNb);
    const float* xc = xn + vp * D;
    const float* cv = cost + (size_t)v * P * D;
    const float* xv = xn + (size_t)v * P * D;
    float acc[D], ws[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = 0.0f, ws[d] = 0.0f;
#pragma unroll 1
    for (int nb = 0; nb < kEvalNb; ++nb) {
        int dy, dx;
        eval_offset(nb, dil - 1, dy, dx);
        const Taps t = border_taps((float)x + ((float)dx + off[2 * nb]), (float)y + ((float)dy + off[2 * nb + 1]), H, W);
        const float f = fw[vp * kEvalNb + nb];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            float xs = 0.0f, cs = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                xs = fmaf(t.w[k], xv[(size_t)t.o[k] * D + d], xs);
                cs = fmaf(t.w[k], cv[(size_t)t.o[k] * D + d], cs);
            }
            const float diff = fminf(fabsf(xs - xc[d]) / scale, 4.0f);
            const float w = sigmoidf((2.0f - diff) * 2.0f) * f;
            ws[d] += w;
            acc[d] = fmaf(cs, w, acc[d]);
        }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        acc[d] /= ws[d];
        mx = fmaxf(mx, acc[d]);
    }
    float den = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        acc[d] = expf(acc[d] - mx);
        den += acc[d];
    }
    const float* sm = samples + vp * D;
    if (!LAST) {
        float e = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) e = fmaf(sm[d], acc[d] / den, e);
        depth_out[vp] = e;
    } else {
        float index = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            acc[d] /= den;
            index = fmaf((float)d, acc[d], index);
        }
        const float inv_far = 1.0f / sm[0], inv_near = 1.0f / sm[D - 1];
        depth_out[vp] = 1.0f / (inv_far + index / (float)(D - 1) * (inv_near - inv_far));
        const int k = min(max((int)index, 0), D - 1);
        float c = 0.0f;
#pragma unroll
        for (int d = 0; d < D; ++d) c += (d >= k - 1 && d <= k + 2) ? acc[d] : 0.0f;
        float* co = conf_out + (size_t)v * 4 * P + (size_t)(2 * y) * (2 * W) + 2 * x;
        co[0] = c;
        co[1] = c;
        co[2 * W] = c;
        co[2 * W + 1] = c;
    }
}

// Refinement's ends: depth (at half size) to [0, 1] of the view's range; and the x2 nearest upsample of that plus the
// residual, back to the range.
__global__ __launch_bounds__(256) void pm_normalise_kernel(const float* __restrict__ depth,
                                                           const float* __restrict__ range, float* __restrict__ out,
                                                           int n, int P) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * P) return;
    const int v = (int)(idx / P);
    const float dmin = range[4 * v], dmax = range[4 * v + 1];
    out[idx] = (depth[idx] - dmin) / (dmax - dmin);
}

__global__ __launch_bounds__(256) void pm_residual_kernel(const float* __restrict__ dn, const float* __restrict__ res,
                                                          const float* __restrict__ range, float* __restrict__ out,
                                                          int n, int H, int W) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * H * W) return;
    const int x = (int)(idx % W), y = (int)((idx / W) % H), v = (int)(idx / ((size_t)W * H));
    const float dmin = range[4 * v], dmax = range[4 * v + 1];
    const float d = dn[((size_t)v * (H / 2) + y / 2) * (W / 2) + x / 2] + res[idx];
    out[idx] = d * (dmax - dmin) + dmin;
}

// ---------------------------------------------------------------------------------------------------------------
// Workspace
// ---------------------------------------------------------------------------------------------------------------
struct PmLayout {
    size_t a0, a1, b0, b1, c0, c1, d0, d1, feat[3], intra2, intra1;  // FeatureNet; a0 and a1 are adjacent (the cat)
    size_t proj, range, eoff, poff, fw, samples, xn, cost, vw, depth_a, depth_b;
    size_t dn, r0, r1, r2, r3, total;
    PmLayout(int n, int S, int H, int W) {
        const size_t f = sizeof(float), P0 = (size_t)n * H * W, P1 = P0 / 4, P2 = P0 / 16, P3 = P0 / 64;
        WsCarver c;
        a0 = c.take(2 * P0 * 8 * f);  // conv0 / conv1 outputs, later Refinement's 16-channel concatenation
        a1 = a0 + P0 * 8 * f;
        b0 = c.take(P1 * 16 * f);
        b1 = c.take(P1 * 16 * f);
        c0 = c.take(P2 * 32 * f);
        c1 = c.take(P2 * 32 * f);
        d0 = c.take(P3 * 64 * f);
        d1 = c.take(P3 * 64 * f);
        feat[0] = c.take(P1 * 16 * f);
        feat[1] = c.take(P2 * 32 * f);
        feat[2] = c.take(P3 * 64 * f);
        intra2 = c.take(P2 * 64 * f);
        intra1 = c.take(P1 * 64 * f);
        proj = c.take((size_t)3 * n * S * 12 * f);
        range = c.take((size_t)n * 4 * f);
        eoff = c.take(P1 * 2 * kEvalNb * f);
        poff = c.take(P2 * 16 * f);          // stage 2: 16 channels at P2; stage 3: 32 at P3
        fw = c.take(P1 * kEvalNb * f);
        samples = c.take(P1 * 8 * f);        // 8 at P1 = 32 at P2 = 128 at P3: covers 16 at P2 and 48 at P3
        xn = c.take(P1 * 8 * f);
        cost = c.take(P1 * 8 * f);
        vw = c.take(P3 * S * f);
        depth_a = c.take(P1 * f);
        depth_b = c.take(P1 * f);
        dn = c.take(P1 * f);
        r0 = c.take(P1 * 8 * f);
        r1 = c.take(P1 * 8 * f);
        r2 = c.take(P0 * 8 * f);
        r3 = c.take(P0 * f);
        total = c.o;
    }
};

bool shape_ok(int n, int S, int H, int W) {
    return n > 0 && S > 0 && H >= 16 && W >= 16 && H % 8 == 0 && W % 8 == 0 && (long long)n * H * W < (1ll << 31) / 16;
}

const gtsfm_patchmatchnet_config kReferenceConfig = {{0.005, 0.0125, 0.025}, {6, 4, 2}, {1, 2, 2}, {8, 8, 16},
                                                     {0, 8, 16},             {9, 9, 9}, {4, 8, 8}};

bool config_ok(const gtsfm_patchmatchnet_config* c) {
    if (!c) return true;
    for (int i = 0; i < 3; ++i) {
        const gtsfm_patchmatchnet_config& r = kReferenceConfig;
        if (c->interval_scale[i] != r.interval_scale[i] || c->propagation_range[i] != r.propagation_range[i] ||
            c->iterations[i] != r.iterations[i] || c->num_samples[i] != r.num_samples[i] ||
            c->propagate_neighbors[i] != r.propagate_neighbors[i] ||
            c->evaluate_neighbors[i] != r.evaluate_neighbors[i] || c->groups[i] != r.groups[i])
            return false;
    }
    return true;
}

// Measurement hook (gtsfm_patchmatchnet_set_phase_events): six events recorded around the five phases of a call.
hipEvent_t g_phase_events[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

int mark_phase(int i, hipStream_t stream) {
    if (g_phase_events[i]) GTSFM_CHECK_HIP(hipEventRecord(g_phase_events[i], stream));
    return GTSFM_OK;
}

#define PM_TRY(expr)                    \
    do {                                \
        const int _rc = (expr);         \
        if (_rc != GTSFM_OK) return _rc; \
    } while (0)

template <class... KArgs, class... Args>
int launch_1d(void (*kernel)(KArgs...), size_t items, hipStream_t stream, Args... args) {
    hipLaunchKernelGGL(kernel, dim3(blocks_for(items, 256)), dim3(256), 0, stream, static_cast<KArgs>(args)...);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

// One patchmatch stage for all reference views. l = stage - 1.
template <int C, int G, int NS, int NP>
int run_stage(int l, const Blob& B, const float* w, char* ws, const PmLayout& L, const int* src_views,
              const float* uniform, int n, int S, int H, int W, float*& depth_prev, float*& depth_next,
              float* conf_out, float* iter_out, size_t& iter_at, hipStream_t stream) {
    const StageCfg& cfg = kStage[l];
    const int P = H * W;
    const float* feat = (const float*)(ws + L.feat[l]);
    const float* proj = (const float*)(ws + L.proj) + (size_t)l * n * S * 12;
    const float* range = (const float*)(ws + L.range);
    float* eoff = (float*)(ws + L.eoff);
    float* poff = (float*)(ws + L.poff);
    float* fw = (float*)(ws + L.fw);
    float* samples = (float*)(ws + L.samples);
    float* xn = (float*)(ws + L.xn);
    float* cost = (float*)(ws + L.cost);
    float* vw = (float*)(ws + L.vw);
    if constexpr (NP > 0)
        PM_TRY((launch_conv<3, 1, C, 2 * NP, false, 6, float>(feat, w + B.propa[l], poff, n, H, W, cfg.dil, cfg.dil, 0,
                                                              0, stream)));
    PM_TRY((launch_conv<3, 1, C, 2 * kEvalNb, false, 6, float>(feat, w + B.eval[l], eoff, n, H, W, cfg.dil, cfg.dil, 0,
                                                               0, stream)));
    PM_TRY(launch_1d(pm_feature_weight_kernel<C, G>, (size_t)n * P * kEvalNb, stream, feat, (const float*)eoff,
                     w + B.fwn[l], fw, n, H, W, cfg.dil));
    for (int it = 1; it <= cfg.iters; ++it) {
        const bool random_init = l == 2 && it == 1;
        const int D = random_init ? kInitBins : NS + NP;
        if (random_init) {
            PM_TRY(launch_1d(pm_init_samples_kernel, (size_t)n * P * D, stream, uniform, range, samples, xn, n, P));
            PM_TRY(launch_1d(pm_view_weight_kernel<C, G>, (size_t)n * S * P, stream, feat, (const float*)samples, proj,
                             src_views, w + B.pixel, vw, n, S, H, W, D));
        } else {
            // the first iteration of stages 2 and 1 reads the previous stage's map, of half the size
            PM_TRY(launch_1d(pm_perturb_kernel<NS, NP>, (size_t)n * P, stream, (const float*)depth_prev,
                             (l < 2 && it == 1) ? 1 : 0, (const float*)poff, range, cfg.scale, samples, xn, n, H, W,
                             cfg.dil));
        }
        PM_TRY(launch_1d(pm_cost_kernel<C, G>, (size_t)n * P * D, stream, feat, (const float*)samples, proj, src_views,
                         (const float*)vw, 2 - l, w + B.sim[l], cost, n, S, H, W, D));
        const bool last = l == 0 && it == cfg.iters;
        if (random_init)
            PM_TRY(launch_1d(pm_aggregate_kernel<kInitBins, false>, (size_t)n * P, stream, (const float*)cost,
                             (const float*)xn, (const float*)samples, (const float*)eoff, (const float*)fw, cfg.scale,
                             depth_next, conf_out, n, H, W, cfg.dil));
        else if (last)
            PM_TRY(launch_1d(pm_aggregate_kernel<NS + NP, true>, (size_t)n * P, stream, (const float*)cost,
                             (const float*)xn, (const float*)samples, (const float*)eoff, (const float*)fw, cfg.scale,
                             depth_next, conf_out, n, H, W, cfg.dil));
        else
            PM_TRY(launch_1d(pm_aggregate_kernel<NS + NP, false>, (size_t)n * P, stream, (const float*)cost,
                             (const float*)xn, (const float*)samples, (const float*)eoff, (const float*)fw, cfg.scale,
                             depth_next, conf_out, n, H, W, cfg.dil));
        if (iter_out) {
            GTSFM_CHECK_HIP(hipMemcpyAsync(iter_out + iter_at, depth_next, (size_t)n * P * sizeof(float),
                                           hipMemcpyDeviceToDevice, stream));
            iter_at += (size_t)n * P;
        }
        float* t = depth_prev;
        depth_prev = depth_next;
        depth_next = t;
    }
    return GTSFM_OK;
}

}  // namespace

extern "C" {

size_t gtsfm_patchmatchnet_weights_floats(void) {
    static const Blob B;
    return B.total;
}

size_t gtsfm_patchmatchnet_workspace_bytes(int n_views, int n_src, int height, int width) {
    if (!shape_ok(n_views, n_src, height, width)) return 0;
    return PmLayout(n_views, n_src, height, width).total;
}

int gtsfm_patchmatchnet_batched(const uint8_t* d_images, int n_views, int height, int width, const double* d_wRc,
                                const double* d_wtc, const double* d_intrinsics, const int* d_src_views, int n_src,
                                const double* d_depth_range, const float* d_weights, const float* d_init_uniform,
                                const gtsfm_patchmatchnet_config* config, void* d_workspace, size_t workspace_bytes,
                                float* d_depth_out, float* d_confidence_out, float* d_features_out,
                                float* d_iter_depth_out, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    const int n = n_views, S = n_src, H = height, W = width;
    if (!shape_ok(n, S, H, W) || !config_ok(config)) return GTSFM_ERR_ARG;
    if (!d_images || !d_wRc || !d_wtc || !d_intrinsics || !d_src_views || !d_depth_range || !d_weights ||
        !d_init_uniform || !d_workspace || !d_depth_out || !d_confidence_out)
        return GTSFM_ERR_ARG;
    static const Blob B;
    const PmLayout L(n, S, H, W);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    char* ws = (char*)d_workspace;
    const float* w = d_weights;
    auto F = [&](size_t off) { return (float*)(ws + off); };
    const int h1 = H / 2, w1 = W / 2, h2 = H / 4, w2 = W / 4, h3 = H / 8, w3 = W / 8;

    // FeatureNet, once per view
    PM_TRY(mark_phase(0, stream));
    PM_TRY((launch_conv<3, 1, 3, 8, true, 1, uint8_t>(d_images, w + B.fconv[0], F(L.a0), n, H, W, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 8, 8, true, 1, float>(F(L.a0), w + B.fconv[1], F(L.a1), n, H, W, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<5, 2, 8, 16, true, 1, float>(F(L.a1), w + B.fconv[2], F(L.b0), n, H, W, 1, 2, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 16, 16, true, 1, float>(F(L.b0), w + B.fconv[3], F(L.b1), n, h1, w1, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 16, 16, true, 1, float>(F(L.b1), w + B.fconv[4], F(L.b0), n, h1, w1, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<5, 2, 16, 32, true, 1, float>(F(L.b0), w + B.fconv[5], F(L.c0), n, h1, w1, 1, 2, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 32, 32, true, 1, float>(F(L.c0), w + B.fconv[6], F(L.c1), n, h2, w2, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 32, 32, true, 1, float>(F(L.c1), w + B.fconv[7], F(L.c0), n, h2, w2, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<5, 2, 32, 64, true, 1, float>(F(L.c0), w + B.fconv[8], F(L.d0), n, h2, w2, 1, 2, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 64, 64, true, 1, float>(F(L.d0), w + B.fconv[9], F(L.d1), n, h3, w3, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 64, 64, true, 1, float>(F(L.d1), w + B.fconv[10], F(L.d0), n, h3, w3, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<1, 1, 64, 64, false, 1, float>(F(L.d0), w + B.output1, F(L.feat[2]), n, h3, w3, 1, 0, 0, 0, stream)));
    PM_TRY((launch_conv<1, 1, 32, 64, false, 1, float>(F(L.c0), w + B.inner1, F(L.intra2), n, h2, w2, 1, 0, 0, 0, stream)));
    PM_TRY(launch_1d(pm_upsample_add_kernel, (size_t)n * h2 * w2 * 64, stream, (const float*)F(L.d0), F(L.intra2), n, h3, w3, 64));
    PM_TRY((launch_conv<1, 1, 64, 32, false, 1, float>(F(L.intra2), w + B.output2, F(L.feat[1]), n, h2, w2, 1, 0, 0, 0, stream)));
    PM_TRY((launch_conv<1, 1, 16, 64, false, 1, float>(F(L.b0), w + B.inner2, F(L.intra1), n, h1, w1, 1, 0, 0, 0, stream)));
    PM_TRY(launch_1d(pm_upsample_add_kernel, (size_t)n * h1 * w1 * 64, stream, (const float*)F(L.intra2), F(L.intra1), n, h2, w2, 64));
    PM_TRY((launch_conv<1, 1, 64, 16, false, 1, float>(F(L.intra1), w + B.output3, F(L.feat[0]), n, h1, w1, 1, 0, 0, 0, stream)));
    if (d_features_out) {
        const size_t n3 = (size_t)n * h3 * w3 * 64, n2 = (size_t)n * h2 * w2 * 32, n1 = (size_t)n * h1 * w1 * 16;
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_features_out, F(L.feat[2]), n3 * 4, hipMemcpyDeviceToDevice, stream));
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_features_out + n3, F(L.feat[1]), n2 * 4, hipMemcpyDeviceToDevice, stream));
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_features_out + n3 + n2, F(L.feat[0]), n1 * 4, hipMemcpyDeviceToDevice, stream));
    }

    // the three stages
    PM_TRY(mark_phase(1, stream));
    hipLaunchKernelGGL(pm_proj_kernel, dim3(blocks_for((size_t)3 * n * S, 64)), dim3(64), 0, stream, d_wRc, d_wtc,
                       d_intrinsics, d_src_views, n, S, F(L.proj));
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(pm_depth_range_kernel, dim3(blocks_for(n, 64)), dim3(64), 0, stream, d_depth_range, n, F(L.range));
    GTSFM_CHECK_HIP(hipGetLastError());
    float* depth_prev = F(L.depth_a);
    float* depth_next = F(L.depth_b);
    size_t iter_at = 0;
    PM_TRY((run_stage<64, 8, 16, 16>(2, B, w, ws, L, d_src_views, d_init_uniform, n, S, h3, w3, depth_prev, depth_next,
                                     d_confidence_out, d_iter_depth_out, iter_at, stream)));
    PM_TRY(mark_phase(2, stream));
    PM_TRY((run_stage<32, 8, 8, 8>(1, B, w, ws, L, d_src_views, d_init_uniform, n, S, h2, w2, depth_prev, depth_next,
                                   d_confidence_out, d_iter_depth_out, iter_at, stream)));
    PM_TRY(mark_phase(3, stream));
    PM_TRY((run_stage<16, 4, 8, 0>(0, B, w, ws, L, d_src_views, d_init_uniform, n, S, h1, w1, depth_prev, depth_next,
                                   d_confidence_out, d_iter_depth_out, iter_at, stream)));

    // Refinement; depth_prev holds stage 1's map
    PM_TRY(mark_phase(4, stream));
    PM_TRY(launch_1d(pm_normalise_kernel, (size_t)n * h1 * w1, stream, (const float*)depth_prev,
                     (const float*)F(L.range), F(L.dn), n, h1 * w1));
    PM_TRY((launch_conv<3, 1, 1, 8, true, 1, float>(F(L.dn), w + B.rconv1, F(L.r0), n, h1, w1, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 8, 8, true, 1, float>(F(L.r0), w + B.rconv2, F(L.r1), n, h1, w1, 1, 1, 0, 0, stream)));
    PM_TRY(launch_1d(pm_deconv_kernel, (size_t)n * H * W, stream, (const float*)F(L.r1), w + B.rdeconv, F(L.a0), n, h1,
                     w1, 16, 0));
    PM_TRY((launch_conv<3, 1, 3, 8, true, 1, uint8_t>(d_images, w + B.rconv0, F(L.a0), n, H, W, 1, 1, 16, 8, stream)));
    PM_TRY((launch_conv<3, 1, 16, 8, true, 1, float>(F(L.a0), w + B.rconv3, F(L.r2), n, H, W, 1, 1, 0, 0, stream)));
    PM_TRY((launch_conv<3, 1, 8, 1, false, 1, float>(F(L.r2), w + B.rres, F(L.r3), n, H, W, 1, 1, 0, 0, stream)));
    PM_TRY(launch_1d(pm_residual_kernel, (size_t)n * H * W, stream, (const float*)F(L.dn), (const float*)F(L.r3),
                     (const float*)F(L.range), d_depth_out, n, H, W));
    return mark_phase(5, stream);
}

int gtsfm_patchmatchnet_set_phase_events(void* const* events) {
    for (int i = 0; i < 6; ++i) g_phase_events[i] = events ? (hipEvent_t)events[i] : nullptr;
    return GTSFM_OK;
}

}  // extern "C"
