// D2-Net detector-descriptor on gfx950: the single-scale path of thirdparty/d2net/lib/pyramid.py:16-146
// (process_multiscale with scales = [1]) on the network of thirdparty/d2net/lib/model_test.py:12-200, as driven by
// gtsfm/frontend/detector_descriptor/d2net.py:47-88 (USE_MULTISCALE False), batched over same-sized images.
//
//   u8 RGB -> x / 255, (x - mean) / std (utils.py:34-38, 'torch')
//   -> VGG16 to conv4_3 (model_test.py:16-39): conv 3->64, 64->64, max-pool, 64->128, 128->128, max-pool,
//      128->256, 256->256 x 2, 2x2 average pool stride 1, then 256->512, 512->512 x 2 with dilation 2; ReLU after
//      every convolution (use_relu) -> F (512, h, w), h = H / 4 - 1, w = W / 4 - 1
//   -> hard detection (:94-145) + handcrafted localisation (:148-200) + the |step| < 0.5 and corner tests
//      (pyramid.py:84-107, utils.py:111-131) -> candidates in torch.nonzero order (c, i, j)
//   -> top max_keypoints by score (d2net.py:77) -> bilinear descriptors, L2-normalised (utils.py:149-164,
//      pyramid.py:112) -> (x, y) in the input image (utils.py:77-80, pyramid.py:115-116, d2net.py:83-87).
//
// Kernels ("D2-Net"):
// - rgb_conv1_kernel<D2Pre> (conv3.hpp, shared with NetVLAD): the preprocessing fused into the 3 -> 64 convolution
//   (27 fp32 FMAs per output, VALU);
// - conv3_kernel (conv3.hpp, shared with SuperPoint and NetVLAD, as are its launcher and weight splitter): the other
//   nine convolutions as implicit GEMMs on the bf16 matrix cores at fp32 accuracy, the two max-pools fused into the
//   epilogue; the three conv4 layers are its DIL = 2 instantiation (patch halo 2, taps two pixels apart, zero padding);
// - d2_avgpool_kernel: the 2x2 stride-1 average pool, a kernel of its own (half a millisecond beside a 30 ms trunk);
// - d2_detect_kernel: ONE pass over F, one wave per location: channel maximum, then the 3x3 tests, the Hessian, the
//   step and the corner test only for the channels that reach the maximum. Run twice (count, emit) around a prefix
//   scan, so no derivative tensor and no dense mask is ever written;
// - d2_chan_count_kernel / d2_chan_emit_kernel: stable regrouping of the location-ordered list by channel, which is
//   the reference's candidate order. Prefix scans only: no floating-point atomics, no atomics at all;
// - d2_select_kernel (select.hpp's radix select on the score bits, shared with SuperPoint) + d2_rank_kernel (rank by
//   counting): the max_keypoints best in descending score, equal scores by candidate position;
// - d2_describe_kernel: one wave per keypoint, 8 channels per lane, so each corner is one contiguous 2 KB read.
#include <float.h>

#include "common.hpp"

#pragma clang fp contract(off)

#include "conv3.hpp"
#include "select.hpp"

namespace {

struct D2Conv {
    int cin, cout, pool, dil;
};
constexpr int kD2Convs = 10;
constexpr D2Conv kD2[kD2Convs] = {
    {3, 64, 0, 1},    {64, 64, 1, 1},   {64, 128, 0, 1},  {128, 128, 1, 1}, {128, 256, 0, 1},
    {256, 256, 0, 1}, {256, 256, 0, 1}, {256, 512, 0, 2}, {512, 512, 0, 2}, {512, 512, 0, 2},
};
constexpr int kD2Dim = 512;

// ------------------------------------------------------------------ packed weight blob (include/gtsfm_hip.h)
__host__ __device__ constexpr size_t d2_conv_floats(int l) { return (size_t)9 * kD2[l].cin * kD2[l].cout + kD2[l].cout; }
__host__ __device__ constexpr size_t d2_conv_offset(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += d2_conv_floats(i);
    return o;
}
__host__ __device__ constexpr size_t d2_w3_offset(int l) {  // bf16 planes of conv layers 1..9
    size_t o = 0;
    for (int i = 1; i < l; ++i) o += (size_t)3 * 9 * kD2[i].cin * kD2[i].cout;
    return o;
}

// ------------------------------------------------------------------ conv 1's preprocessing (rgb_conv1_kernel)
// utils.py:23, 35-38: float32 image, /= 255.0 in float32, then (image - mean) / std against float64 arrays, narrowed to
// float32 by d2net.py:71. C == 1: the gray value in all three channels (resize_image's np.repeat, d2net.py:106-109).
struct D2Pre {
    __device__ __forceinline__ float operator()(const uint8_t* px, int C, int c) const {
        const double mean[3] = {0.485, 0.456, 0.406}, sd[3] = {0.229, 0.224, 0.225};
        const float t = (float)px[C == 1 ? 0 : c] / 255.0f;
        return (float)(((double)t - mean[c]) / sd[c]);
    }
};

// ------------------------------------------------------------------ AvgPool2d(2, stride=1) (model_test.py:33)
// in (n, Hi, Wi, 256) -> out (n, Hi - 1, Wi - 1, 256); a lane owns four channels of one output location; the window
// is summed in raster order and divided by 4, as torch's CPU kernel does.
__global__ __launch_bounds__(256) void d2_avgpool_kernel(const float* __restrict__ in, int n, int Hi, int Wi,
                                                         float* __restrict__ out) {
    const int Ho = Hi - 1, Wo = Wi - 1;
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)n * Ho * Wo * 64) return;
    const int q = (int)(e & 63);
    const size_t loc = e >> 6;
    const int x = (int)(loc % Wo);
    const int y = (int)((loc / Wo) % Ho);
    const int img = (int)(loc / ((size_t)Wo * Ho));
    const float* p = in + (((size_t)img * Hi + y) * Wi + x) * 256 + 4 * q;
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 256);
    const f32x4 c = *(const f32x4*)(p + (size_t)Wi * 256), d = *(const f32x4*)(p + (size_t)Wi * 256 + 256);
    f32x4 r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = (((a[k] + b[k]) + c[k]) + d[k]) / 4.0f;
    *(f32x4*)(out + loc * 256 + 4 * q) = r;
}

// ------------------------------------------------------------------ detection + localisation, one pass over F
// A candidate: its position in the reference's candidate order is the order of `key` = (c h + i) w + j.
struct D2Cand {
    uint32_t key;
    float score, pi, pj;
};

// The tests of model_test.py:110-145 and :169-200 and pyramid.py:84-107 on element (c, i, j) of one image's map
// F (h, w, 512), whose value v > 0 is already known to be the maximum over the channels. Out-of-map neighbours are 0
// for the derivatives (conv2d's zero padding); for the 3x3 maximum max_pool2d ignores them, which with v > 0 >= 0 is
// the same as comparing against 0. fp32 in the reference's operation order (the 3x3 filter sums are left to right).
__device__ __forceinline__ bool d2_test(const float* __restrict__ F, int h, int w, int c, int i, int j, float v,
                                        float& pi, float& pj) {
    float nb[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int y = i + dy - 1, x = j + dx - 1;
            nb[dy][dx] = (y >= 0 && y < h && x >= 0 && x < w) ? F[((size_t)y * w + x) * kD2Dim + c] : 0.0f;
        }
    float mx = nb[0][0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, nb[k / 3][k % 3]);
    if (v != mx) return false;
    const float dii = (nb[0][1] - 2.0f * v) + nb[2][1];
    const float djj = (nb[1][0] - 2.0f * v) + nb[1][2];
    const float dij = 0.25f * (((nb[0][0] - nb[0][2]) - nb[2][0]) + nb[2][2]);
    const float det = dii * djj - dij * dij;
    const float tr = dii + djj;
    if (!(det > 0.0f) || !(tr * tr / det <= 7.2f)) return false;  // (5 + 1)^2 / 5
    const float h00 = djj / det, h01 = -dij / det, h11 = dii / det;
    const float di = 0.5f * (nb[2][1] - nb[0][1]), dj = 0.5f * (nb[1][2] - nb[1][0]);
    const float si = -(h00 * di + h01 * dj), sj = -(h01 * di + h11 * dj);
    if (!(fabsf(si) < 0.5f) || !(fabsf(sj) < 0.5f)) return false;
    pi = (float)i + si;
    pj = (float)j + sj;
    return floorf(pi) >= 0.0f && ceilf(pi) < (float)h && floorf(pj) >= 0.0f && ceilf(pj) < (float)w;
}

// One wave per location (4 per workgroup), lane l holding channels 8 l .. 8 l + 7. EMIT false: pcnt[location] = its
// number of candidates. EMIT true: they are written at poff[location], in channel order, as long as they fall below
// `cap` per image. A candidate's value is positive (det > 0 needs dii, djj < 0 at a 3x3 maximum of a map >= 0), so a
// location whose maximum is 0 has none.
template <bool EMIT>
__global__ __launch_bounds__(256) void d2_detect_kernel(const float* __restrict__ Fall, int n, int h, int w,
                                                        int* __restrict__ pcnt, const int* __restrict__ poff, int cap,
                                                        D2Cand* __restrict__ list) {
    const size_t hw = (size_t)h * w;
    const size_t loc = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (loc >= (size_t)n * hw) return;
    const int img = (int)(loc / hw);
    const int r = (int)(loc - (size_t)img * hw);
    const int i = r / w, j = r - i * w;
    const float* F = Fall + (size_t)img * hw * kD2Dim;
    const f32x4* src = (const f32x4*)(F + (size_t)r * kD2Dim) + 2 * lane;
    const f32x4 a = src[0], b = src[1];
    float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    float m = v[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) m = fmaxf(m, v[k]);
    m = wave_max(m);
    int cnt = 0;
    float pi[8], pj[8];
    unsigned hit = 0;
    if (m > 0.0f) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (v[k] == m && d2_test(F, h, w, 8 * lane + k, i, j, v[k], pi[k], pj[k])) {
                hit |= 1u << k;
                ++cnt;
            }
    }
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(incl, d);
        if (lane >= d) incl += y;
    }
    if constexpr (!EMIT) {
        if (lane == 63) pcnt[loc] = incl;
    } else {
        int o = poff[loc] + incl - cnt;
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (hit & (1u << k)) {
                if (o < cap) {
                    D2Cand cd;
                    cd.key = (uint32_t)((size_t)(8 * lane + k) * hw + r);
                    cd.score = v[k];
                    cd.pi = pi[k];
                    cd.pj = pj[k];
                    list[(size_t)img * cap + o] = cd;
                }
                ++o;
            }
    }
}

// ------------------------------------------------------------------ prefix scans (select.hpp)
// image_excl_scan_kernel: per image, poff = exclusive scan of pcnt over its h w locations, ncand = the total.

// The location-ordered list (i, j, c) -> the reference's order (c, i, j): a stable partition by channel. Workgroup
// (c, img) counts, then (second kernel) places, the entries of channel c in list order.
__global__ __launch_bounds__(kScanThreads) void d2_chan_count_kernel(const D2Cand* __restrict__ list, int cap,
                                                                      const int* __restrict__ ncand, uint32_t hw,
                                                                      int* __restrict__ ccnt) {
    __shared__ int sh[4];
    const int c = blockIdx.x, img = blockIdx.y;
    const int N = min(ncand[img], cap);
    const D2Cand* L = list + (size_t)img * cap;
    int v = 0;
    for (int e = threadIdx.x; e < N; e += kScanThreads) v += (int)(L[e].key / hw) == c ? 1 : 0;
    int total;
    block_excl_scan(v, sh, total);
    if (threadIdx.x == 0) ccnt[img * kD2Dim + c] = total;
}

__global__ __launch_bounds__(kScanThreads) void d2_chan_emit_kernel(const D2Cand* __restrict__ list, int cap,
                                                                     const int* __restrict__ ncand, uint32_t hw,
                                                                     const int* __restrict__ ccnt,
                                                                     D2Cand* __restrict__ out) {
    __shared__ int sh[4];
    const int c = blockIdx.x, img = blockIdx.y;
    const int N = min(ncand[img], cap);
    if (ccnt[img * kD2Dim + c] == 0) return;
    int v = 0;
    for (int k = threadIdx.x; k < c; k += kScanThreads) v += ccnt[img * kD2Dim + k];
    int off;
    block_excl_scan(v, sh, off);
    const D2Cand* L = list + (size_t)img * cap;
    D2Cand* O = out + (size_t)img * cap;
    for (int base = 0; base < N; base += kScanThreads) {
        const int e = base + threadIdx.x;
        D2Cand cd{};
        int f = 0;
        if (e < N) {
            cd = L[e];
            f = (int)(cd.key / hw) == c ? 1 : 0;
        }
        int total;
        const int ex = block_excl_scan(f, sh, total);
        if (f) O[off + ex] = cd;
        off += total;
    }
}

// ------------------------------------------------------------------ top-k: select, then order
// d2net.py:77 np.argsort(-scores)[:k]. Select: select.hpp's exact radix select on the score bits (scores are > 0, so
// the bits are monotone); the candidates above the k-th score and the first of those equal to it, in candidate
// order, are kept in candidate order.
__global__ __launch_bounds__(kScanThreads) void d2_select_kernel(const D2Cand* __restrict__ list, int cap,
                                                                  const int* __restrict__ ncand, int k,
                                                                  D2Cand* __restrict__ sel, int* __restrict__ out_count) {
    __shared__ int histo[256];
    __shared__ int sh[4];
    __shared__ int pick[2];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int N = min(ncand[img], cap);
    const D2Cand* L = list + (size_t)img * cap;
    const auto score_at = [&](int i) { return L[i].score; };
    const TopkCut cut = topk_cut(N, k, histo, pick, score_at);
    topk_emit(N, k, cut, sh, score_at, [&](int i, int o) { sel[(size_t)img * k + o] = L[i]; });
    if (tid == 0) out_count[img] = min(N, k);
}

// Order: a kept candidate's output row is the number of kept candidates that precede it: a larger score, or the same
// score earlier in the candidate list (sel is in candidate order). Writes (x, y), the score and the map position;
// rows past the count are zeroed. utils.py:77-80 with two scaling steps, pyramid.py:115-116 / d2net.py:83-87:
// ((p * 2 + 0.5) * 2 + 0.5) * fact in fp32, (x, y) = (column, row).
__global__ __launch_bounds__(kScanThreads) void d2_rank_kernel(const D2Cand* __restrict__ sel, const int* __restrict__ count,
                                                                int k, float fact_i, float fact_j,
                                                                float* __restrict__ out_xy, float* __restrict__ out_score,
                                                                float* __restrict__ kpos) {
    __shared__ float ss[kScanThreads];
    const int img = blockIdx.y, t = blockIdx.x * kScanThreads + threadIdx.x;
    const int N = count[img];
    const D2Cand* S = sel + (size_t)img * k;
    D2Cand me{};
    if (t < N) me = S[t];
    int rank = 0;
    for (int base = 0; base < N; base += kScanThreads) {
        const int u = base + threadIdx.x;
        __syncthreads();
        ss[threadIdx.x] = u < N ? S[u].score : 0.0f;
        __syncthreads();
        const int lim = min(kScanThreads, N - base);
        for (int q = 0; q < lim; ++q) {
            const float s = ss[q];
            rank += (s > me.score || (s == me.score && base + q < t)) ? 1 : 0;
        }
    }
    if (t < N) {
        const size_t o = (size_t)img * k + rank;
        out_xy[2 * o] = ((me.pj * 2.0f + 0.5f) * 2.0f + 0.5f) * fact_j;
        out_xy[2 * o + 1] = ((me.pi * 2.0f + 0.5f) * 2.0f + 0.5f) * fact_i;
        out_score[o] = me.score;
        kpos[2 * o] = me.pi;
        kpos[2 * o + 1] = me.pj;
    } else if (t < k) {
        const size_t o = (size_t)img * k + t;
        out_xy[2 * o] = out_xy[2 * o + 1] = 0.0f;
        out_score[o] = 0.0f;
    }
}

// ------------------------------------------------------------------ descriptors (utils.py:149-164, pyramid.py:112)
// Bilinear weights (1-a)(1-b), (1-a) b, a (1-b), a b on the corners floor/floor, floor/ceil, ceil/floor, ceil/ceil,
// summed in that order, then x / max(||x||, 1e-12). One wave per keypoint, 8 channels per lane.
__global__ __launch_bounds__(64) void d2_describe_kernel(const float* __restrict__ Fall, int h, int w,
                                                         const float* __restrict__ kpos, const int* __restrict__ count,
                                                         int k, float* __restrict__ out) {
    const int img = blockIdx.y, t = blockIdx.x, lane = threadIdx.x;
    f32x4* o = (f32x4*)(out + ((size_t)img * k + t) * kD2Dim) + 2 * lane;
    if (t >= count[img]) {
        o[0] = o[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    const float pi = kpos[((size_t)img * k + t) * 2], pj = kpos[((size_t)img * k + t) * 2 + 1];
    const float fi = floorf(pi), fj = floorf(pj);
    const int i0 = (int)fi, j0 = (int)fj, i1 = (int)ceilf(pi), j1 = (int)ceilf(pj);
    const float a = pi - fi, b = pj - fj;
    const float wtl = (1.0f - a) * (1.0f - b), wtr = (1.0f - a) * b, wbl = a * (1.0f - b), wbr = a * b;
    const float* F = Fall + (size_t)img * h * w * kD2Dim;
    auto corner = [&](int y, int x, int half) { return *((const f32x4*)(F + ((size_t)y * w + x) * kD2Dim) + 2 * lane + half); };
    f32x4 r[2];
    float ssq = 0.0f;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const f32x4 tl = corner(i0, j0, half), tr = corner(i0, j1, half), bl = corner(i1, j0, half),
                    br = corner(i1, j1, half);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[half][e] = ((wtl * tl[e] + wtr * tr[e]) + wbl * bl[e]) + wbr * br[e];
            ssq = __builtin_fmaf(r[half][e], r[half][e], ssq);
        }
    }
    const float nrm = fmaxf(__builtin_sqrtf(wave_sum(ssq)), 1e-12f);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        f32x4 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = r[half][e] / nrm;
        o[half] = q;
    }
}

// ------------------------------------------------------------------ workspace
struct D2Dims {
    int H2, W2, H4, W4, h, w;
};
D2Dims d2_dims(int H, int W) {
    D2Dims d;
    d.H2 = H / 2; d.W2 = W / 2;
    d.H4 = d.H2 / 2; d.W4 = d.W2 / 2;
    d.h = d.H4 - 1; d.w = d.W4 - 1;
    return d;
}

struct D2Layout {
    size_t actA, actB, w3, pcnt, poff, ncand, ccnt, list1, list2, sel, kpos, total;
    int cap;  // candidates held per image: one per location
};
D2Layout d2_layout(int n, int H, int W, int k, const D2Dims& d) {
    D2Layout L;
    WsCarver c;
    const size_t px = (size_t)H * W, p2 = (size_t)d.H2 * d.W2, p4 = (size_t)d.H4 * d.W4, hw = (size_t)d.h * d.w;
    // ping-pong: A holds the outputs of convs 1, 3, 5, 7, 8 (dilated 1) and 10 (F); B those of 2, 4, 6, the
    // average pool and conv 9
    const size_t fa = std::max(std::max(px * 64, p2 * 128), std::max(p4 * 256, hw * 512));
    const size_t fb = std::max(std::max(p2 * 64, p4 * 128), std::max(p4 * 256, hw * 512));
    L.cap = (int)hw;
    L.actA = c.take((size_t)n * fa * 4);
    L.actB = c.take((size_t)n * fb * 4);
    L.w3 = c.take(d2_w3_offset(kD2Convs) * sizeof(__bf16));
    L.pcnt = c.take((size_t)n * hw * 4);
    L.poff = c.take((size_t)n * hw * 4);
    L.ncand = c.take((size_t)n * 4);
    L.ccnt = c.take((size_t)n * kD2Dim * 4);
    L.list1 = c.take((size_t)n * L.cap * sizeof(D2Cand));
    L.list2 = c.take((size_t)n * L.cap * sizeof(D2Cand));
    L.sel = c.take((size_t)n * k * sizeof(D2Cand));
    L.kpos = c.take((size_t)n * k * 2 * 4);
    L.total = c.o;
    return L;
}

bool d2_shape_ok(int n, int H, int W, int k) {
    if (n <= 0 || H < 12 || W < 12 || k <= 0) return false;
    const D2Dims d = d2_dims(H, W);
    // the candidate key (c h + i) w + j and the per-image location count are 32-bit
    return (size_t)kD2Dim * d.h * d.w < ((size_t)1 << 32) && (size_t)n * H * W < ((size_t)1 << 40);
}

// conv layer l of the blob (3x3, ReLU), NHWC activations of exactly its channel counts
template <bool POOL, int DIL>
hipError_t d2_conv(int n, const float* in, int Hi, int Wi, const float* blob, const __bf16* w3, int l, float* out,
                   hipStream_t stream) {
    return conv3_launch<3, POOL, DIL>(n, in, Hi, Wi, kD2[l].cin, 0, kD2[l].cin, blob + d2_conv_offset(l), kD2[l].cout,
                                      w3 + d2_w3_offset(l), out, kD2[l].cout, 0, kD2[l].cout, 1, stream);
}

}  // namespace

extern "C" {

size_t gtsfm_d2net_weights_floats(void) { return d2_conv_offset(kD2Convs); }

size_t gtsfm_d2net_workspace_bytes(int n_img, int H, int W, int max_keypoints) {
    if (!d2_shape_ok(n_img, H, W, max_keypoints)) return 0;
    return d2_layout(n_img, H, W, max_keypoints, d2_dims(H, W)).total;
}

int gtsfm_d2net_stages(const uint8_t* d_images, int n, int H, int W, int C, const float* d_weights, int max_keypoints,
                       float fact_i, float fact_j, void* d_workspace, size_t workspace_bytes, float* d_xy,
                       float* d_score, float* d_desc, int* d_count, int* d_n_candidates, float* d_dense_map,
                       int last_stage, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n == 0) return GTSFM_OK;
    if (!d_images || !d_weights || !d_workspace || !d_xy || !d_score || !d_desc || !d_count || (C != 1 && C != 3) ||
        last_stage < GTSFM_D2NET_STAGE_TRUNK || last_stage > GTSFM_D2NET_STAGE_DESCRIBE ||
        !d2_shape_ok(n, H, W, max_keypoints))
        return GTSFM_ERR_ARG;
    const D2Dims d = d2_dims(H, W);
    const int k = max_keypoints;
    const D2Layout L = d2_layout(n, H, W, k, d);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    float* A = (float*)(ws + L.actA);
    float* B = (float*)(ws + L.actB);
    __bf16* w3 = (__bf16*)(ws + L.w3);
    const float* blob = d_weights;
    // ---- trunk (model_test.py:17-33)
    {
        Conv3SplitJob jobs[kD2Convs - 1];
        for (int l = 1; l < kD2Convs; ++l)
            jobs[l - 1] = {blob + d2_conv_offset(l), w3 + d2_w3_offset(l), 9, kD2[l].cin, kD2[l].cout};
        GTSFM_CHECK_HIP(conv3_split_weights(jobs, kD2Convs - 1, stream));
    }
    GTSFM_CHECK_HIP(rgb_conv1_launch(d_images, n, H, W, C, blob + d2_conv_offset(0), D2Pre{}, A, stream));
    GTSFM_CHECK_HIP((d2_conv<true, 1>(n, A, H, W, blob, w3, 1, B, stream)));
    GTSFM_CHECK_HIP((d2_conv<false, 1>(n, B, d.H2, d.W2, blob, w3, 2, A, stream)));
    GTSFM_CHECK_HIP((d2_conv<true, 1>(n, A, d.H2, d.W2, blob, w3, 3, B, stream)));
    GTSFM_CHECK_HIP((d2_conv<false, 1>(n, B, d.H4, d.W4, blob, w3, 4, A, stream)));
    GTSFM_CHECK_HIP((d2_conv<false, 1>(n, A, d.H4, d.W4, blob, w3, 5, B, stream)));
    GTSFM_CHECK_HIP((d2_conv<false, 1>(n, B, d.H4, d.W4, blob, w3, 6, A, stream)));
    hipLaunchKernelGGL(d2_avgpool_kernel, dim3(blocks_for((size_t)n * d.h * d.w * 64, 256)), dim3(256), 0, stream,
                       (const float*)A, n, d.H4, d.W4, B);
    GTSFM_CHECK_HIP(hipGetLastError());
    if (last_stage == GTSFM_D2NET_STAGE_TRUNK) return GTSFM_OK;
    // ---- conv4_1..3, dilation 2 (model_test.py:34-38), ReLU after the last too (:56-57)
    GTSFM_CHECK_HIP((d2_conv<false, 2>(n, B, d.h, d.w, blob, w3, 7, A, stream)));
    GTSFM_CHECK_HIP((d2_conv<false, 2>(n, A, d.h, d.w, blob, w3, 8, B, stream)));
    GTSFM_CHECK_HIP((d2_conv<false, 2>(n, B, d.h, d.w, blob, w3, 9, A, stream)));
    const float* F = A;
    const size_t hw = (size_t)d.h * d.w;
    if (d_dense_map)
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_dense_map, F, (size_t)n * hw * kD2Dim * 4, hipMemcpyDeviceToDevice, stream));
    if (last_stage == GTSFM_D2NET_STAGE_DILATED) return GTSFM_OK;
    // ---- detection, candidate list, top-k
    int* pcnt = (int*)(ws + L.pcnt);
    int* poff = (int*)(ws + L.poff);
    int* ncand = (int*)(ws + L.ncand);
    int* ccnt = (int*)(ws + L.ccnt);
    D2Cand* list1 = (D2Cand*)(ws + L.list1);
    D2Cand* list2 = (D2Cand*)(ws + L.list2);
    D2Cand* sel = (D2Cand*)(ws + L.sel);
    float* kpos = (float*)(ws + L.kpos);
    const dim3 dgrid(blocks_for((size_t)n * hw, 4));
    hipLaunchKernelGGL((d2_detect_kernel<false>), dgrid, dim3(256), 0, stream, F, n, d.h, d.w, pcnt, (const int*)nullptr,
                       L.cap, (D2Cand*)nullptr);
    hipLaunchKernelGGL(image_excl_scan_kernel, dim3(n), dim3(kScanThreads), 0, stream, (const int*)pcnt, (int)hw, poff, ncand);
    hipLaunchKernelGGL((d2_detect_kernel<true>), dgrid, dim3(256), 0, stream, F, n, d.h, d.w, (int*)nullptr,
                       (const int*)poff, L.cap, list1);
    hipLaunchKernelGGL(d2_chan_count_kernel, dim3(kD2Dim, n), dim3(kScanThreads), 0, stream, (const D2Cand*)list1, L.cap,
                       (const int*)ncand, (uint32_t)hw, ccnt);
    hipLaunchKernelGGL(d2_chan_emit_kernel, dim3(kD2Dim, n), dim3(kScanThreads), 0, stream, (const D2Cand*)list1, L.cap,
                       (const int*)ncand, (uint32_t)hw, (const int*)ccnt, list2);
    hipLaunchKernelGGL(d2_select_kernel, dim3(n), dim3(kScanThreads), 0, stream, (const D2Cand*)list2, L.cap,
                       (const int*)ncand, k, sel, d_count);
    hipLaunchKernelGGL(d2_rank_kernel, dim3(blocks_for(k, kScanThreads), n), dim3(kScanThreads), 0, stream,
                       (const D2Cand*)sel, (const int*)d_count, k, fact_i, fact_j, d_xy, d_score, kpos);
    GTSFM_CHECK_HIP(hipGetLastError());
    if (d_n_candidates)
        GTSFM_CHECK_HIP(hipMemcpyAsync(d_n_candidates, ncand, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, stream));
    if (last_stage == GTSFM_D2NET_STAGE_DETECT) return GTSFM_OK;
    // ---- descriptors
    hipLaunchKernelGGL(d2_describe_kernel, dim3(k, n), dim3(64), 0, stream, F, d.h, d.w, (const float*)kpos,
                       (const int*)d_count, k, d_desc);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

int gtsfm_d2net_batched(const uint8_t* d_images, int n, int H, int W, int C, const float* d_weights, int max_keypoints,
                        float fact_i, float fact_j, void* d_workspace, size_t workspace_bytes, float* d_xy,
                        float* d_score, float* d_desc, int* d_count, int* d_n_candidates, float* d_dense_map,
                        void* stream) {
    return gtsfm_d2net_stages(d_images, n, H, W, C, d_weights, max_keypoints, fact_i, fact_j, d_workspace,
                              workspace_bytes, d_xy, d_score, d_desc, d_count, d_n_candidates, d_dense_map,
                              GTSFM_D2NET_STAGE_DESCRIBE, stream);
}

}  // extern "C"
