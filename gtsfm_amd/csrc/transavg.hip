// Translation averaging, 1DSfM: world-frame direction measurements and track selection, the MFAS outlier filter over
// many projection directions, and the recovery of camera and landmark positions by Levenberg-Marquardt.
//
// Reference: gtsfm/averaging/translation/averaging_1dsfm.py (get_valid_measurements_in_world_frame :593-616,
// _select_tracks_for_averaging :273-339, _get_landmark_directions :341-372, compute_inliers :194-256,
// __run_averaging :374-430) on GTSAM's MFAS and TranslationRecovery. The semantics are stated in include/gtsfm_hip.h.
//
// MFAS is the hot path: the reference runs its 2000 greedy orderings one after another in Python. Here one 256-lane
// workgroup owns one projection direction; inSum, outSum and the removal position of every node live in LDS (20 bytes
// per node), the graph is a node-major list of incident measurements built once per call by a stable counting sort
// (csr.hpp), and an edge's weight is recomputed from its 24-byte direction wherever it is needed. The ordering is the
// sequential one of the contract, one removal per step: a parallel search for the lowest source, else for the best
// heuristic, then the removed node's incident edges in parallel (every neighbour is touched by one lane; a node with
// two edges to the same neighbour is flagged at build time and updated by one lane in list order). The step count is
// the node count by construction. The violated edges of a direction are kept as one bit each; one pass per edge then
// adds the weights of its set bits in ascending direction order. The recovery shares gba.hip's LM schedule (lm.hpp),
// Huber treatment (se3.hpp) and fixed-order reductions (reduce.hpp); its matrix-free PCG has 3 x 3 blocks and no
// elimination.
// fp64, no FMA contraction, no floating-point atomics: two calls return the same bytes.
#include <limits.h>
#include <math.h>

#include "twoview.hpp"  // sm_mix

#pragma clang fp contract(off)

#include "csr.hpp"
#include "lm.hpp"
#include "reduce.hpp"
#include "se3.hpp"  // mv3, inv3, Huber

namespace {

constexpr int kMinTrackMeas = 3;  // MIN_TRACK_MEASUREMENTS_FOR_AVERAGING
constexpr int kSelBlock = 1024;
constexpr int kMfasBlock = 256;
constexpr int kVecBlock = 1024;
constexpr int kNodeBlock = 256;  // 4 nodes per workgroup, one wave each
constexpr int kChunksMax = 256;
constexpr double kSourceEps = 1e-8;
constexpr double kIsig = 100.0;    // 1 / NOISE_MODEL_SIGMA
constexpr double kPriorW = 1.0e4;  // 1 / 0.01^2
constexpr int kLin = 12;  // doubles per factor: A[9], b[3]

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Unit3(p): p / |p|, a zero vector stays zero
__device__ __forceinline__ void unit3(const double* p, double* o) {
    const double n2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (n2 > 0.0) {
        const double n = sqrt(n2);
        o[0] = p[0] / n; o[1] = p[1] / n; o[2] = p[2] / n;
    } else {
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
    }
}

// ------------------------------------------------------------------ node-major incidence lists (stable counting sort)
// csr.hpp source: every used measurement is listed at both of its nodes
struct CsrArgs {
    static constexpr int kKeys = 2;
    const int* key;      // [E][2]
    const uint8_t* use;  // [E]
    int E, n;
    int* node_off;  // [n + 1]
    int* inc;       // [2 E]
    int* hist;      // [chunks][n]
    uint8_t* dup;   // [n] or NULL
    CsrChunks chunks;
    __device__ bool keys(long long m, int* k) const {
        if (!use[m]) return false;
        k[0] = key[2 * m];
        k[1] = key[2 * m + 1];
        return true;
    }
    __device__ void put(long long m, const int*, const size_t* slot) const {
        inc[slot[0]] = (int)m;
        inc[slot[1]] = (int)m;
    }
};

// dup[v] = 1 when two of v's incident measurements lead to the same neighbour
__global__ void ta_csr_dup(CsrArgs a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n) return;
    uint8_t d = 0;
    const int b = a.node_off[v], e = a.node_off[v + 1];
    for (int k = b + 1; k < e && !d; ++k) {
        const int m = a.inc[k];
        const int o = a.key[2 * m] == v ? a.key[2 * m + 1] : a.key[2 * m];
        for (int l = b; l < k; ++l) {
            const int m2 = a.inc[l];
            const int o2 = a.key[2 * m2] == v ? a.key[2 * m2 + 1] : a.key[2 * m2];
            if (o2 == o) { d = 1; break; }
        }
    }
    a.dup[v] = d;
}

int ta_csr_build(const CsrArgs& a, hipStream_t stream) {
    const int rc = csr_build(a, a.E, a.n, a.chunks, a.hist, a.node_off, stream);
    if (rc != GTSFM_OK) return rc;
    if (a.dup) hipLaunchKernelGGL(ta_csr_dup, dim3(blocks_for(a.n, 256)), dim3(256), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

// ------------------------------------------------------------------ (a), (b): measurements and track selection
struct MeasArgs {
    const int* edges;
    const double* i2Ui1;
    const uint8_t* evalid;
    int n_edges;
    const double* wRi;
    const uint8_t* rvalid;
    int n_img;
    const int* off;
    const int* img;
    const void* uv;
    int uv64;
    int T, M;
    const long long* d_nt;
    const double* intr;
    int per_cam;
    int* key;
    double* dir;
    uint8_t* mvalid;
    int* selected;
    uint8_t* cam_valid;
    long long* counts;
    int* imp;        // [T]
    int* remaining;  // [n_img]
    int* mtrack;     // [M]
    int* sel_off;    // [T]
};

__device__ __forceinline__ int ta_tracks_eff(const MeasArgs& a) {
    if (!a.d_nt) return a.T;
    const long long n = a.d_nt[0];
    return n < 0 ? 0 : (n < (long long)a.T ? (int)n : a.T);
}

__global__ void ta_meas_init(MeasArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4) a.counts[i] = 0;
    if (i < (size_t)a.n_img) {
        a.cam_valid[i] = 0;
        a.remaining[i] = a.per_cam;
    }
    if (i < (size_t)a.n_edges + (size_t)a.M) {
        a.mvalid[i] = 0;
        a.key[2 * i] = a.key[2 * i + 1] = -1;
        a.dir[3 * i] = a.dir[3 * i + 1] = a.dir[3 * i + 2] = 0.0;
    }
    if (i < (size_t)a.T) {
        a.selected[i] = -1;
        a.imp[i] = 0;
        a.sel_off[i] = 0;
    }
    if (i < (size_t)a.M) a.mtrack[i] = -1;
}

__global__ void ta_cam_edges(MeasArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.n_edges) return;
    const int i1 = a.edges[2 * e], i2 = a.edges[2 * e + 1];
    if (a.evalid && a.evalid[e] == 0) return;
    if (i1 < 0 || i1 >= a.n_img || i2 < 0 || i2 >= a.n_img || i1 == i2) return;
    if (a.rvalid && a.rvalid[i2] == 0) return;
    double w[3], u[3];
    mv3(a.wRi + 9 * (size_t)i2, a.i2Ui1 + 3 * (size_t)e, w);
    unit3(w, u);
    a.key[2 * e] = i2;
    a.key[2 * e + 1] = i1;
    for (int k = 0; k < 3; ++k) a.dir[3 * (size_t)e + k] = u[k];
    a.mvalid[e] = 1;
    a.cam_valid[i1] = 1;
    a.cam_valid[i2] = 1;
    atomicAdd((unsigned long long*)&a.counts[0], 1ull);
}

__global__ void ta_track_filter(MeasArgs a) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ta_tracks_eff(a)) return;
    const int b = a.off[t], e = a.off[t + 1];
    if (b < 0 || e < b || e > a.M) return;
    int cnt = 0;
    for (int m = b; m < e; ++m) {
        const int c = a.img[m];
        cnt += c >= 0 && c < a.n_img && a.cam_valid[c];
    }
    if (cnt < kMinTrackMeas) return;
    a.imp[t] = cnt;
    for (int m = b; m < e; ++m) {
        const int c = a.img[m];
        if (c >= 0 && c < a.n_img && a.cam_valid[c]) a.mtrack[m] = t;
    }
}

// The greedy loop of _select_tracks_for_averaging: one workgroup, a parallel first-maximum and a parallel update per
// step. imp[] is read and written through agent-scope atomics only, so the lanes agree on it across the barriers.
__global__ __launch_bounds__(kSelBlock) void ta_select(MeasArgs a) {
    __shared__ int s_val[16], s_idx[16];
    __shared__ int s_hit, s_cam;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = ta_tracks_eff(a);
    int ns = 0, run = 0;
    for (int step = 0; step < T; ++step) {
        int bv = -1, bi = INT_MAX;
        for (int t = threadIdx.x; t < T; t += kSelBlock) {
            const int v = ld_int(a.imp + t);
            if (v > bv) { bv = v; bi = t; }
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const int ov = __shfl_xor(bv, o), oi = __shfl_xor(bi, o);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { s_val[wave] = bv; s_idx[wave] = bi; }
        __syncthreads();
        bv = s_val[0]; bi = s_idx[0];
        for (int w = 1; w < kSelBlock / 64; ++w)
            if (s_val[w] > bv || (s_val[w] == bv && s_idx[w] < bi)) { bv = s_val[w]; bi = s_idx[w]; }
        __syncthreads();
        if (bv <= 0) break;
        if (threadIdx.x == 0) {
            a.selected[ns] = bi;
            a.sel_off[ns] = run;
            st_int(a.imp + bi, 0);
        }
        const int b = a.off[bi], e = a.off[bi + 1];
        for (int m = b; m < e; ++m) {
            if (a.mtrack[m] != bi) continue;
            ++run;
            if (threadIdx.x == 0) {
                const int c = a.img[m], r = a.remaining[c];
                if (r > 0) a.remaining[c] = r - 1;
                s_hit = r == 1;
                s_cam = c;
            }
            __syncthreads();
            if (s_hit) {
                // the camera just got covered: one decrement, clamped at zero, per measurement that any track has in it
                const int c = s_cam;
                for (int m2 = threadIdx.x; m2 < a.M; m2 += kSelBlock) {
                    const int t2 = a.mtrack[m2];
                    if (t2 < 0 || a.img[m2] != c) continue;
                    if (atomicSub(a.imp + t2, 1) <= 0) atomicAdd(a.imp + t2, 1);
                }
            }
            __syncthreads();
        }
        ++ns;
    }
    if (threadIdx.x == 0) {
        a.counts[2] = ns;
        a.counts[1] = run;
    }
}

__global__ void ta_track_dirs(MeasArgs a) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.T || (long long)s >= a.counts[2]) return;
    const int t = a.selected[s];
    size_t slot = (size_t)a.n_edges + (size_t)a.sel_off[s];
    for (int m = a.off[t]; m < a.off[t + 1]; ++m) {
        if (a.mtrack[m] != t) continue;
        const int c = a.img[m];
        if (a.rvalid && a.rvalid[c] == 0) {
            // the reference raises here ("rotation cannot be None for input track measurements"): counted, slot unused
            atomicAdd((unsigned long long*)&a.counts[3], 1ull);
            ++slot;
            continue;
        }
        double uv[2];
        if (a.uv64) {
            uv[0] = ((const double*)a.uv)[2 * (size_t)m];
            uv[1] = ((const double*)a.uv)[2 * (size_t)m + 1];
        } else {
            uv[0] = ((const float*)a.uv)[2 * (size_t)m];
            uv[1] = ((const float*)a.uv)[2 * (size_t)m + 1];
        }
        const double* K = a.intr + 3 * (size_t)c;
        const double h[3] = {(uv[0] - K[1]) / K[0], (uv[1] - K[2]) / K[0], 1.0};
        double hu[3], w[3], u[3];
        unit3(h, hu);
        mv3(a.wRi + 9 * (size_t)c, hu, w);
        unit3(w, u);
        a.key[2 * slot] = c;
        a.key[2 * slot + 1] = a.n_img + s;
        for (int k = 0; k < 3; ++k) a.dir[3 * slot + k] = u[k];
        a.mvalid[slot] = 1;
        ++slot;
    }
}

struct MeasLayout { size_t imp, remaining, mtrack, sel_off, total; };

MeasLayout meas_layout(long long T, long long M, int C) {
    MeasLayout L;
    WsCarver w;
    L.imp = w.take((size_t)T * 4);
    L.remaining = w.take((size_t)C * 4);
    L.mtrack = w.take((size_t)M * 4);
    L.sel_off = w.take((size_t)T * 4);
    L.total = w.o;
    return L;
}

// ------------------------------------------------------------------ (c): MFAS
struct MfasArgs {
    const int* key;
    const double* dir;
    const uint8_t* use;
    int E, n, n_dir, words;
    const double* proj;
    const int* node_off;
    const int* inc;
    const uint8_t* dup;
    uint32_t* viol;  // [n_dir][words]
    double thr;
    const uint8_t* mvalid;
    double* osum;
    uint8_t* inlier;
};

__global__ void ta_mfas_use(const int* key, const uint8_t* mvalid, int E, int n, uint8_t* use) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int k1 = key[2 * e], k2 = key[2 * e + 1];
    use[e] = (!mvalid || mvalid[e]) && k1 >= 0 && k1 < n && k2 >= 0 && k2 < n && k1 != k2;
}

__global__ __launch_bounds__(kMfasBlock) void ta_mfas(MfasArgs a) {
    extern __shared__ double lds[];
    __shared__ int s_i[kMfasBlock / 64];
    __shared__ double s_d[kMfasBlock / 64];
    __shared__ int s_j[kMfasBlock / 64];
    const int n = a.n;
    double* inS = lds;
    double* outS = lds + n;
    int* pos = (int*)(lds + 2 * (size_t)n);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double d[3] = {a.proj[3 * (size_t)blockIdx.x], a.proj[3 * (size_t)blockIdx.x + 1],
                         a.proj[3 * (size_t)blockIdx.x + 2]};
    // initial sums, ascending measurement index per node
    for (int v = threadIdx.x; v < n; v += kMfasBlock) {
        double si = 0.0, so = 0.0;
        for (int k = a.node_off[v]; k < a.node_off[v + 1]; ++k) {
            const int e = a.inc[k];
            const double w = dot3(a.dir + 3 * (size_t)e, d);
            const int src = w >= 0.0 ? a.key[2 * e] : a.key[2 * e + 1];
            if (src == v) so += fabs(w);
            else si += fabs(w);
        }
        inS[v] = si;
        outS[v] = so;
        pos[v] = -1;
    }
    __syncthreads();
    for (int step = 0; step < n; ++step) {  // one removal per step
        int pick = INT_MAX;
        for (int v = threadIdx.x; v < n; v += kMfasBlock)
            if (pos[v] < 0 && inS[v] < kSourceEps) { pick = v; break; }
        for (int o = 32; o >= 1; o >>= 1) {
            const int p2 = __shfl_xor(pick, o);
            pick = p2 < pick ? p2 : pick;
        }
        if (lane == 0) s_i[wave] = pick;
        __syncthreads();
        pick = s_i[0];
        for (int w = 1; w < kMfasBlock / 64; ++w) pick = s_i[w] < pick ? s_i[w] : pick;
        if (pick == INT_MAX) {  // no source: the largest (outSum + 1) / (inSum + 1), lowest index on ties
            double bv = -1.0;
            int bi = INT_MAX;
            for (int v = threadIdx.x; v < n; v += kMfasBlock)
                if (pos[v] < 0) {
                    const double r = (outS[v] + 1.0) / (inS[v] + 1.0);
                    if (r > bv || bi == INT_MAX) { bv = r; bi = v; }
                }
            for (int o = 32; o >= 1; o >>= 1) {
                const double ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (oi != INT_MAX && (bi == INT_MAX || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
            }
            if (lane == 0) { s_d[wave] = bv; s_j[wave] = bi; }
            __syncthreads();
            bv = s_d[0]; bi = s_j[0];
            for (int w = 1; w < kMfasBlock / 64; ++w)
                if (s_j[w] != INT_MAX && (bi == INT_MAX || s_d[w] > bv || (s_d[w] == bv && s_j[w] < bi))) {
                    bv = s_d[w]; bi = s_j[w];
                }
            pick = bi;
        }
        if (pick == INT_MAX) break;  // cannot happen: step < n leaves a node
        if (threadIdx.x == 0) pos[pick] = step;
        const int b = a.node_off[pick], e = a.node_off[pick + 1];
        const bool serial = a.dup[pick] != 0;
        const int k0 = serial ? (threadIdx.x == 0 ? b : e) : b + (int)threadIdx.x;
        const int kstep = serial ? 1 : kMfasBlock;
        for (int k = k0; k < e; k += kstep) {
            const int m = a.inc[k];
            const int k1 = a.key[2 * m], k2 = a.key[2 * m + 1];
            const int other = k1 == pick ? k2 : k1;
            if (pos[other] >= 0) continue;
            const double w = dot3(a.dir + 3 * (size_t)m, d);
            const int src = w >= 0.0 ? k1 : k2;
            if (src == pick) inS[other] -= fabs(w);
            else outS[other] -= fabs(w);
        }
        __syncthreads();
    }
    // an edge is violated when its sink was removed before its source
    uint32_t* vw = a.viol + (size_t)blockIdx.x * a.words;
    for (int wi = threadIdx.x; wi < a.words; wi += kMfasBlock) {
        uint32_t bits = 0;
        for (int j = 0; j < 32; ++j) {
            const int e = 32 * wi + j;
            if (e >= a.E || !a.use[e]) continue;
            const double w = dot3(a.dir + 3 * (size_t)e, d);
            const int k1 = a.key[2 * e], k2 = a.key[2 * e + 1];
            const int src = w >= 0.0 ? k1 : k2, dst = w >= 0.0 ? k2 : k1;
            if (pos[dst] < pos[src]) bits |= 1u << j;
        }
        vw[wi] = bits;
    }
}

__global__ void ta_mfas_sum(MfasArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E) return;
    double s = 0.0;
    if (a.use[e]) {
        const double u[3] = {a.dir[3 * (size_t)e], a.dir[3 * (size_t)e + 1], a.dir[3 * (size_t)e + 2]};
        const uint32_t bit = 1u << (e & 31);
        for (int di = 0; di < a.n_dir; ++di)
            if (a.viol[(size_t)di * a.words + (e >> 5)] & bit) s += fabs(dot3(u, a.proj + 3 * (size_t)di));
    }
    a.osum[e] = s;
    a.inlier[e] = a.use[e] && s / (double)a.n_dir < a.thr;
}

struct MfasLayout { size_t use, node_off, inc, hist, dup, viol, total; CsrChunks chunks; int words; };

MfasLayout mfas_layout(long long E, int n, int n_dir) {
    MfasLayout L;
    L.chunks = csr_chunks(E, kChunksMax);
    L.words = (int)((E + 31) / 32);
    WsCarver w;
    L.use = w.take((size_t)E);
    L.node_off = w.take(((size_t)n + 1) * 4);
    L.inc = w.take((size_t)E * 8);
    L.hist = w.take(csr_hist_bytes(L.chunks, n));
    L.dup = w.take((size_t)n);
    L.viol = w.take((size_t)n_dir * L.words * 4);
    L.total = w.o;
    return L;
}

bool mfas_sizes_ok(long long E, int n, int n_dir) {
    return E > 0 && E < (1ll << 30) && n > 0 && n <= GTSFM_TRANSAVG_MFAS_MAX_NODES && n_dir > 0 && n_dir <= (1 << 20);
}

// ------------------------------------------------------------------ (d): recovery
enum { S_RR = 0, S_RZ = 1, S_BB = 2, S_OLDLIN = 3, S_NEWLIN = 4, S_NEWERR = 5, S_COUNT = 8 };
enum { I_E0 = 0, I_NFAC = 1, I_NACT = 2, I_BAD = 3, I_NKEPT = 4, I_COUNT = 8 };

struct RecArgs {
    const int* key;
    const double* dir;
    const uint8_t* inl;
    int E, n_img, n_land, n;
    const uint8_t* rvalid;
    int robust;
    double scale;
    uint64_t seed;
    uint8_t* cam_inl;  // [n_img]
    uint8_t* isvar;    // [n]
    uint8_t* active;   // [n]
    int* rep;          // [n]
    int* rkey;         // [E + 1][2]; slot E is the scale factor
    uint8_t* ruse;     // [E + 1]
    int* icnt;
    double* XA;  // [n][3]
    double* XB;
    double* lin;   // [E + 1][kLin]
    double* D;     // [n][9]
    double* g;     // [n][3]
    double* Minv;  // [n][9]
    double* ye;    // [E + 1][3]
    double* te;    // [E + 1]
    double* tl;    // [E + 1]
    double* x;     // [3 n] each
    double* r;
    double* z;
    double* p;
    double* q;
    double* scal;
    const int* node_off;
    const int* inc;
};

__global__ void rec_init(RecArgs a) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        for (int k = 0; k < I_COUNT; ++k) a.icnt[k] = 0;
        a.icnt[I_E0] = INT_MAX;
        for (int k = 0; k < S_COUNT; ++k) a.scal[k] = 0.0;
    }
    if (i < (size_t)a.n_img) a.cam_inl[i] = 0;
    if (i < (size_t)a.n) {
        a.isvar[i] = 0;
        a.active[i] = 0;
        a.rep[i] = (int)i;
    }
    if (i <= (size_t)a.E) {
        a.ruse[i] = 0;
        a.rkey[2 * i] = a.rkey[2 * i + 1] = 0;
        a.te[i] = 0.0;
        a.tl[i] = 0.0;
    }
}

__device__ __forceinline__ bool rec_keys_ok(const RecArgs& a, int e, int& k1, int& k2) {
    k1 = a.key[2 * e];
    k2 = a.key[2 * e + 1];
    return a.inl[e] != 0 && k1 >= 0 && k1 < a.n_img && k2 >= 0 && k2 < a.n && k1 != k2;
}

__global__ void rec_caminl(RecArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int k1, k2;
    if (e >= a.E || !rec_keys_ok(a, e, k1, k2) || k2 >= a.n_img) return;
    a.cam_inl[k1] = 1;
    a.cam_inl[k2] = 1;
}

__global__ void rec_keep(RecArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int k1, k2;
    if (e >= a.E || !rec_keys_ok(a, e, k1, k2)) return;
    if (k2 >= a.n_img && !a.cam_inl[k1]) return;  // a track measurement needs an inlier camera edge at its camera
    a.ruse[e] = 1;
    a.isvar[k1] = 1;
    a.isvar[k2] = 1;
    atomicAdd(&a.icnt[I_NKEPT], 1);
}

__device__ __forceinline__ bool zero_dir(const double* u) {
    return fabs(u[0]) <= 1e-9 && fabs(u[1]) <= 1e-9 && fabs(u[2]) <= 1e-9;
}

// nodes joined by a zero direction share one position (TranslationRecovery's same-translation sets): rep[v] becomes the
// lowest index of v's set, by label propagation; at most n rounds
__global__ __launch_bounds__(kVecBlock) void rec_merge(RecArgs a) {
    __shared__ int s_changed;
    for (int round = 0; round < a.n; ++round) {
        if (threadIdx.x == 0) s_changed = 0;
        __syncthreads();
        for (int e = threadIdx.x; e < a.E; e += kVecBlock) {
            if (!a.ruse[e] || !zero_dir(a.dir + 3 * (size_t)e)) continue;
            const int k1 = a.key[2 * e], k2 = a.key[2 * e + 1];
            const int r1 = ld_int(a.rep + k1), r2 = ld_int(a.rep + k2);
            if (r1 == r2) continue;
            const int m = r1 < r2 ? r1 : r2;
            atomicMin(a.rep + (r1 < r2 ? k2 : k1), m);
            s_changed = 1;
        }
        __syncthreads();
        const int c = s_changed;
        __syncthreads();
        if (!c) break;
    }
}

__global__ void rec_factors(RecArgs a) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.E || !a.ruse[e]) return;
    const int ra = a.rep[a.key[2 * e]], rb = a.rep[a.key[2 * e + 1]];
    if (ra == rb) {
        a.ruse[e] = 0;
        return;
    }
    a.rkey[2 * e] = ra;
    a.rkey[2 * e + 1] = rb;
    a.active[ra] = 1;
    a.active[rb] = 1;
    atomicMin(&a.icnt[I_E0], e);
    atomicAdd(&a.icnt[I_NFAC], 1);
}

__global__ void rec_start(RecArgs a) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v == 0) {
        const int e0 = a.icnt[I_E0];
        if (e0 != INT_MAX) {
            a.rkey[2 * (size_t)a.E] = a.rkey[2 * e0];
            a.rkey[2 * (size_t)a.E + 1] = a.rkey[2 * e0 + 1];
            a.ruse[a.E] = 1;
        }
    }
    if (v >= a.n) return;
    for (int k = 0; k < 3; ++k) {
        double c = 0.0;
        if (a.active[v]) {
            const uint64_t h = sm_mix(sm_mix(a.seed ^ sm_mix((uint64_t)(uint32_t)v)) + (uint64_t)k);
            c = 2.0 * ((double)(h >> 11) * (1.0 / 9007199254740992.0)) - 1.0;
        }
        a.XA[3 * (size_t)v + k] = a.XB[3 * (size_t)v + k] = c;
    }
    if (a.active[v]) atomicAdd(&a.icnt[I_NACT], 1);
}

// residual r and, with J, d normalize / d (tb - ta) (the scale factor: identity) of factor e at X
__device__ __forceinline__ void rec_residual(const RecArgs& a, const double* X, int e, double* r, double* J) {
    const int ka = a.rkey[2 * (size_t)e], kb = a.rkey[2 * (size_t)e + 1];
    const double v[3] = {X[3 * (size_t)kb] - X[3 * (size_t)ka], X[3 * (size_t)kb + 1] - X[3 * (size_t)ka + 1],
                         X[3 * (size_t)kb + 2] - X[3 * (size_t)ka + 2]};
    if (e == a.E) {
        const double* u = a.dir + 3 * (size_t)a.icnt[I_E0];
        for (int k = 0; k < 3; ++k) r[k] = v[k] - a.scale * u[k];
        if (J)
            for (int k = 0; k < 9; ++k) J[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return;
    }
    const double* u = a.dir + 3 * (size_t)e;
    const double nrm = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double nh[3] = {v[0] / nrm, v[1] / nrm, v[2] / nrm};
    for (int k = 0; k < 3; ++k) r[k] = nh[k] - u[k];
    if (J)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) J[3 * i + j] = ((i == j ? 1.0 : 0.0) - nh[i] * nh[j]) / nrm;
}

__device__ __forceinline__ double rec_loss(const RecArgs& a, const double* r) {
    const double d = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) * kIsig;
    return a.robust ? huber_loss(d) : 0.5 * d * d;
}

__global__ void rec_eval(RecArgs a, const double* X) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > a.E || !a.ruse[e]) return;
    double r[3];
    rec_residual(a, X, e, r, nullptr);
    a.te[e] = rec_loss(a, r);
}

__device__ __forceinline__ int rec_prior_node(const RecArgs& a) { return a.rkey[2 * (size_t)a.E]; }

// scal[S_NEWERR] = sum te + prior(Xerr); with_lin: scal[S_NEWLIN] = 0.5 (sum tl + prior row of the step)
__global__ __launch_bounds__(kVecBlock) void rec_reduce(RecArgs a, const double* Xerr, const double* Xold, int with_lin) {
    __shared__ double sh[32];
    double v[2] = {0.0, 0.0};
    for (int e = threadIdx.x; e <= a.E; e += kVecBlock) {
        v[0] += a.te[e];
        v[1] += a.tl[e];
    }
    block_sum<2>(v, sh);
    if (threadIdx.x == 0) {
        const int p0 = rec_prior_node(a);
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s += Xerr[3 * (size_t)p0 + k] * Xerr[3 * (size_t)p0 + k];
        a.scal[S_NEWERR] = v[0] + 0.5 * s * kPriorW;
        if (with_lin) {
            double nl = v[1];
            for (int k = 0; k < 3; ++k) {
                const double dd = a.x[3 * (size_t)p0 + k] + Xold[3 * (size_t)p0 + k];
                nl += dd * dd * kPriorW;
            }
            a.scal[S_NEWLIN] = 0.5 * nl;
        } else {
            a.scal[S_OLDLIN] = 0.5 * (v[1] + s * kPriorW);
        }
    }
}

__global__ void rec_linearize(RecArgs a, const double* X) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > a.E || !a.ruse[e]) return;
    double r[3], J[9];
    rec_residual(a, X, e, r, J);
    const double ew[3] = {r[0] * kIsig, r[1] * kIsig, r[2] * kIsig};
    const double sw = a.robust ? sqrt(huber_weight(sqrt(ew[0] * ew[0] + ew[1] * ew[1] + ew[2] * ew[2]))) : 1.0;
    const double s = sw * kIsig;
    double* L = a.lin + (size_t)e * kLin;
    for (int k = 0; k < 9; ++k) L[k] = J[k] * s;
    double bb = 0.0;
    for (int k = 0; k < 3; ++k) {
        L[9 + k] = -sw * ew[k];
        bb += L[9 + k] * L[9 + k];
    }
    a.tl[e] = bb;
}

// sum of v[0..NV) over a wave, the same on every lane
template <int NV>
__device__ __forceinline__ void wave_sum(double* v) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
    }
}

// per node (one wave): D = sum A^T A (+ the prior), g = sum +-A^T b (- prior)
__global__ __launch_bounds__(kNodeBlock) void rec_node_lin(RecArgs a, const double* X) {
    const int v = blockIdx.x * (kNodeBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= a.n) return;
    double s[9];
    for (int k = 0; k < 9; ++k) s[k] = 0.0;
    if (a.active[v])
        for (int i = a.node_off[v] + lane; i < a.node_off[v + 1]; i += 64) {
            const int e = a.inc[i];
            const double* L = a.lin + (size_t)e * kLin;
            const double sg = a.rkey[2 * (size_t)e + 1] == v ? 1.0 : -1.0;
            int n = 0;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = r; c < 3; ++c, ++n) s[n] += L[r] * L[c] + L[3 + r] * L[3 + c] + L[6 + r] * L[6 + c];
                s[6 + r] += sg * (L[r] * L[9] + L[3 + r] * L[10] + L[6 + r] * L[11]);
            }
        }
    wave_sum<9>(s);
    if (lane == 0) {
        double* D = a.D + 9 * (size_t)v;
        D[0] = s[0]; D[1] = D[3] = s[1]; D[2] = D[6] = s[2]; D[4] = s[3]; D[5] = D[7] = s[4]; D[8] = s[5];
        double* g = a.g + 3 * (size_t)v;
        for (int k = 0; k < 3; ++k) g[k] = s[6 + k];
        if (a.active[v] && v == rec_prior_node(a))
            for (int k = 0; k < 3; ++k) {
                D[4 * k] += kPriorW;
                g[k] += -X[3 * (size_t)v + k] * kPriorW;
            }
    }
}

__global__ void rec_damp(RecArgs a, double lambda) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n) return;
    double Mi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (a.active[v]) {
        double H[9];
        for (int k = 0; k < 9; ++k) H[k] = a.D[9 * (size_t)v + k];
        for (int k = 0; k < 3; ++k) H[4 * k] += lambda;
        if (!inv3(H, Mi)) {
            for (int k = 0; k < 9; ++k) Mi[k] = 0.0;
            a.icnt[I_BAD] = 1;
        }
    }
    for (int k = 0; k < 9; ++k) a.Minv[9 * (size_t)v + k] = Mi[k];
}

__device__ __forceinline__ double precond_row(const RecArgs& a, int i) {
    const int v = i / 3, k = i - 3 * v;
    const double* Pm = a.Minv + 9 * (size_t)v + 3 * k;
    const double* rc = a.r + 3 * (size_t)v;
    return Pm[0] * rc[0] + Pm[1] * rc[1] + Pm[2] * rc[2];
}

__global__ __launch_bounds__(kVecBlock) void rec_pcg_init(RecArgs a) {
    __shared__ double sh[32];
    const int n = 3 * a.n;
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        a.x[i] = 0.0;
        a.r[i] = a.g[i];
    }
    __syncthreads();
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        const double zi = precond_row(a, i), ri = a.r[i];
        a.z[i] = zi;
        a.p[i] = zi;
        v[0] += ri * ri;
        v[1] += ri * zi;
    }
    block_sum<2>(v, sh);
    if (threadIdx.x == 0) {
        a.scal[S_RR] = v[0];
        a.scal[S_RZ] = v[1];
        a.scal[S_BB] = v[0];
    }
}

// ye = A (vec_b - vec_a) per factor
__global__ void rec_prod_edges(RecArgs a, const double* vec) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > a.E || !a.ruse[e]) return;
    const int ka = a.rkey[2 * (size_t)e], kb = a.rkey[2 * (size_t)e + 1];
    const double* L = a.lin + (size_t)e * kLin;
    const double dv[3] = {vec[3 * (size_t)kb] - vec[3 * (size_t)ka], vec[3 * (size_t)kb + 1] - vec[3 * (size_t)ka + 1],
                          vec[3 * (size_t)kb + 2] - vec[3 * (size_t)ka + 2]};
    for (int r = 0; r < 3; ++r) a.ye[3 * (size_t)e + r] = L[3 * r] * dv[0] + L[3 * r + 1] * dv[1] + L[3 * r + 2] * dv[2];
}

// q_v = lambda p_v + sum +-A^T ye (+ the prior): one wave per node over its incidence list
__global__ __launch_bounds__(kNodeBlock) void rec_prod_nodes(RecArgs a, double lambda) {
    const int v = blockIdx.x * (kNodeBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (v >= a.n) return;
    double s[3] = {0.0, 0.0, 0.0};
    if (a.active[v])
        for (int i = a.node_off[v] + lane; i < a.node_off[v + 1]; i += 64) {
            const int e = a.inc[i];
            const double* L = a.lin + (size_t)e * kLin;
            const double* y = a.ye + 3 * (size_t)e;
            const double sg = a.rkey[2 * (size_t)e + 1] == v ? 1.0 : -1.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += sg * (L[c] * y[0] + L[3 + c] * y[1] + L[6 + c] * y[2]);
        }
    wave_sum<3>(s);
    if (lane < 3) {
        const double pk = a.p[3 * (size_t)v + lane];
        double qv = 0.0;
        if (a.active[v]) {
            qv = s[lane] + lambda * pk;
            if (v == rec_prior_node(a)) qv += kPriorW * pk;
        }
        a.q[3 * (size_t)v + lane] = qv;
    }
}

__global__ __launch_bounds__(kVecBlock) void rec_pcg_step(RecArgs a) {
    __shared__ double sh[32];
    const int n = 3 * a.n;
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < n; i += kVecBlock) v[0] += a.p[i] * a.q[i];
    block_sum<1>(v, sh);
    const double rz = a.scal[S_RZ];
    const double alpha = rz / v[0];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        a.x[i] = a.x[i] + alpha * a.p[i];
        a.r[i] = a.r[i] - alpha * a.q[i];
    }
    __syncthreads();
    v[0] = v[1] = 0.0;
    for (int i = threadIdx.x; i < n; i += kVecBlock) {
        const double zi = precond_row(a, i), ri = a.r[i];
        a.z[i] = zi;
        v[0] += ri * ri;
        v[1] += ri * zi;
    }
    block_sum<2>(v, sh);
    const double beta = v[1] / rz;
    for (int i = threadIdx.x; i < n; i += kVecBlock) a.p[i] = a.z[i] + beta * a.p[i];
    if (threadIdx.x == 0) {
        a.scal[S_RR] = v[0];
        a.scal[S_RZ] = v[1];
    }
}

__global__ void rec_update(RecArgs a, const double* X, double* Xn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * a.n) return;
    Xn[i] = a.active[i / 3] ? X[i] + a.x[i] : X[i];
}

// per factor: the linearised cost of the step (ye = A (x_b - x_a) from rec_prod_edges) and the cost at Xn
__global__ void rec_step_cost(RecArgs a, const double* Xn) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e > a.E || !a.ruse[e]) return;
    const double* L = a.lin + (size_t)e * kLin;
    double nl = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double d = a.ye[3 * (size_t)e + k] - L[9 + k];
        nl += d * d;
    }
    a.tl[e] = nl;
    double r[3];
    rec_residual(a, Xn, e, r, nullptr);
    a.te[e] = rec_loss(a, r);
}

__global__ void rec_output(RecArgs a, const double* X, double* wti, uint8_t* wti_valid, double* land,
                           uint8_t* land_valid) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n) return;
    const int r = a.rep[v];
    const bool ok = a.isvar[v] && (v >= a.n_img || !a.rvalid || a.rvalid[v]);
    double* o = v < a.n_img ? wti + 3 * (size_t)v : land + 3 * (size_t)(v - a.n_img);
    for (int k = 0; k < 3; ++k) o[k] = ok ? X[3 * (size_t)r + k] : 0.0;
    if (v < a.n_img) wti_valid[v] = ok;
    else land_valid[v - a.n_img] = ok;
}

__global__ void rec_stats(RecArgs a, double* stats, double err0, double err, double iters, double trials,
                          double pcg_iters, double cap_hits, double status, const uint8_t* wti_valid) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int nv = 0;
    for (int c = 0; c < a.n_img; ++c) nv += wti_valid[c];
    stats[0] = err0;
    stats[1] = err;
    stats[2] = iters;
    stats[3] = trials;
    stats[4] = pcg_iters;
    stats[5] = cap_hits;
    stats[6] = (double)a.icnt[I_NACT];
    stats[7] = (double)a.icnt[I_NFAC];
    stats[8] = (double)nv;
    stats[9] = status;
}

struct RecLayout {
    size_t cam_inl, isvar, active, rep, rkey, ruse, icnt, XA, XB, lin, D, g, Minv, ye, te, tl, vec, scal, node_off, inc,
        hist, total;
    CsrChunks chunks;
};

RecLayout rec_layout(long long E, int n_img, int n) {
    RecLayout L;
    const long long E1 = E + 1;
    L.chunks = csr_chunks(E1, kChunksMax);
    WsCarver w;
    const size_t e = (size_t)E1, v = (size_t)n, d = sizeof(double);
    L.cam_inl = w.take((size_t)n_img);
    L.isvar = w.take(v);
    L.active = w.take(v);
    L.rep = w.take(v * 4);
    L.rkey = w.take(e * 8);
    L.ruse = w.take(e);
    L.icnt = w.take(I_COUNT * 4);
    L.XA = w.take(v * 3 * d);
    L.XB = w.take(v * 3 * d);
    L.lin = w.take(e * kLin * d);
    L.D = w.take(v * 9 * d);
    L.g = w.take(v * 3 * d);
    L.Minv = w.take(v * 9 * d);
    L.ye = w.take(e * 3 * d);
    L.te = w.take(e * d);
    L.tl = w.take(e * d);
    L.vec = w.take(5 * 3 * v * d);
    L.scal = w.take(S_COUNT * d);
    L.node_off = w.take((v + 1) * 4);
    L.inc = w.take(e * 8);
    L.hist = w.take(csr_hist_bytes(L.chunks, v));
    L.total = w.o;
    return L;
}

bool rec_sizes_ok(long long E, int n_img, int n_land) {
    return E > 0 && E < (1ll << 30) && n_img > 0 && n_land >= 0 && (long long)n_img + n_land <= (1 << 24);
}

}  // namespace

extern "C" {

size_t gtsfm_transavg_measurements_workspace_bytes(int n_edges, long long n_tracks, long long n_meas, int n_img) {
    if (n_edges <= 0 || n_img <= 0 || n_tracks < 0 || n_meas < 0 || n_tracks >= (1ll << 30) || n_meas >= (1ll << 30) ||
        n_edges >= (1 << 30) || n_img > (1 << 20))
        return 0;
    return meas_layout(n_tracks, n_meas, n_img).total;
}

int gtsfm_transavg_measurements(const int* d_edges, const double* d_i2Ui1, const uint8_t* d_edge_valid, int n_edges,
                                const double* d_wRi, const uint8_t* d_rot_valid, int n_img,
                                const int* d_track_offsets, const int* d_track_img, const void* d_track_uv,
                                int uv_is_f64, long long n_tracks, const long long* d_n_tracks, long long n_meas,
                                const double* d_intrinsics, int measurements_per_camera, void* d_workspace,
                                size_t workspace_bytes, int* d_meas_key, double* d_meas_dir, uint8_t* d_meas_valid,
                                int* d_selected, uint8_t* d_cam_valid, long long* d_counts, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_edges <= 0 || n_img <= 0 || n_tracks < 0 || n_meas < 0 || n_tracks >= (1ll << 30) || n_meas >= (1ll << 30) ||
        n_edges >= (1 << 30) || n_img > (1 << 20) || measurements_per_camera < 0 || (uv_is_f64 != 0 && uv_is_f64 != 1) ||
        !d_edges || !d_i2Ui1 || !d_wRi || !d_meas_key || !d_meas_dir || !d_meas_valid || !d_cam_valid || !d_counts ||
        !d_workspace)
        return GTSFM_ERR_ARG;
    if (n_tracks > 0 && (!d_track_offsets || !d_selected || !d_intrinsics)) return GTSFM_ERR_ARG;
    if (n_tracks > 0 && n_meas > 0 && (!d_track_img || !d_track_uv)) return GTSFM_ERR_ARG;
    const MeasLayout L = meas_layout(n_tracks, n_meas, n_img);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    MeasArgs a;
    a.edges = d_edges; a.i2Ui1 = d_i2Ui1; a.evalid = d_edge_valid; a.n_edges = n_edges;
    a.wRi = d_wRi; a.rvalid = d_rot_valid; a.n_img = n_img;
    a.off = d_track_offsets; a.img = d_track_img; a.uv = d_track_uv; a.uv64 = uv_is_f64;
    a.T = (int)n_tracks; a.M = n_tracks > 0 ? (int)n_meas : 0; a.d_nt = d_n_tracks; a.intr = d_intrinsics;
    a.per_cam = measurements_per_camera;
    a.key = d_meas_key; a.dir = d_meas_dir; a.mvalid = d_meas_valid; a.selected = d_selected;
    a.cam_valid = d_cam_valid; a.counts = d_counts;
    a.imp = (int*)(ws + L.imp); a.remaining = (int*)(ws + L.remaining); a.mtrack = (int*)(ws + L.mtrack);
    a.sel_off = (int*)(ws + L.sel_off);
    const unsigned B = 256;
    size_t nmax = (size_t)n_edges + (size_t)n_meas;
    if ((size_t)n_img > nmax) nmax = n_img;
    if ((size_t)n_tracks > nmax) nmax = (size_t)n_tracks;
    if (nmax < 4) nmax = 4;
    // the output arrays have n_edges + n_meas slots whatever n_tracks is; a.M = 0 keeps the track kernels off them
    MeasArgs ai = a;
    ai.M = (int)n_meas;
    hipLaunchKernelGGL(ta_meas_init, dim3(blocks_for(nmax, B)), dim3(B), 0, stream, ai);
    hipLaunchKernelGGL(ta_cam_edges, dim3(blocks_for(n_edges, B)), dim3(B), 0, stream, a);
    if (a.T > 0 && a.M > 0) {
        hipLaunchKernelGGL(ta_track_filter, dim3(blocks_for(a.T, B)), dim3(B), 0, stream, a);
        hipLaunchKernelGGL(ta_select, dim3(1), dim3(kSelBlock), 0, stream, a);
        hipLaunchKernelGGL(ta_track_dirs, dim3(blocks_for(a.T, B)), dim3(B), 0, stream, a);
    }
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

size_t gtsfm_transavg_mfas_workspace_bytes(long long n_meas, int n_nodes, int n_dir) {
    if (!mfas_sizes_ok(n_meas, n_nodes, n_dir)) return 0;
    return mfas_layout(n_meas, n_nodes, n_dir).total;
}

int gtsfm_transavg_mfas(const int* d_meas_key, const double* d_meas_dir, const uint8_t* d_meas_valid, long long n_meas,
                        int n_nodes, const double* d_proj, int n_dir, double outlier_weight_threshold,
                        void* d_workspace, size_t workspace_bytes, double* d_outlier_sum, uint8_t* d_inlier,
                        uint32_t* d_violated, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!mfas_sizes_ok(n_meas, n_nodes, n_dir) || !d_meas_key || !d_meas_dir || !d_proj || !d_outlier_sum ||
        !d_inlier || !d_workspace || !(outlier_weight_threshold > 0))
        return GTSFM_ERR_ARG;
    const MfasLayout L = mfas_layout(n_meas, n_nodes, n_dir);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    const int E = (int)n_meas;
    uint8_t* use = ws + L.use;
    hipLaunchKernelGGL(ta_mfas_use, dim3(blocks_for(E, 256)), dim3(256), 0, stream, d_meas_key, d_meas_valid, E, n_nodes,
                       use);
    CsrArgs c;
    c.key = d_meas_key; c.use = use; c.E = E; c.n = n_nodes;
    c.node_off = (int*)(ws + L.node_off); c.inc = (int*)(ws + L.inc); c.hist = (int*)(ws + L.hist);
    c.dup = ws + L.dup; c.chunks = L.chunks;
    int rc = ta_csr_build(c, stream);
    if (rc != GTSFM_OK) return rc;
    MfasArgs a;
    a.key = d_meas_key; a.dir = d_meas_dir; a.use = use; a.E = E; a.n = n_nodes; a.n_dir = n_dir; a.words = L.words;
    a.proj = d_proj; a.node_off = c.node_off; a.inc = c.inc; a.dup = c.dup;
    a.viol = d_violated ? d_violated : (uint32_t*)(ws + L.viol);
    a.thr = outlier_weight_threshold; a.mvalid = d_meas_valid; a.osum = d_outlier_sum; a.inlier = d_inlier;
    const int lds = 20 * n_nodes;  // inSum, outSum, position; n_nodes <= GTSFM_TRANSAVG_MFAS_MAX_NODES keeps it in 160 KiB
    GTSFM_CHECK_HIP(gtsfm_set_dynamic_lds((const void*)ta_mfas, lds));
    hipLaunchKernelGGL(ta_mfas, dim3(n_dir), dim3(kMfasBlock), lds, stream, a);
    hipLaunchKernelGGL(ta_mfas_sum, dim3(blocks_for(E, 256)), dim3(256), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

size_t gtsfm_transavg_recover_workspace_bytes(long long n_meas, int n_img, int n_landmarks) {
    if (!rec_sizes_ok(n_meas, n_img, n_landmarks)) return 0;
    return rec_layout(n_meas, n_img, n_img + n_landmarks).total;
}

int gtsfm_transavg_recover(const int* d_meas_key, const double* d_meas_dir, const uint8_t* d_meas_inlier,
                           long long n_meas, int n_img, int n_landmarks, const uint8_t* d_rot_valid, int robust,
                           double scale, uint64_t seed, int max_iterations, double pcg_rel_tol, int pcg_max_iter,
                           void* d_workspace, size_t workspace_bytes, double* d_wti, uint8_t* d_wti_valid,
                           double* d_landmark, uint8_t* d_landmark_valid, double* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!rec_sizes_ok(n_meas, n_img, n_landmarks) || !d_meas_key || !d_meas_dir || !d_meas_inlier || !d_workspace ||
        !d_wti || !d_wti_valid || !d_stats || (n_landmarks > 0 && (!d_landmark || !d_landmark_valid)) ||
        max_iterations < 0 || !(pcg_rel_tol > 0) || pcg_max_iter <= 0 || !isfinite(scale))
        return GTSFM_ERR_ARG;
    const int E = (int)n_meas, n = n_img + n_landmarks;
    const RecLayout L = rec_layout(E, n_img, n);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;
    unsigned char* ws = (unsigned char*)d_workspace;
    RecArgs a;
    a.key = d_meas_key; a.dir = d_meas_dir; a.inl = d_meas_inlier; a.E = E; a.n_img = n_img; a.n_land = n_landmarks;
    a.n = n; a.rvalid = d_rot_valid; a.robust = robust != 0; a.scale = scale; a.seed = seed;
    a.cam_inl = ws + L.cam_inl; a.isvar = ws + L.isvar; a.active = ws + L.active; a.rep = (int*)(ws + L.rep);
    a.rkey = (int*)(ws + L.rkey); a.ruse = ws + L.ruse; a.icnt = (int*)(ws + L.icnt);
    a.XA = (double*)(ws + L.XA); a.XB = (double*)(ws + L.XB); a.lin = (double*)(ws + L.lin);
    a.D = (double*)(ws + L.D); a.g = (double*)(ws + L.g); a.Minv = (double*)(ws + L.Minv);
    a.ye = (double*)(ws + L.ye); a.te = (double*)(ws + L.te); a.tl = (double*)(ws + L.tl);
    double* vec = (double*)(ws + L.vec);
    const size_t n3 = 3 * (size_t)n;
    a.x = vec; a.r = vec + n3; a.z = vec + 2 * n3; a.p = vec + 3 * n3; a.q = vec + 4 * n3;
    a.scal = (double*)(ws + L.scal);
    a.node_off = (int*)(ws + L.node_off); a.inc = (int*)(ws + L.inc);

    const unsigned B = 256;
    const unsigned gE = blocks_for((size_t)E + 1, B), gN = blocks_for(n, B), gW = blocks_for(n, kNodeBlock / 64),
                   g3 = blocks_for(n3, B);
    int icnt[I_COUNT];
    double scal[6];
    auto read_icnt = [&]() { return read_back(icnt, a.icnt, I_COUNT, stream); };
    auto read_scal = [&]() { return read_back(scal, a.scal, 6, stream); };
    const size_t nmax = (size_t)E + 1 > (size_t)n ? (size_t)E + 1 : (size_t)n;
    hipLaunchKernelGGL(rec_init, dim3(blocks_for(nmax, B)), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(rec_caminl, dim3(gE), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(rec_keep, dim3(gE), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(rec_merge, dim3(1), dim3(kVecBlock), 0, stream, a);
    hipLaunchKernelGGL(rec_factors, dim3(gE), dim3(B), 0, stream, a);
    hipLaunchKernelGGL(rec_start, dim3(gN), dim3(B), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    int rc = read_icnt();
    if (rc != GTSFM_OK) return rc;
    double* X = a.XA;
    double* Xn = a.XB;
    double err0 = 0.0, err = 0.0, status = icnt[I_NKEPT] == 0 ? 1.0 : 0.0;
    long long iters = 0, trials = 0, pcg_total = 0, cap_hits = 0;
    if (icnt[I_NFAC] > 0) {
        CsrArgs c;
        c.key = a.rkey; c.use = a.ruse; c.E = E + 1; c.n = n;
        c.node_off = (int*)(ws + L.node_off); c.inc = (int*)(ws + L.inc); c.hist = (int*)(ws + L.hist);
        c.dup = nullptr; c.chunks = L.chunks;
        if ((rc = ta_csr_build(c, stream)) != GTSFM_OK) return rc;
        hipLaunchKernelGGL(rec_eval, dim3(gE), dim3(B), 0, stream, a, X);
        hipLaunchKernelGGL(rec_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, X, X, 0);
        GTSFM_CHECK_HIP(hipGetLastError());
        if ((rc = read_scal()) != GTSFM_OK) return rc;
        err0 = err = scal[S_NEWERR];
        double lambda = 1e-5;
        const int max_iters = max_iterations > 0 ? max_iterations : 100;
        if (err > 0.0 && isfinite(err)) {
            for (;;) {  // ends: every outer step either accepts (iters <= max_iters) or leaves err unchanged (dec = 0)
                const double cur = err;
                hipLaunchKernelGGL(rec_linearize, dim3(gE), dim3(B), 0, stream, a, X);
                hipLaunchKernelGGL(rec_node_lin, dim3(gW), dim3(kNodeBlock), 0, stream, a, X);
                hipLaunchKernelGGL(rec_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, X, X, 0);
                GTSFM_CHECK_HIP(hipGetLastError());
                if ((rc = read_scal()) != GTSFM_OK) return rc;
                const double oldLin = scal[S_OLDLIN];
                for (int inner = 0; inner < kInnerMax; ++inner) {
                    ++trials;
                    GTSFM_CHECK_HIP(hipMemsetAsync(a.icnt + I_BAD, 0, sizeof(int), stream));
                    hipLaunchKernelGGL(rec_damp, dim3(gN), dim3(B), 0, stream, a, lambda);
                    hipLaunchKernelGGL(rec_pcg_init, dim3(1), dim3(kVecBlock), 0, stream, a);
                    GTSFM_CHECK_HIP(hipGetLastError());
                    if ((rc = read_icnt()) != GTSFM_OK) return rc;
                    LmTrial trial;
                    if (!icnt[I_BAD]) {
                        if ((rc = read_scal()) != GTSFM_OK) return rc;
                        rc = pcg_iterate(scal[S_BB], scal[S_RR], pcg_rel_tol, pcg_max_iter, pcg_total, cap_hits,
                                         [&](double& rr) -> int {
                            hipLaunchKernelGGL(rec_prod_edges, dim3(gE), dim3(B), 0, stream, a, a.p);
                            hipLaunchKernelGGL(rec_prod_nodes, dim3(gW), dim3(kNodeBlock), 0, stream, a, lambda);
                            hipLaunchKernelGGL(rec_pcg_step, dim3(1), dim3(kVecBlock), 0, stream, a);
                            GTSFM_CHECK_HIP(hipGetLastError());
                            const int rc2 = read_scal();
                            rr = scal[S_RR];
                            return rc2;
                        });
                        if (rc != GTSFM_OK) return rc;
                        hipLaunchKernelGGL(rec_update, dim3(g3), dim3(B), 0, stream, a, X, Xn);
                        hipLaunchKernelGGL(rec_prod_edges, dim3(gE), dim3(B), 0, stream, a, a.x);
                        hipLaunchKernelGGL(rec_step_cost, dim3(gE), dim3(B), 0, stream, a, Xn);
                        hipLaunchKernelGGL(rec_reduce, dim3(1), dim3(kVecBlock), 0, stream, a, Xn, X, 1);
                        GTSFM_CHECK_HIP(hipGetLastError());
                        if ((rc = read_scal()) != GTSFM_OK) return rc;
                        trial = lm_judge(err, oldLin, scal[S_NEWLIN], scal[S_NEWERR]);
                    }
                    if (trial.success) {
                        double* s = X; X = Xn; Xn = s;
                        err = trial.newErr;
                        ++iters;
                    }
                    if (lm_trials_done(trial, lambda)) break;
                }
                if (lm_done(cur, err, iters, max_iters)) break;
            }
        }
        if (!isfinite(err)) status = 2.0;
    }
    hipLaunchKernelGGL(rec_output, dim3(gN), dim3(B), 0, stream, a, X, d_wti, d_wti_valid, d_landmark,
                       d_landmark_valid);
    hipLaunchKernelGGL(rec_stats, dim3(1), dim3(64), 0, stream, a, d_stats, err0, err, (double)iters, (double)trials,
                       (double)pcg_total, (double)cap_hits, status, d_wti_valid);
    GTSFM_CHECK_HIP(hipGetLastError());
    GTSFM_CHECK_HIP(hipStreamSynchronize(stream));
    return GTSFM_OK;
}

}  // extern "C"
