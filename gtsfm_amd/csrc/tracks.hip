// 2D feature tracks from verified correspondences: a lock-free union-find over (image, keypoint) nodes, then a
// grouping into tracks in canonical order.
//
// Reference: gtsfm/data_association/dsf_tracks_estimator.py:56-85 DsfTracksEstimator.run (one dsf.merge per row in a
// Python loop, dsf.sets(), then the unique-camera filter of gtsfm/common/sfm_track.py:105-112) and
// cpp_dsf_tracks_estimator.py:63-74 (the same through gtsam's tracksFromPairwiseMatches).
//
// Node id = image * kmax + keypoint, N = n_img * kmax < 2^31 nodes. Phases, one kernel boundary between each (the only
// ordering the algorithm relies on; nothing waits on another lane, wave or workgroup inside a kernel):
//   1. union     one lane per correspondence row. The row's pair comes from a binary search of d_offsets that is
//                narrowed to the pairs the wave's 64 consecutive rows span. Hooking keeps parent[x] <= x: both roots
//                are found with path halving, the larger is hooked onto the smaller by atomicCAS(parent[big], big,
//                small), and a lost CAS continues from the value it returned. Every chain strictly decreases, so every
//                loop ends; a node becomes a non-root exactly once, so a component's root ends as its smallest id
//                whatever the arrival order. parent is read and halved with relaxed loads and stores: a stale value
//                is an older ancestor of the same component, still on a decreasing chain to the root.
//   2. flatten   one lane per node: root[x], and a slot in the root's member counter. A wave groups its lanes by root
//                with ballots and issues one atomic add per distinct root, so a fused component of many nodes costs
//                its counter one add per wave.
//   3. scan A    exclusive scan of the member counts over node ids: every component's segment in `members`.
//   4. place     members[segment + slot] = node. Slots follow arrival order; nothing below depends on it.
//   5. rank      one lane per touched node reads its component's segment: rank = members with a smaller id, and a
//                second member of its own image marks the component erroneous. A component of more than n_img members
//                is erroneous by counting and is not read. Work is bounded by n_img per node.
//   6. scan B    exclusive scans of (is a track) and (its size) over node ids: track index and measurement offset.
//                Ascending root = ascending smallest member, so this is the canonical track order.
//   7. scatter   measurement[offset(root) + rank] = (image, keypoint, uv): ascending node id inside a track.
// The scans are three kernels each (tile sums, one workgroup over the tile sums, apply): no look-back between
// workgroups. All outputs are functions of the set of rows, so they are byte-identical from launch to launch.
#include <algorithm>

#include "common.hpp"
#include "reduce.hpp"  // uf_unite

namespace {

typedef unsigned long long u64;

#define TR_BLOCK 256
#define TR_SCAN_PER_THREAD 8
#define TR_SCAN_TILE (TR_BLOCK * TR_SCAN_PER_THREAD)
#define TR_UNION_MAX_BLOCKS 2048  // 8 workgroups per CU; more rows than 2048 x 256 are grid-strided

struct TrLayout {
    // zeroed on every call: [zero_begin, zero_end)
    size_t cnt, bad, touched, counters, zero_end;
    size_t parent, root, slot, seg, members, rank, tile_sums, total;
};

// counters: u64 bad_rows, then u32 totals[4] = {touched, components, measurements, tracks}
#define TR_COUNTER_BYTES 32

inline size_t tr_tiles(size_t N) { return (N + TR_SCAN_TILE - 1) / TR_SCAN_TILE; }

inline TrLayout tr_layout(size_t N) {
    TrLayout L;
    WsCarver w;
    L.cnt = w.take(N * 4);
    L.bad = w.take(N);
    L.touched = w.take(N);
    L.counters = w.take(TR_COUNTER_BYTES);
    L.zero_end = w.o;
    L.parent = w.take(N * 4);
    L.root = w.take(N * 4);
    L.slot = w.take(N * 4);     // member slot, later the track index of a root
    L.seg = w.take(N * 4);      // segment base of a root, later its measurement offset
    L.members = w.take(N * 4);
    L.rank = w.take(N * 4);
    L.tile_sums = w.take(tr_tiles(N) * 2 * 4);
    L.total = w.o;
    return L;
}

// Largest p in [lo, hi) with offsets[p] <= row, given offsets[lo] <= row.
__device__ __forceinline__ int tr_pair_of(const int* __restrict__ offsets, int lo, int hi, int row) {
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= row) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(TR_BLOCK) void tr_init_kernel(int* __restrict__ parent, unsigned N) {
    const unsigned x = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (x < N) parent[x] = (int)x;
}

__global__ __launch_bounds__(TR_BLOCK) void tr_union_kernel(const int* __restrict__ pairs,
                                                            const int* __restrict__ offsets,
                                                            const uint2* __restrict__ v_corr,
                                                            const uint8_t* __restrict__ valid,
                                                            const int* __restrict__ kp_count, int n_img, int kmax,
                                                            int n_pairs, long long n_rows, int* parent,
                                                            uint8_t* touched, u64* bad_rows) {
    const int row_begin = std::max(offsets[0], 0);
    const long long row_end = std::min<long long>(offsets[n_pairs], n_rows);
    const int lane = threadIdx.x & 63;
    unsigned n_bad = 0;
    // wave-uniform trip count: whole waves reach the ballot after the loop
    for (long long base = row_begin + ((long long)blockIdx.x * TR_BLOCK + (threadIdx.x & ~63)); base < row_end;
         base += (long long)gridDim.x * TR_BLOCK) {
        const long long row = base + lane;
        if (row >= row_end) continue;
        // the pairs of the wave's first and last row bracket every lane's search
        const long long last = std::min<long long>(base + 63, row_end - 1);
        const int p_lo = tr_pair_of(offsets, 0, n_pairs, (int)base);
        const int p_hi = tr_pair_of(offsets, p_lo, n_pairs, (int)last);
        const int p = tr_pair_of(offsets, p_lo, p_hi + 1, (int)row);
        if (valid && !valid[p]) continue;
        const int i1 = pairs[2 * p], i2 = pairs[2 * p + 1];
        const uint2 k = v_corr[row];
        bool ok = (unsigned)i1 < (unsigned)n_img && (unsigned)i2 < (unsigned)n_img;
        if (ok) {
            const int n1 = std::min(kp_count[i1], kmax), n2 = std::min(kp_count[i2], kmax);
            ok = n1 > 0 && n2 > 0 && k.x < (unsigned)n1 && k.y < (unsigned)n2;
        }
        if (!ok) {
            ++n_bad;
            continue;
        }
        const int u = i1 * kmax + (int)k.x, v = i2 * kmax + (int)k.y;
        touched[u] = 1;
        touched[v] = 1;
        uf_unite(parent, u, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_bad += __shfl_xor(n_bad, o, 64);
    if (lane == 0 && n_bad) atomicAdd(bad_rows, (u64)n_bad);  // one add per wave
}

__global__ __launch_bounds__(TR_BLOCK) void tr_flatten_kernel(const int* __restrict__ parent,
                                                              const uint8_t* __restrict__ touched, unsigned N,
                                                              int* __restrict__ root, unsigned* __restrict__ cnt,
                                                              unsigned* __restrict__ slot) {
    const unsigned x = blockIdx.x * TR_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool on = x < N && touched[x];
    int r = -1;
    if (on) {
        r = (int)x;
        for (int p = parent[r]; p != r; p = parent[r]) r = p;
    }
    if (x < N) root[x] = r;
    // a slot in the root's member count: the wave's lanes are grouped by root with ballots (registers only, one
    // round per distinct root), then the first lane of every group adds the group's size, all groups in one atomic
    // instruction. A component fused from many nodes then costs its counter one add per wave, not one per node.
    u64 rest = __ballot(on);
    if (rest == 0) return;
    const u64 below = (1ull << lane) - 1;
    int leader = lane;
    unsigned ahead = 0, size = 1;
    while (rest) {  // wave-uniform: rest is built from ballots
        const int first = __ffsll((long long)rest) - 1;
        const int r0 = __shfl(r, first, 64);
        const bool mine = on && r == r0;
        const u64 group = __ballot(mine);  // holds `first`, so rest shrinks every round
        if (mine) {
            leader = first;
            ahead = (unsigned)__popcll(group & below);
            size = (unsigned)__popcll(group);
        }
        rest &= ~group;
    }
    unsigned base = 0;
    if (on && leader == lane) base = atomicAdd(cnt + r, size);
    base = __shfl(base, leader, 64);
    if (on) slot[x] = base + ahead;
}

// ---- exclusive scan over node ids of (v0, v1) = (members, 1) of every root that counts in this pass ----
// pass A: every component. pass B: the components that are tracks (not marked bad).
__device__ __forceinline__ unsigned tr_scan_value(const unsigned* __restrict__ cnt, const uint8_t* __restrict__ bad,
                                                  bool tracks_only, unsigned x, unsigned N) {
    if (x >= N) return 0;
    const unsigned c = cnt[x];
    return (c && tracks_only && bad[x]) ? 0u : c;
}

// Block-wide exclusive scan of one value per thread (TR_BLOCK threads); returns the exclusive prefix, total in `sum`.
__device__ __forceinline__ unsigned tr_block_exscan(unsigned v, unsigned* lds, unsigned& sum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    __syncthreads();  // lds is reused between calls
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    unsigned before = 0;
    sum = 0;
#pragma unroll
    for (int i = 0; i < TR_BLOCK / 64; ++i) {
        const unsigned t = lds[i];
        if (i < w) before += t;
        sum += t;
    }
    return before + incl - v;
}

__global__ __launch_bounds__(TR_BLOCK) void tr_tile_sums_kernel(const unsigned* __restrict__ cnt,
                                                                const uint8_t* __restrict__ bad, int tracks_only,
                                                                unsigned N, unsigned* __restrict__ tile_sums) {
    __shared__ unsigned lds[2 * (TR_BLOCK / 64)];
    const size_t x0 = (size_t)blockIdx.x * TR_SCAN_TILE + (size_t)threadIdx.x * TR_SCAN_PER_THREAD;
    unsigned s0 = 0, s1 = 0;
#pragma unroll
    for (int j = 0; j < TR_SCAN_PER_THREAD; ++j) {
        const unsigned c = x0 + j < N ? tr_scan_value(cnt, bad, tracks_only, (unsigned)(x0 + j), N) : 0u;
        s0 += c;
        s1 += c ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s0 += __shfl_xor(s0, o, 64);
        s1 += __shfl_xor(s1, o, 64);
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        lds[2 * w] = s0;
        lds[2 * w + 1] = s1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t0 = 0, t1 = 0;
        for (int i = 0; i < TR_BLOCK / 64; ++i) {
            t0 += lds[2 * i];
            t1 += lds[2 * i + 1];
        }
        tile_sums[2 * (size_t)blockIdx.x] = t0;
        tile_sums[2 * (size_t)blockIdx.x + 1] = t1;
    }
}

// One workgroup turns the tile sums into exclusive prefixes in place and writes the two totals.
__global__ __launch_bounds__(TR_BLOCK) void tr_scan_tiles_kernel(unsigned* __restrict__ tile_sums, unsigned n_tiles,
                                                                 unsigned* __restrict__ totals) {
    __shared__ unsigned lds[TR_BLOCK / 64];
    unsigned carry0 = 0, carry1 = 0;
    for (unsigned b0 = 0; b0 < n_tiles; b0 += TR_BLOCK) {  // block-uniform trip count
        const unsigned b = b0 + threadIdx.x;
        const unsigned v0 = b < n_tiles ? tile_sums[2 * (size_t)b] : 0u;
        const unsigned v1 = b < n_tiles ? tile_sums[2 * (size_t)b + 1] : 0u;
        unsigned sum0, sum1;
        const unsigned e0 = tr_block_exscan(v0, lds, sum0);
        const unsigned e1 = tr_block_exscan(v1, lds, sum1);
        if (b < n_tiles) {
            tile_sums[2 * (size_t)b] = carry0 + e0;
            tile_sums[2 * (size_t)b + 1] = carry1 + e1;
        }
        carry0 += sum0;
        carry1 += sum1;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry0;
        totals[1] = carry1;
    }
}

__global__ __launch_bounds__(TR_BLOCK) void tr_scan_apply_kernel(const unsigned* __restrict__ cnt,
                                                                 const uint8_t* __restrict__ bad, int tracks_only,
                                                                 unsigned N, const unsigned* __restrict__ tile_sums,
                                                                 unsigned* __restrict__ out0,
                                                                 unsigned* __restrict__ out1) {
    __shared__ unsigned lds[TR_BLOCK / 64];
    const size_t x0 = (size_t)blockIdx.x * TR_SCAN_TILE + (size_t)threadIdx.x * TR_SCAN_PER_THREAD;
    unsigned c[TR_SCAN_PER_THREAD];
    unsigned s0 = 0, s1 = 0;
#pragma unroll
    for (int j = 0; j < TR_SCAN_PER_THREAD; ++j) {
        c[j] = x0 + j < N ? tr_scan_value(cnt, bad, tracks_only, (unsigned)(x0 + j), N) : 0u;
        s0 += c[j];
        s1 += c[j] ? 1u : 0u;
    }
    unsigned sum;
    unsigned e0 = tile_sums[2 * (size_t)blockIdx.x] + tr_block_exscan(s0, lds, sum);
    unsigned e1 = tile_sums[2 * (size_t)blockIdx.x + 1] + tr_block_exscan(s1, lds, sum);
#pragma unroll
    for (int j = 0; j < TR_SCAN_PER_THREAD; ++j) {
        if (x0 + j < N && c[j]) {  // only roots that count are read back
            out0[x0 + j] = e0;
            if (out1) out1[x0 + j] = e1;
        }
        e0 += c[j];
        e1 += c[j] ? 1u : 0u;
    }
}

__global__ __launch_bounds__(TR_BLOCK) void tr_place_kernel(const int* __restrict__ root,
                                                            const unsigned* __restrict__ slot,
                                                            const unsigned* __restrict__ seg, unsigned N,
                                                            int* __restrict__ members) {
    const unsigned x = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (x >= N) return;
    const int r = root[x];
    if (r < 0) return;
    members[seg[r] + slot[x]] = (int)x;  // seg[r] + slot < touched nodes <= N
}

__global__ __launch_bounds__(TR_BLOCK) void tr_rank_kernel(const int* __restrict__ root,
                                                           const unsigned* __restrict__ cnt,
                                                           const unsigned* __restrict__ seg,
                                                           const int* __restrict__ members, unsigned N, int n_img,
                                                           int kmax, unsigned* __restrict__ rank,
                                                           uint8_t* __restrict__ bad) {
    const unsigned x = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (x >= N) return;
    const int r = root[x];
    if (r < 0) return;
    const unsigned n = cnt[r];
    if (n > (unsigned)n_img) {  // more members than images: two of them share one
        if ((int)x == r) bad[r] = 1;
        return;
    }
    const int* m = members + seg[r];
    const int img_lo = (int)(x / (unsigned)kmax) * kmax, img_hi = img_lo + kmax;  // the ids of x's image
    unsigned below = 0;
    bool dup = false;
    for (unsigned j = 0; j < n; ++j) {
        const int y = m[j];
        below += y < (int)x ? 1u : 0u;
        dup |= y >= img_lo && y < img_hi && y != (int)x;
    }
    rank[x] = below;
    if (dup) bad[r] = 1;  // every writer stores the same value
}

__global__ __launch_bounds__(TR_BLOCK) void tr_scatter_kernel(const int* __restrict__ root,
                                                              const uint8_t* __restrict__ bad,
                                                              const unsigned* __restrict__ moff,
                                                              const unsigned* __restrict__ tidx,
                                                              const unsigned* __restrict__ rank,
                                                              const float2* __restrict__ kp_xy, unsigned N, int kmax,
                                                              long long track_cap, long long meas_cap,
                                                              int* __restrict__ track_offsets,
                                                              int* __restrict__ track_img, int* __restrict__ track_kp,
                                                              float2* __restrict__ track_uv) {
    const unsigned x = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (x >= N) return;
    const int r = root[x];
    if (r < 0 || bad[r]) return;
    const unsigned base = moff[r];
    if ((int)x == r && (long long)tidx[r] <= track_cap) track_offsets[tidx[r]] = (int)base;
    const unsigned pos = base + rank[x];
    if ((long long)pos >= meas_cap) return;
    track_img[pos] = (int)(x / (unsigned)kmax);
    track_kp[pos] = (int)(x % (unsigned)kmax);
    if (kp_xy && track_uv) track_uv[pos] = kp_xy[x];
}

__global__ void tr_stats_kernel(const u64* __restrict__ bad_rows, const unsigned* __restrict__ totals,
                                long long track_cap, int* __restrict__ track_offsets, long long* __restrict__ stats) {
    const unsigned n_comp = totals[1], n_meas = totals[2], n_tracks = totals[3];
    stats[0] = n_tracks;
    stats[1] = n_meas;
    stats[2] = n_comp;
    stats[3] = (long long)n_comp - (long long)n_tracks;
    stats[4] = (long long)bad_rows[0];
    if ((long long)n_tracks <= track_cap) track_offsets[n_tracks] = (int)n_meas;
}

}  // namespace

extern "C" {

size_t gtsfm_tracks_workspace_bytes(int n_img, int kmax, int n_pairs, long long n_rows) {
    if (n_img <= 0 || kmax <= 0 || n_pairs <= 0 || n_rows <= 0) return 0;
    if ((long long)n_img * kmax >= (1ll << 31) || n_rows >= (1ll << 31)) return 0;
    return tr_layout((size_t)n_img * kmax).total;
}

int gtsfm_tracks_from_matches(const int* d_pairs, const int* d_offsets, const uint32_t* d_v_corr,
                              const uint8_t* d_valid, int n_pairs, long long n_rows, const int* d_kp_count,
                              const float* d_kp_xy, int n_img, int kmax, void* d_workspace, size_t workspace_bytes,
                              int* d_track_offsets, long long track_cap, int* d_track_img, int* d_track_kp,
                              float* d_track_uv, long long meas_cap, long long* d_stats, void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (n_img < 0 || kmax < 0 || n_pairs < 0 || n_rows < 0 || track_cap < 0 || meas_cap < 0) return GTSFM_ERR_ARG;
    if ((long long)n_img * kmax >= (1ll << 31) || n_rows >= (1ll << 31)) return GTSFM_ERR_ARG;
    if (!d_stats || !d_track_offsets) return GTSFM_ERR_ARG;
    if (n_pairs == 0 || n_rows == 0) {  // no rows: no components. Nothing below indexes an input.
        GTSFM_CHECK_HIP(hipMemsetAsync(d_stats, 0, 5 * sizeof(long long), stream));
        GTSFM_CHECK_HIP(hipMemsetAsync(d_track_offsets, 0, sizeof(int), stream));
        return GTSFM_OK;
    }
    if (n_img == 0 || kmax == 0) return GTSFM_ERR_ARG;
    if (!d_pairs || !d_offsets || !d_v_corr || !d_kp_count || !d_workspace) return GTSFM_ERR_ARG;
    if (meas_cap > 0 && (!d_track_img || !d_track_kp)) return GTSFM_ERR_ARG;
    const size_t N = (size_t)n_img * kmax;
    const TrLayout L = tr_layout(N);
    if (workspace_bytes < L.total) return GTSFM_ERR_ARG;

    char* ws = (char*)d_workspace;
    unsigned* cnt = (unsigned*)(ws + L.cnt);
    uint8_t* bad = (uint8_t*)(ws + L.bad);
    uint8_t* touched = (uint8_t*)(ws + L.touched);
    u64* bad_rows = (u64*)(ws + L.counters);
    unsigned* totals = (unsigned*)(ws + L.counters + 8);
    int* parent = (int*)(ws + L.parent);
    int* root = (int*)(ws + L.root);
    unsigned* slot = (unsigned*)(ws + L.slot);
    unsigned* seg = (unsigned*)(ws + L.seg);
    int* members = (int*)(ws + L.members);
    unsigned* rank = (unsigned*)(ws + L.rank);
    unsigned* tile_sums = (unsigned*)(ws + L.tile_sums);

    const unsigned Nu = (unsigned)N;
    const unsigned node_blocks = (unsigned)((N + TR_BLOCK - 1) / TR_BLOCK);
    const unsigned n_tiles = (unsigned)tr_tiles(N);
    const unsigned union_blocks =
        (unsigned)std::min<long long>(TR_UNION_MAX_BLOCKS, (n_rows + TR_BLOCK - 1) / TR_BLOCK);

    GTSFM_CHECK_HIP(hipMemsetAsync(ws, 0, L.zero_end, stream));
    hipLaunchKernelGGL(tr_init_kernel, dim3(node_blocks), dim3(TR_BLOCK), 0, stream, parent, Nu);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(tr_union_kernel, dim3(union_blocks), dim3(TR_BLOCK), 0, stream, d_pairs, d_offsets,
                       (const uint2*)d_v_corr, d_valid, d_kp_count, n_img, kmax, n_pairs, n_rows, parent, touched,
                       bad_rows);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(tr_flatten_kernel, dim3(node_blocks), dim3(TR_BLOCK), 0, stream, parent, touched, Nu, root, cnt,
                       slot);
    GTSFM_CHECK_HIP(hipGetLastError());
    // scan A: segment base of every component; totals[0] = touched nodes, totals[1] = components
    hipLaunchKernelGGL(tr_tile_sums_kernel, dim3(n_tiles), dim3(TR_BLOCK), 0, stream, cnt, bad, 0, Nu, tile_sums);
    hipLaunchKernelGGL(tr_scan_tiles_kernel, dim3(1), dim3(TR_BLOCK), 0, stream, tile_sums, n_tiles, totals);
    hipLaunchKernelGGL(tr_scan_apply_kernel, dim3(n_tiles), dim3(TR_BLOCK), 0, stream, cnt, bad, 0, Nu, tile_sums, seg,
                       (unsigned*)nullptr);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(tr_place_kernel, dim3(node_blocks), dim3(TR_BLOCK), 0, stream, root, slot, seg, Nu, members);
    hipLaunchKernelGGL(tr_rank_kernel, dim3(node_blocks), dim3(TR_BLOCK), 0, stream, root, cnt, seg, members, Nu, n_img,
                       kmax, rank, bad);
    GTSFM_CHECK_HIP(hipGetLastError());
    // scan B: measurement offset (over seg) and track index (over slot) of every track; totals[2], totals[3]
    hipLaunchKernelGGL(tr_tile_sums_kernel, dim3(n_tiles), dim3(TR_BLOCK), 0, stream, cnt, bad, 1, Nu, tile_sums);
    hipLaunchKernelGGL(tr_scan_tiles_kernel, dim3(1), dim3(TR_BLOCK), 0, stream, tile_sums, n_tiles, totals + 2);
    hipLaunchKernelGGL(tr_scan_apply_kernel, dim3(n_tiles), dim3(TR_BLOCK), 0, stream, cnt, bad, 1, Nu, tile_sums, seg,
                       slot);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(tr_scatter_kernel, dim3(node_blocks), dim3(TR_BLOCK), 0, stream, root, bad, seg, slot, rank,
                       (const float2*)d_kp_xy, Nu, kmax, track_cap, meas_cap, d_track_offsets, d_track_img, d_track_kp,
                       (float2*)d_track_uv);
    hipLaunchKernelGGL(tr_stats_kernel, dim3(1), dim3(1), 0, stream, bad_rows, totals, track_cap, d_track_offsets,
                       d_stats);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // extern "C"
