// The input of global bundle adjustment from the triangulated tracks: the largest connected component of cameras, where
// two cameras are joined when one accepted 3D track sees both, and the tracks that lie wholly inside it.
//
// Reference: gtsfm/data_association/data_assoc.py:123-160 (the valid tracks, then select_largest_connected_component),
// gtsfm/common/gtsfm_data.py:238-317 (the camera edges of every track, from_selected_cameras) and
// gtsfm/utils/graph.py:20-39 (max(nx.connected_components(G), key=len)). Semantics in include/gtsfm_hip.h.
//
// Integers only. Phases, one kernel boundary between each (the only ordering relied on; nothing waits on another lane,
// wave or workgroup inside a kernel):
//   1. init     parent[i] = i, per-camera counters cleared, d_stats cleared.
//   2. track    one lane per track: accepted or not, its inlier count and its first inlier camera.
//   3. union    one lane per measurement, then one per extra edge. A measurement finds its track by a binary search of
//               the offsets and unites its camera with the track's first inlier camera (reduce.hpp's uf_unite: every
//               chain strictly descends, a retry follows only another lane's successful CAS).
//   4. root     one lane per camera: root[i] by a read-only walk, one integer atomicAdd into the root's size.
//   5. first    one lane per track and per extra edge: atomicMin of the item's index into its root.
//   6. select   one workgroup reduces the roots to the winner: most cameras, then the smallest first item.
//   7. cameras  one lane per camera: d_cam_keep, and the camera counts.
//   8. tracks   one lane per track: d_track_keep, d_track_len, and the track counts.
// Every output is a function of the input set: a component's root is its smallest camera whatever the arrival order,
// sizes and first items are sums and minima of integers.
#include <algorithm>

#include "common.hpp"
#include "reduce.hpp"  // uf_unite

namespace {

typedef unsigned long long u64;

#define AS_BLOCK 256

enum { AS_COMPONENTS, AS_CAMS_KEPT, AS_TRACKS_KEPT, AS_MEAS_KEPT, AS_ACCEPTED, AS_CAMS_VALID, AS_STATS };

struct AsLayout {
    size_t parent, size, first, root, isnode, tfirst, tlen, winner, total;
};

inline AsLayout as_layout(size_t n_tracks, size_t n_img) {
    AsLayout L;
    WsCarver w;
    L.parent = w.take(n_img * 4);
    L.size = w.take(n_img * 4);
    L.first = w.take(n_img * 4);
    L.root = w.take(n_img * 4);
    L.isnode = w.take(n_img);
    L.tfirst = w.take(n_tracks * 4);  // first inlier camera of an accepted track of >= 2 measurements, else -1
    L.tlen = w.take(n_tracks * 4);    // inlier count of an accepted track, else -1
    L.winner = w.take(4);
    L.total = w.o;
    return L;
}

inline bool as_sizes_ok(long long n_tracks, long long n_meas, int n_img, long long n_extra) {
    const long long lim = (1ll << 31) - 1;
    return n_tracks >= 0 && n_meas >= 0 && n_img >= 0 && n_extra >= 0 && n_tracks + n_extra < lim &&
           n_meas + n_extra < lim;
}

struct AsArgs {
    const int* offsets;
    const int* img;
    const long long* n_tracks_dev;
    const uint8_t* track_valid;
    const uint8_t* inlier;
    const uint8_t* cam_valid;
    const int* extra;
    int n_tracks, n_meas, n_img, n_extra;
    int *parent, *size, *first, *root, *tfirst, *tlen, *winner;
    uint8_t* isnode;
    uint8_t* cam_keep;
    uint8_t* track_keep;
    int* track_len;
    u64* stats;
};

__device__ __forceinline__ int as_tracks_in_use(const AsArgs& a) {
    if (!a.n_tracks_dev) return a.n_tracks;
    const long long n = a.n_tracks_dev[0];
    return (int)std::min<long long>(std::max<long long>(n, 0), a.n_tracks);
}

__device__ __forceinline__ bool as_cam_ok(const AsArgs& a, int c) {
    return (unsigned)c < (unsigned)a.n_img && (!a.cam_valid || a.cam_valid[c]);
}

// Adds the number of lanes of the wave with `flag` set to *counter: one atomic per wave. Whole waves must call it.
__device__ __forceinline__ void as_count(u64* counter, bool flag) {
    const u64 b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(counter, (u64)__popcll(b));
}

__global__ __launch_bounds__(AS_BLOCK) void as_init_kernel(AsArgs a) {
    const int i = blockIdx.x * AS_BLOCK + threadIdx.x;
    if (i < AS_STATS) a.stats[i] = 0;
    if (i == 0) a.winner[0] = -1;
    if (i >= a.n_img) return;
    a.parent[i] = i;
    a.size[i] = 0;
    a.first[i] = 0x7fffffff;
    a.isnode[i] = 0;
}

__global__ __launch_bounds__(AS_BLOCK) void as_track_kernel(AsArgs a) {
    const int t = blockIdx.x * AS_BLOCK + threadIdx.x;
    bool accepted = false;
    if (t < as_tracks_in_use(a)) {
        const int lo = a.offsets[t], hi = a.offsets[t + 1];
        accepted = (!a.track_valid || a.track_valid[t]) && lo >= 0 && lo <= hi && hi <= a.n_meas;
        int n = 0, c0 = -1;
        if (accepted) {
            for (int m = lo; m < hi; ++m) {
                if (a.inlier && !a.inlier[m]) continue;
                ++n;
                const int c = a.img[m];
                if (c0 < 0 && (unsigned)c < (unsigned)a.n_img) c0 = c;
            }
        }
        a.tlen[t] = accepted ? n : -1;
        a.tfirst[t] = n >= 2 ? c0 : -1;
    }
    as_count(a.stats + AS_ACCEPTED, accepted);
}

// Largest t in [0, T) with offsets[t] <= m, given offsets[0] <= m.
__device__ __forceinline__ int as_track_of(const int* __restrict__ offsets, int T, int m) {
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= m) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(AS_BLOCK) void as_union_kernel(AsArgs a) {
    const long long x = (long long)blockIdx.x * AS_BLOCK + threadIdx.x;
    if (x < a.n_meas) {
        const int m = (int)x;
        const int T = as_tracks_in_use(a);
        if (T <= 0 || (a.inlier && !a.inlier[m]) || a.offsets[0] > m) return;
        const int t = as_track_of(a.offsets, T, m);
        if (m >= a.offsets[t + 1]) return;  // in the gap after the last track in use, or the offsets do not ascend
        const int c0 = a.tfirst[t], c = a.img[m];
        if (c0 < 0 || (unsigned)c >= (unsigned)a.n_img) return;
        a.isnode[c] = 1;  // every writer stores the same value
        uf_unite(a.parent, c, c0);
        return;
    }
    const long long e = x - a.n_meas;
    if (e >= a.n_extra) return;
    const int u = a.extra[2 * e], v = a.extra[2 * e + 1];
    if (!as_cam_ok(a, u) || !as_cam_ok(a, v)) return;
    a.isnode[u] = 1;
    a.isnode[v] = 1;
    uf_unite(a.parent, u, v);
}

__global__ __launch_bounds__(AS_BLOCK) void as_root_kernel(AsArgs a) {
    const int i = blockIdx.x * AS_BLOCK + threadIdx.x;
    if (i >= a.n_img) return;
    int r = -1;
    if (a.isnode[i]) {
        r = i;
        for (int p = a.parent[r]; p != r; p = a.parent[r]) r = p;  // parent[x] < x off the root: strictly descends
        atomicAdd(a.size + r, 1);
    }
    a.root[i] = r;
}

__global__ __launch_bounds__(AS_BLOCK) void as_first_kernel(AsArgs a) {
    const long long x = (long long)blockIdx.x * AS_BLOCK + threadIdx.x;
    if (x < a.n_tracks) {
        if (x >= as_tracks_in_use(a)) return;
        const int c0 = a.tfirst[x];
        const int r = c0 >= 0 ? a.root[c0] : -1;  // -1 only when the offsets do not ascend: no lane united c0
        if (r >= 0) atomicMin(a.first + r, (int)x);
        return;
    }
    const long long e = x - a.n_tracks;
    if (e >= a.n_extra) return;
    const int u = a.extra[2 * e], v = a.extra[2 * e + 1];
    if (!as_cam_ok(a, u) || !as_cam_ok(a, v)) return;
    const int r = a.root[u];
    if (r >= 0) atomicMin(a.first + r, (int)x);  // x = n_tracks + e
}

// One workgroup. The key of a root packs (size, ~first): the largest key is the component with the most cameras and,
// among equals, the smallest first item. No two roots share a first item, so the maximum is unique.
__global__ __launch_bounds__(AS_BLOCK) void as_select_kernel(AsArgs a) {
    __shared__ u64 sh_key[AS_BLOCK / 64];
    __shared__ int sh_root[AS_BLOCK / 64];
    __shared__ unsigned sh_cnt[AS_BLOCK / 64];
    u64 key = 0;
    int best = -1;
    unsigned cnt = 0;
    for (int i = threadIdx.x; i < a.n_img; i += AS_BLOCK) {
        if (a.root[i] != i) continue;
        ++cnt;
        const u64 k = ((u64)(unsigned)a.size[i] << 32) | (u64)(0x7fffffffu - (unsigned)a.first[i]);
        if (k > key) {
            key = k;
            best = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 k2 = __shfl_xor(key, o, 64);
        const int b2 = __shfl_xor(best, o, 64);
        cnt += __shfl_xor(cnt, o, 64);
        if (k2 > key) {
            key = k2;
            best = b2;
        }
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        sh_key[w] = key;
        sh_root[w] = best;
        sh_cnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int i = 1; i < AS_BLOCK / 64; ++i) {
        cnt += sh_cnt[i];
        if (sh_key[i] > key) {
            key = sh_key[i];
            best = sh_root[i];
        }
    }
    a.winner[0] = best;
    a.stats[AS_COMPONENTS] = cnt;
}

__global__ __launch_bounds__(AS_BLOCK) void as_cameras_kernel(AsArgs a) {
    const int i = blockIdx.x * AS_BLOCK + threadIdx.x;
    bool valid = false, keep = false;
    if (i < a.n_img) {
        valid = !a.cam_valid || a.cam_valid[i];
        const int r = a.root[i];
        keep = valid && r >= 0 && r == a.winner[0];
        a.cam_keep[i] = keep;
    }
    as_count(a.stats + AS_CAMS_VALID, valid);
    as_count(a.stats + AS_CAMS_KEPT, keep);
}

__global__ __launch_bounds__(AS_BLOCK) void as_tracks_kernel(AsArgs a) {
    const int t = blockIdx.x * AS_BLOCK + threadIdx.x;
    int len = 0;
    bool keep = false;
    if (t < a.n_tracks) {
        // no component at all: the reference returns an empty scene (gtsfm_data.py:265-266)
        if (t < as_tracks_in_use(a) && a.tlen[t] >= 0 && a.winner[0] >= 0) {
            keep = true;
            const int hi = a.offsets[t + 1];  // an accepted track's range lies inside [0, n_meas]
            for (int m = a.offsets[t]; m < hi && keep; ++m) {
                if (a.inlier && !a.inlier[m]) continue;
                const int c = a.img[m];
                keep = (unsigned)c < (unsigned)a.n_img && a.cam_keep[c];
            }
            if (keep) len = a.tlen[t];
        }
        a.track_keep[t] = keep;
        a.track_len[t] = len;
    }
    as_count(a.stats + AS_TRACKS_KEPT, keep);
    u64 n = (u64)len;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(a.stats + AS_MEAS_KEPT, n);
}

}  // namespace

extern "C" {

size_t gtsfm_assemble_ba_input_workspace_bytes(long long n_tracks, int n_img) {
    if (n_tracks <= 0 || n_img <= 0 || !as_sizes_ok(n_tracks, 0, n_img, 0)) return 0;
    return as_layout((size_t)n_tracks, (size_t)n_img).total;
}

int gtsfm_assemble_ba_input(const int* d_track_offsets, const int* d_track_img, long long n_tracks,
                            const long long* d_n_tracks, long long n_meas, const uint8_t* d_track_valid,
                            const uint8_t* d_meas_inlier, const uint8_t* d_cam_valid, int n_img,
                            const int* d_extra_edges, int n_extra, void* d_workspace, size_t workspace_bytes,
                            uint8_t* d_cam_keep, uint8_t* d_track_keep, int* d_track_len, long long* d_stats,
                            void* stream_v) {
    hipStream_t stream = (hipStream_t)stream_v;
    if (!as_sizes_ok(n_tracks, n_meas, n_img, n_extra)) return GTSFM_ERR_ARG;
    if (!d_stats || (n_img > 0 && !d_cam_keep) || (n_tracks > 0 && (!d_track_keep || !d_track_len)))
        return GTSFM_ERR_ARG;
    if (n_tracks == 0 || n_meas == 0 || n_img == 0) {  // nothing to join. Nothing below indexes an input.
        GTSFM_CHECK_HIP(hipMemsetAsync(d_stats, 0, AS_STATS * sizeof(long long), stream));
        if (n_img > 0) GTSFM_CHECK_HIP(hipMemsetAsync(d_cam_keep, 0, (size_t)n_img, stream));
        if (n_tracks > 0) {
            GTSFM_CHECK_HIP(hipMemsetAsync(d_track_keep, 0, (size_t)n_tracks, stream));
            GTSFM_CHECK_HIP(hipMemsetAsync(d_track_len, 0, (size_t)n_tracks * sizeof(int), stream));
        }
        return GTSFM_OK;
    }
    if (!d_track_offsets || !d_track_img || !d_workspace || (n_extra > 0 && !d_extra_edges)) return GTSFM_ERR_ARG;
    const AsLayout L = as_layout((size_t)n_tracks, (size_t)n_img);
    if (workspace_bytes < L.total) return GTSFM_ERR_CAPACITY;

    char* ws = (char*)d_workspace;
    AsArgs a;
    a.offsets = d_track_offsets;
    a.img = d_track_img;
    a.n_tracks_dev = d_n_tracks;
    a.track_valid = d_track_valid;
    a.inlier = d_meas_inlier;
    a.cam_valid = d_cam_valid;
    a.extra = d_extra_edges;
    a.n_tracks = (int)n_tracks;
    a.n_meas = (int)n_meas;
    a.n_img = n_img;
    a.n_extra = n_extra;
    a.parent = (int*)(ws + L.parent);
    a.size = (int*)(ws + L.size);
    a.first = (int*)(ws + L.first);
    a.root = (int*)(ws + L.root);
    a.isnode = (uint8_t*)(ws + L.isnode);
    a.tfirst = (int*)(ws + L.tfirst);
    a.tlen = (int*)(ws + L.tlen);
    a.winner = (int*)(ws + L.winner);
    a.cam_keep = d_cam_keep;
    a.track_keep = d_track_keep;
    a.track_len = d_track_len;
    a.stats = (u64*)d_stats;

    const unsigned cam_blocks = blocks_for((size_t)n_img, AS_BLOCK);
    const unsigned track_blocks = blocks_for((size_t)n_tracks, AS_BLOCK);
    hipLaunchKernelGGL(as_init_kernel, dim3(cam_blocks), dim3(AS_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(as_track_kernel, dim3(track_blocks), dim3(AS_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(as_union_kernel, dim3(blocks_for((size_t)(n_meas + n_extra), AS_BLOCK)), dim3(AS_BLOCK), 0,
                       stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(as_root_kernel, dim3(cam_blocks), dim3(AS_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(as_first_kernel, dim3(blocks_for((size_t)(n_tracks + n_extra), AS_BLOCK)), dim3(AS_BLOCK), 0,
                       stream, a);
    hipLaunchKernelGGL(as_select_kernel, dim3(1), dim3(AS_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(as_cameras_kernel, dim3(cam_blocks), dim3(AS_BLOCK), 0, stream, a);
    hipLaunchKernelGGL(as_tracks_kernel, dim3(track_blocks), dim3(AS_BLOCK), 0, stream, a);
    GTSFM_CHECK_HIP(hipGetLastError());
    return GTSFM_OK;
}

}  // extern "C"
