// Voxel down-sampling of a point cloud: one output point per occupied voxel, the mean of its members (what Open3D's
// voxel_down_sample computes on positions; step 1 of qed-init-pc calls it per frame, per merge and once at the end,
// create_init_pointcloud.py:83-90, :193-194, :260).
//
// Contract (include/qed_splat.h): voxel of a point = floorf(p / v) per axis with a correctly rounded fp32 division
// (the library is built without fast-math); sums in float64, rounded to fp32 once; output in ascending (ix, iy, iz)
// order; the result is a pure function of the input -- no floating-point atomics, every sum is combined in an order
// that depends only on the sorted list's positions.
//
// Launches: (1) per-axis min / max of the voxel indices + count of non-finite points (partials per workgroup),
// (2) one workgroup folds them and decides (span > 2^21 on an axis: refused), (3) 64-bit keys
// (ix - min) << 42 | (iy - min) << 21 | (iz - min) with the row as the value, non-finite rows get the all-ones key,
// (4) qed_sort_pairs (stable: members stay in row order), (5) heads per 64-entry chunk, (6) qed_isect_scan,
// (7) per chunk (one wave): segmented inclusive scan of the gathered points in float64 through the wave's shuffles --
// a voxel that lies inside a chunk is finished there; a chunk's leading and trailing open pieces are stored,
// (8) one wave per voxel that crosses a chunk border adds its pieces in chunk order (lane l takes pieces l, l + 64,
// ... in turn, then a butterfly), so a million points in one voxel cost 256 additions per lane, not a million in a row.
//
// qed_voxel_down_sample_attr is the same pipeline carrying K float attribute columns and a weight per point: kernels (7)
// and (8) are templates over K and sum the 3 + K + 1 columns w x, w a_k, w in the same order (K = 0 is the plain entry
// point, whose arithmetic is untouched: with every weight 1 the products are exact and the weight sum is the count, so the
// positions of the two entry points agree bit for bit).  A row with a non-finite attribute or weight, or a weight <= 0,
// takes the route of a non-finite coordinate: counted in (1), the all-ones key in (3).
#include "qed_common.h"

#include <math.h>

extern "C" int qed_isect_scan(const int32_t* block_sums, int32_t n_blocks, int32_t* block_offsets, int32_t* n_isect,
                              int64_t capacity, int32_t* status, void* stream);

namespace qed {

constexpr int kVoxThreads = 256;
constexpr int kVoxChunk = 64;                       // sorted entries per wave in the reduction
constexpr int kVoxAxisBits = 21;
constexpr unsigned long long kVoxInvalidKey = ~0ull;
constexpr int kVoxMaxGrid = 2048;

// device header at the front of the workspace
struct VoxelHeader {
    float mn[3], mx[3];     // per-axis min / max of floorf(p / v) over the finite points
    int n_sort;             // pairs handed to the sort (n, or 0 when refused)
    int n_valid;            // finite points (0 when refused)
    int scan_status[4];     // qed_isect_scan's status word (the count never exceeds n)
};

struct VoxelWorkspace {
    VoxelHeader* hdr;
    float* part;                            // [kVoxMaxGrid][6] min / max partials
    int* part_bad;                          // [kVoxMaxGrid] non-finite points per workgroup
    unsigned long long *keys, *keys_alt;    // [n]
    int *vals, *vals_alt;                   // [n]
    int *chunk_heads, *chunk_base;          // [n_chunks] heads per chunk, exclusive scan
    int* seg_start;                         // [n + 1] first sorted position of output slot s
    int* span_slot;                         // [n_chunks] the slot whose voxel leaves the chunk open, or -1
    double *first_piece, *last_piece;       // [n_chunks][columns]
    void* sort_ws;
    long long sort_ws_bytes;
    long long total_bytes;
};

static inline long long align256(long long b) { return (b + 255) & ~255ll; }

// summed columns: 3 for positions alone, 3 + K + 1 (positions, attributes, the weight) with K >= 1 attributes
static constexpr int voxel_columns(int K) { return K == 0 ? 3 : 3 + K + 1; }

static VoxelWorkspace voxel_layout(void* base, long long n, int columns = 3) {
    VoxelWorkspace w;
    const long long nc = (n + kVoxChunk - 1) / kVoxChunk;
    char* p = (char*)base;
    long long o = 0;
    auto take = [&](long long bytes) { char* r = p + o; o += align256(bytes); return r; };
    w.hdr = (VoxelHeader*)take(sizeof(VoxelHeader));
    w.part = (float*)take((long long)kVoxMaxGrid * 6 * 4);
    w.part_bad = (int*)take((long long)kVoxMaxGrid * 4);
    w.keys = (unsigned long long*)take(n * 8);
    w.keys_alt = (unsigned long long*)take(n * 8);
    w.vals = (int*)take(n * 4);
    w.vals_alt = (int*)take(n * 4);
    w.chunk_heads = (int*)take(nc * 4);
    w.chunk_base = (int*)take(nc * 4);
    w.seg_start = (int*)take((n + 1) * 4);
    w.span_slot = (int*)take(nc * 4);
    w.first_piece = (double*)take(nc * 8 * columns);
    w.last_piece = (double*)take(nc * 8 * columns);
    w.sort_ws_bytes = qed_sort_workspace_bytes(n);
    w.sort_ws = take(w.sort_ws_bytes);
    w.total_bytes = o;
    return w;
}

// the voxel index of one coordinate, as a float (an integer value, or non-finite); ONE definition: membership is
// part of the contract and every kernel must compute it the same way
__device__ __forceinline__ float voxel_index(float x, float v) { return floorf(x / v); }

// qed_voxel_down_sample_attr: a row takes part only with finite attributes and a finite weight > 0 (attrs == NULL: the
// plain entry point, every row does)
__device__ __forceinline__ bool voxel_row_ok(const float* __restrict__ attrs, int K, const float* __restrict__ weights,
                                             long long i) {
    bool ok = true;
    if (weights != nullptr) { const float w = weights[i]; ok = isfinite(w) && w > 0.f; }
    for (int k = 0; k < K; ++k) ok = ok && isfinite(attrs[i * K + k]);
    return ok;
}

// ---- (1) min / max of the voxel indices ---------------------------------------------------------------------------
__global__ void __launch_bounds__(kVoxThreads)
voxel_minmax_kernel(int n, const float* __restrict__ points, const float* __restrict__ attrs, int K,
                    const float* __restrict__ weights, float v, float* __restrict__ part, int* __restrict__ part_bad) {
    __shared__ float s_m[kVoxThreads / 64][6];
    __shared__ int s_bad[kVoxThreads / 64];
    Bounds3 b;
    for (long long i = (long long)blockIdx.x * kVoxThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kVoxThreads) {
        const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
        float f[3] = {voxel_index(x, v), voxel_index(y, v), voxel_index(z, v)};
        if (!voxel_row_ok(attrs, K, weights, i)) f[0] = __builtin_nanf("");
        bounds3_add(b, f);
    }
    bounds3_block<kVoxThreads>(b, s_m, s_bad);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[6 * blockIdx.x + a] = b.mn[a]; part[6 * blockIdx.x + 3 + a] = b.mx[a]; }
        part_bad[blockIdx.x] = b.bad;
    }
}

// ---- (2) fold the partials, decide -------------------------------------------------------------------------------
// status[0]: 1 = refused (an axis spans more than 2^21 voxels), status[1]: non-finite points dropped,
// status[2]: the widest axis span in voxels (saturated)
__global__ void __launch_bounds__(kVoxThreads)
voxel_fold_kernel(int n, int n_parts, const float* __restrict__ part, const int* __restrict__ part_bad,
                  VoxelHeader* __restrict__ hdr, int* __restrict__ status) {
    __shared__ float s_m[kVoxThreads / 64][6];
    __shared__ int s_bad[kVoxThreads / 64];
    Bounds3 b;
    for (int i = threadIdx.x; i < n_parts; i += kVoxThreads) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.mn[a] = fminf(b.mn[a], part[6 * i + a]); b.mx[a] = fmaxf(b.mx[a], part[6 * i + 3 + a]); }
        b.bad += part_bad[i];
    }
    bounds3_block<kVoxThreads>(b, s_m, s_bad);
    if (threadIdx.x == 0) {
        const int n_valid = n - b.bad;
        double widest = 0.0;
        if (n_valid > 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) widest = fmax(widest, (double)b.mx[a] - (double)b.mn[a] + 1.0);
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) { b.mn[a] = 0.f; b.mx[a] = 0.f; }
        }
        const bool refused = widest > (double)(1 << kVoxAxisBits);
#pragma unroll
        for (int a = 0; a < 3; ++a) { hdr->mn[a] = b.mn[a]; hdr->mx[a] = b.mx[a]; }
        hdr->n_sort = refused ? 0 : n;
        hdr->n_valid = refused ? 0 : n_valid;
        hdr->scan_status[0] = 0;
        status[0] = refused ? 1 : 0;
        status[1] = b.bad;
        status[2] = (int)fmin(widest, 2147483647.0);
        status[3] = 0;
    }
}

// ---- (3) keys --------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kVoxThreads)
voxel_key_kernel(int n, const float* __restrict__ points, const float* __restrict__ attrs, int K,
                 const float* __restrict__ weights, float v, const VoxelHeader* __restrict__ hdr,
                 unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    if (hdr->n_sort == 0) return;
    const long long i = (long long)blockIdx.x * kVoxThreads + threadIdx.x;
    if (i >= n) return;
    const float f[3] = {voxel_index(points[3 * i], v), voxel_index(points[3 * i + 1], v), voxel_index(points[3 * i + 2], v)};
    unsigned long long key = kVoxInvalidKey;
    if (isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]) && voxel_row_ok(attrs, K, weights, i)) {
        // exact: both are integer-valued floats and the difference is below 2^21
        const unsigned long long dx = (unsigned long long)((double)f[0] - (double)hdr->mn[0]);
        const unsigned long long dy = (unsigned long long)((double)f[1] - (double)hdr->mn[1]);
        const unsigned long long dz = (unsigned long long)((double)f[2] - (double)hdr->mn[2]);
        key = (dx << (2 * kVoxAxisBits)) | (dy << kVoxAxisBits) | dz;
    }
    keys[i] = key;
    vals[i] = (int)i;
}

// head of a voxel's run in the sorted list: position i < n_valid whose predecessor has another key
__device__ __forceinline__ bool voxel_head(const unsigned long long* __restrict__ keys, long long i, int n_valid,
                                           unsigned long long& key) {
    if (i >= n_valid) { key = kVoxInvalidKey; return false; }
    key = keys[i];
    return i == 0 || keys[i - 1] != key;
}

// ---- (5) heads per chunk ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kVoxThreads)
voxel_count_kernel(int n_chunks, const unsigned long long* __restrict__ keys, const VoxelHeader* __restrict__ hdr,
                   int* __restrict__ chunk_heads) {
    const int chunk = blockIdx.x * (kVoxThreads / 64) + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    unsigned long long key;
    const bool head = voxel_head(keys, (long long)chunk * kVoxChunk + (threadIdx.x & 63), hdr->n_valid, key);
    const unsigned long long hb = __ballot(head);
    if ((threadIdx.x & 63) == 0) chunk_heads[chunk] = __popcll(hb);
}

// ---- (7), (8): templates over K attribute columns (0: positions alone, the plain entry point) ----------------------------
struct VoxelOut {
    float* points;      // [n,3]
    float* attrs;       // [n,K]  (K >= 1)
    float* weights;     // [n]    (K >= 1)
};

// the sums of one finished voxel -> its row: K == 0 divides by the member count, K >= 1 by the weight sum (the last column)
template <int K>
__device__ __forceinline__ void voxel_store(const double (&s)[voxel_columns(K)], double count, long long slot,
                                            const VoxelOut& out) {
    const double inv = K == 0 ? count : s[voxel_columns(K) - 1];
#pragma unroll
    for (int a = 0; a < 3; ++a) out.points[3 * slot + a] = (float)(s[a] / inv);
    if (K > 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) out.attrs[K * slot + k] = (float)(s[3 + k] / inv);
        out.weights[slot] = (float)inv;
    }
}

// ---- (7) one wave per chunk: segmented scan in float64 ------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(kVoxThreads)
voxel_reduce_kernel(int n_chunks, const float* __restrict__ points, const float* __restrict__ attrs,
                    const float* __restrict__ weights, const unsigned long long* __restrict__ keys,
                    const int* __restrict__ vals, const VoxelHeader* __restrict__ hdr, const int* __restrict__ chunk_base,
                    int* __restrict__ seg_start, int* __restrict__ span_slot, double* __restrict__ first_piece,
                    double* __restrict__ last_piece, VoxelOut out) {
    constexpr int NC = voxel_columns(K);
    const int chunk = blockIdx.x * (kVoxThreads / 64) + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const int lane = threadIdx.x & 63;
    const int n_valid = hdr->n_valid;
    const long long i = (long long)chunk * kVoxChunk + lane;
    const bool valid = i < n_valid;
    unsigned long long key;
    const bool head = voxel_head(keys, i, n_valid, key);
    const bool tail = valid && (i + 1 >= n_valid || keys[i + 1] != key);
    double s[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) s[a] = 0.0;
    if (valid) {
        const long long row = vals[i];
        s[0] = (double)points[3 * row]; s[1] = (double)points[3 * row + 1]; s[2] = (double)points[3 * row + 2];
        if (K > 0) {
            const double w = weights != nullptr ? (double)weights[row] : 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) s[a] *= w;
#pragma unroll
            for (int k = 0; k < K; ++k) s[3 + k] = w * (double)attrs[K * row + k];
            s[NC - 1] = w;
        }
    }
    const unsigned long long hb = __ballot(head);
    const unsigned long long upto = hb & ((2ull << lane) - 1ull);          // heads at lanes <= mine
    const bool has_head = upto != 0ull;                                    // my piece starts inside this chunk
    const int head_lane = has_head ? 63 - __builtin_clzll(upto) : 0;
    const int d = lane - head_lane;                                        // my distance from the start of my piece
    // after the step with offset o, s covers min(2 o, d + 1) entries ending at this lane
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
#pragma unroll
        for (int a = 0; a < NC; ++a) {
            const double t = __shfl_up(s[a], o, 64);
            if (d >= o) s[a] += t;
        }
    }
    const int slot = chunk_base[chunk] + __popcll(upto) - 1;              // (-1 + base: the voxel that began earlier)
    if (head) seg_start[slot] = (int)i;
    const bool last_valid = valid && (lane == 63 || i + 1 >= n_valid);
    if (valid && tail) {
        if (has_head) {                                                     // a voxel wholly inside the chunk
            voxel_store<K>(s, (double)(d + 1), slot, out);
        } else {                                                            // the end of a voxel that began earlier
#pragma unroll
            for (int a = 0; a < NC; ++a) first_piece[NC * (long long)chunk + a] = s[a];
        }
    } else if (last_valid) {                                                // the chunk ends inside a voxel
        if (has_head) {
#pragma unroll
            for (int a = 0; a < NC; ++a) last_piece[NC * (long long)chunk + a] = s[a];
        } else {                                                            // the whole chunk is the middle of one voxel
#pragma unroll
            for (int a = 0; a < NC; ++a) first_piece[NC * (long long)chunk + a] = s[a];
        }
    }
    // the voxel this chunk leaves open, if it began here (one word per chunk, written by lane 0)
    const unsigned long long open = __ballot(last_valid && !tail && has_head);
    const int open_slot = __shfl(slot, open ? __builtin_ctzll(open) : 0, 64);
    if (lane == 0) span_slot[chunk] = open ? open_slot : -1;
}

// ---- (8) one wave per voxel that crosses a chunk border: pieces added in chunk order ------------------------------
template <int K>
__global__ void __launch_bounds__(kVoxThreads)
voxel_span_kernel(int n_chunks, const VoxelHeader* __restrict__ hdr, const int* __restrict__ n_out,
                  const int* __restrict__ seg_start, const int* __restrict__ span_slot,
                  const double* __restrict__ first_piece, const double* __restrict__ last_piece, VoxelOut out) {
    constexpr int NC = voxel_columns(K);
    const int c0 = blockIdx.x * (kVoxThreads / 64) + (threadIdx.x >> 6);
    if (c0 >= n_chunks) return;
    const int slot = span_slot[c0];
    if (slot < 0) return;
    const int lane = threadIdx.x & 63;
    const int n_valid = hdr->n_valid;
    const int begin = seg_start[slot];
    const int end = slot + 1 < n_out[0] ? seg_start[slot + 1] : n_valid;
    const int c1 = (end - 1) / kVoxChunk;
    // piece 0 = the tail of chunk c0; piece j >= 1 = the leading piece of chunk c0 + j (all of it for j < c1 - c0)
    double s[NC];
#pragma unroll
    for (int a = 0; a < NC; ++a) s[a] = 0.0;
    for (int j = lane; j <= c1 - c0; j += 64) {
        const double* p = j == 0 ? last_piece + NC * (long long)c0 : first_piece + NC * (long long)(c0 + j);
#pragma unroll
        for (int a = 0; a < NC; ++a) s[a] += p[a];
    }
#pragma unroll
    for (int a = 0; a < NC; ++a) s[a] = wave_sum_d(s[a]);
    if (lane == 0) voxel_store<K>(s, (double)(end - begin), slot, out);
}

// the launches both entry points share: K == 0 with attrs == weights == NULL is qed_voxel_down_sample
template <int K>
static int voxel_run(const char* who, int n, const float* points, const float* attrs, const float* weights, float voxel_size,
                     const VoxelOut& out, int* n_out, const VoxelWorkspace& w, int* status, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int n_chunks = (n + kVoxChunk - 1) / kVoxChunk;
    const unsigned grid_mm = stream_grid(n, kVoxMaxGrid);
    const unsigned grid_n = (unsigned)(((long long)n + kVoxThreads - 1) / kVoxThreads);
    const unsigned grid_c = (unsigned)((n_chunks + kVoxThreads / 64 - 1) / (kVoxThreads / 64));
    hipLaunchKernelGGL(voxel_minmax_kernel, dim3(grid_mm), dim3(kVoxThreads), 0, st, n, points, attrs, K, weights, voxel_size,
                       w.part, w.part_bad);
    hipLaunchKernelGGL(voxel_fold_kernel, dim3(1), dim3(kVoxThreads), 0, st, n, (int)grid_mm, (const float*)w.part,
                       (const int*)w.part_bad, w.hdr, status);
    hipLaunchKernelGGL(voxel_key_kernel, dim3(grid_n), dim3(kVoxThreads), 0, st, n, points, attrs, K, weights, voxel_size,
                       (const VoxelHeader*)w.hdr, w.keys, w.vals);
    // all 64 bits: 3 x 21 of the voxel + the top bit that sends the dropped rows to the end
    const int side = qed_sort_pairs((uint64_t*)w.keys, w.vals, (uint64_t*)w.keys_alt, w.vals_alt, &w.hdr->n_sort, n, 64,
                                    w.sort_ws, w.sort_ws_bytes, w.hdr->scan_status, stream);
    if (side < 0) return side;
    const unsigned long long* keys = side ? w.keys_alt : w.keys;
    const int* vals = side ? w.vals_alt : w.vals;
    hipLaunchKernelGGL(voxel_count_kernel, dim3(grid_c), dim3(kVoxThreads), 0, st, n_chunks, keys,
                       (const VoxelHeader*)w.hdr, w.chunk_heads);
    const int rc = qed_isect_scan(w.chunk_heads, n_chunks, w.chunk_base, n_out, n, w.hdr->scan_status, stream);
    if (rc != QED_OK) return rc;
    hipLaunchKernelGGL(voxel_reduce_kernel<K>, dim3(grid_c), dim3(kVoxThreads), 0, st, n_chunks, points, attrs, weights, keys,
                       vals, (const VoxelHeader*)w.hdr, (const int*)w.chunk_base, w.seg_start, w.span_slot, w.first_piece,
                       w.last_piece, out);
    hipLaunchKernelGGL(voxel_span_kernel<K>, dim3(grid_c), dim3(kVoxThreads), 0, st, n_chunks, (const VoxelHeader*)w.hdr,
                       (const int*)n_out, (const int*)w.seg_start, (const int*)w.span_slot, (const double*)w.first_piece,
                       (const double*)w.last_piece, out);
    return check_launch(who);
}

static int voxel_zero_outputs(const char* who, int32_t* n_out, int32_t* status, hipStream_t st) {
    if (hipMemsetAsync(n_out, 0, sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(status, 0, QED_STATUS_WORDS * sizeof(int32_t), st) != hipSuccess) {
        set_error("%s: memset failed", who);
        return QED_E_LAUNCH;
    }
    return QED_OK;
}

}  // namespace qed

using namespace qed;

extern "C" int64_t qed_voxel_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (1ll << 30)) return QED_E_INVALID_ARG;
    return voxel_layout(nullptr, n > 0 ? n : 1).total_bytes;
}

extern "C" int qed_voxel_down_sample(int32_t n, const float* points, float voxel_size, float* out_points,
                                     int32_t* n_out, void* workspace, int64_t workspace_bytes, int32_t* status,
                                     void* stream) {
    QED_REQUIRE(n >= 0 && n < (1 << 30), "n out of range");
    QED_REQUIRE(isfinite(voxel_size) && voxel_size > 0.f, "voxel_size must be finite and > 0");
    QED_REQUIRE(n_out && status, "null buffers");
    if (n == 0) return voxel_zero_outputs("qed_voxel_down_sample", n_out, status, (hipStream_t)stream);
    QED_REQUIRE(points && out_points && workspace, "null buffers");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    const VoxelWorkspace w = voxel_layout(workspace, n);
    if (workspace_bytes < w.total_bytes) {
        set_error("qed_voxel_down_sample: workspace too small (%lld < %lld)", (long long)workspace_bytes, w.total_bytes);
        return QED_E_WORKSPACE;
    }
    const VoxelOut out = {out_points, nullptr, nullptr};
    return voxel_run<0>("qed_voxel_down_sample", n, points, nullptr, nullptr, voxel_size, out, n_out, w, status, stream);
}

extern "C" int64_t qed_voxel_attr_workspace_bytes(int64_t n, int32_t n_attrs) {
    if (n < 0 || n >= (1ll << 30) || n_attrs < 1 || n_attrs > QED_VOXEL_MAX_ATTRS) return QED_E_INVALID_ARG;
    return voxel_layout(nullptr, n > 0 ? n : 1, voxel_columns(n_attrs)).total_bytes;
}

extern "C" int qed_voxel_down_sample_attr(int32_t n, const float* points, int32_t n_attrs, const float* attrs,
                                          const float* weights, float voxel_size, float* out_points, float* out_attrs,
                                          float* out_weights, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                                          int32_t* status, void* stream) {
    QED_REQUIRE(n >= 0 && n < (1 << 30), "n out of range");
    QED_REQUIRE(n_attrs >= 1 && n_attrs <= QED_VOXEL_MAX_ATTRS, "n_attrs must be 1 to 8");
    QED_REQUIRE(isfinite(voxel_size) && voxel_size > 0.f, "voxel_size must be finite and > 0");
    QED_REQUIRE(n_out && status, "null buffers");
    if (n == 0) return voxel_zero_outputs("qed_voxel_down_sample_attr", n_out, status, (hipStream_t)stream);
    QED_REQUIRE(points && attrs && out_points && out_attrs && out_weights && workspace, "null buffers");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    const VoxelWorkspace w = voxel_layout(workspace, n, voxel_columns(n_attrs));
    if (workspace_bytes < w.total_bytes) {
        set_error("qed_voxel_down_sample_attr: workspace too small (%lld < %lld)", (long long)workspace_bytes, w.total_bytes);
        return QED_E_WORKSPACE;
    }
    const VoxelOut out = {out_points, out_attrs, out_weights};
    const char* who = "qed_voxel_down_sample_attr";
    switch (n_attrs) {
        case 1: return voxel_run<1>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        case 2: return voxel_run<2>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        case 3: return voxel_run<3>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        case 4: return voxel_run<4>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        case 5: return voxel_run<5>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        case 6: return voxel_run<6>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        case 7: return voxel_run<7>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
        default: return voxel_run<8>(who, n, points, attrs, weights, voxel_size, out, n_out, w, status, stream);
    }
}
