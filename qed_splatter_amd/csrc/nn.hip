// Exact nearest-neighbour distances between two point clouds, and the two reductions the reference's PDMetrics needs
// (metrics.py:9-63: cKDTree over one cloud, queried with the other; accuracy = a percentile of the distances,
// completeness = the share of distances under a threshold).
//
// Index over the TARGET cloud (qed_nn_build): a uniform grid, stored sparsely.  Cell of a point = trunc((p - mn) / h)
// per axis (mn = the cloud's per-axis minimum), 21 bits per axis in one 64-bit key, sorted with qed_sort_pairs (stable:
// the rows of a cell stay in row order), then compacted into the list of OCCUPIED cells (key + first sorted position)
// and the points in sorted order (x, y, z, row).  Cells are found by binary search over the sorted unique keys, not by
// a hash table: the keys come out of the sort for nothing, the z neighbours of a cell are its neighbours in the list
// (one search finds a whole run of cells along z, the rest is a linear walk), there is no table to size, and nothing
// in the build depends on the order in which workgroups arrive.  A dense grid is out of the question: clouds are
// surfaces, 2^21 cells per axis.  The cell size is given, or chosen here from the data without a host round trip:
// a first build at max extent / 1024 counts the occupied cells, then h is scaled by sqrt(4 / occupancy) (a surface's
// occupancy grows with h^2) and the build is repeated.  A cell size that would need more than 2^20 cells on an axis
// is enlarged: the build never refuses a finite cloud.
//
// Grid query (qed_nn_query): one lane per query, queries taken in the order of their (clamped) cell in the target's
// grid so that the lanes of a wave walk the same cells.  Shells of growing Chebyshev radius r around the query's cell,
// clipped to the index's bounds; after shell r every unvisited point lies beyond the faces of the visited box, so the
// search stops as soon as the best squared distance is below the squared distance to the nearest face that still has
// cells behind it (computed with a margin that covers the fp32 rounding of the cell coordinates: the margin can only
// cost a shell, never an answer).  A query still open after max_rings shells goes to the fallback list.
//
// Brute force (qed_nn_brute): the rows of a list, or all rows.  Targets tiled through LDS, four queries per lane, the
// target cloud cut into slices over blockIdx.y; the slices meet in a 64-bit integer atomicMin.
//
// ONE definition of the result: nn_dist2 (fp32 differences, one product, two fmas) and the packed candidate
// (bits of d2) << 32 | row, of which the smallest wins -- non-negative floats order like their bit patterns, so that
// is the smallest squared distance and, among equals, the smallest row.  min is associative and commutative: both
// paths return bit-identical (distance, index) whatever the cell size, max_rings, the slicing or the arrival order.
// No floating-point atomics anywhere.
//
// k nearest neighbours (qed_knn_query, qed_knn_brute): the same index, the same walk and the same two paths with a sorted
// list of the k smallest packed candidates per query in registers; see the section further down.
#include "qed_common.h"

#include <math.h>

extern "C" int qed_isect_scan(const int32_t* block_sums, int32_t n_blocks, int32_t* block_offsets, int32_t* n_isect,
                              int64_t capacity, int32_t* status, void* stream);

namespace qed {

constexpr int kNnThreads = 256;
constexpr int kNnChunk = 64;                        // sorted entries per wave in the compaction
constexpr int kNnAxisBits = 21;
constexpr int kNnMaxGrid = 2048;
constexpr int kNnMaxRings = 64;                       // shell r costs ~2 (2 r + 1)^2 look-ups: beyond this the brute force is cheaper
constexpr float kNnAutoCells = 1024.f;              // first guess of the automatic cell size: max extent / 1024
constexpr float kNnAutoOccupancy = 4.f;             // points per occupied cell the automatic cell size aims at
constexpr int kBruteTile = 1024;                    // targets per LDS tile (16 KiB)
constexpr int kBruteQ = 4;                          // queries per lane
constexpr int kBruteMaxSlices = 64;
constexpr int kBruteMaxGridX = 512;
constexpr unsigned long long kNnNone = ~0ull;

struct NnHeader {
    float mn[3];            // per-axis minimum of the finite target points
    float ext[3];           // per-axis extent
    float max_ext;
    float h, inv_h;         // cell size in use and its reciprocal
    float slop;             // absolute margin of the face distances
    int dims[3];            // cells per axis, 1 .. 2^21
    int n_sort;             // pairs handed to the sort
    int n_cells;            // occupied cells
    int scan_status[4];
};

struct NnWorkspace {
    NnHeader* hdr;
    float* part;                            // [kNnMaxGrid][6]
    int* part_bad;                          // [kNnMaxGrid]
    unsigned long long *keys, *keys_alt;    // [nt]
    int *vals, *vals_alt;                   // [nt]
    int *chunk_heads, *chunk_base;          // [n_chunks]
    unsigned long long* cell_key;           // [nt] keys of the occupied cells, ascending
    int* cell_start;                        // [nt + 1] first sorted position of each occupied cell, then nt
    float4* sorted_pts;                     // [nt] x, y, z, row (bits) in sorted order
    void* sort_ws;
    long long sort_ws_bytes;
    // query side
    int* q_n;                               // [4] device copy of n_query (the sort's n_dev) + the sort's status
    unsigned long long *qkeys, *qkeys_alt;  // [nq]
    int *qvals, *qvals_alt;                 // [nq]
    void* qsort_ws;
    long long qsort_ws_bytes;
    long long total_bytes;
};

static inline long long nn_align(long long b) { return (b + 255) & ~255ll; }

static NnWorkspace nn_layout(void* base, long long nt, long long nq) {
    NnWorkspace w;
    nt = nt > 0 ? nt : 1;
    nq = nq > 0 ? nq : 1;
    const long long nc = (nt + kNnChunk - 1) / kNnChunk;
    char* p = (char*)base;
    long long o = 0;
    auto take = [&](long long bytes) { char* r = p + o; o += nn_align(bytes); return r; };
    w.hdr = (NnHeader*)take(sizeof(NnHeader));
    w.part = (float*)take((long long)kNnMaxGrid * 6 * 4);
    w.part_bad = (int*)take((long long)kNnMaxGrid * 4);
    w.keys = (unsigned long long*)take(nt * 8);
    w.keys_alt = (unsigned long long*)take(nt * 8);
    w.vals = (int*)take(nt * 4);
    w.vals_alt = (int*)take(nt * 4);
    w.chunk_heads = (int*)take(nc * 4);
    w.chunk_base = (int*)take(nc * 4);
    w.cell_key = (unsigned long long*)take(nt * 8);
    w.cell_start = (int*)take((nt + 1) * 4);
    w.sorted_pts = (float4*)take(nt * 16);
    w.sort_ws_bytes = qed_sort_workspace_bytes(nt);
    w.sort_ws = take(w.sort_ws_bytes);
    w.q_n = (int*)take(8 * 4);
    w.qkeys = (unsigned long long*)take(nq * 8);
    w.qkeys_alt = (unsigned long long*)take(nq * 8);
    w.qvals = (int*)take(nq * 4);
    w.qvals_alt = (int*)take(nq * 4);
    w.qsort_ws_bytes = qed_sort_workspace_bytes(nq);
    w.qsort_ws = take(w.qsort_ws_bytes);
    w.total_bytes = o;
    return w;
}

// ---- the one definition of the distance and of the winner ------------------------------------------------------------
__device__ __forceinline__ float nn_dist2(float qx, float qy, float qz, float tx, float ty, float tz) {
    const float dx = tx - qx, dy = ty - qy, dz = tz - qz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
__device__ __forceinline__ unsigned long long nn_pack(float d2, int row) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)row;
}
__device__ __forceinline__ float nn_unpack_dist(unsigned long long b) { return sqrtf(__uint_as_float((unsigned)(b >> 32))); }
__device__ __forceinline__ int nn_unpack_row(unsigned long long b) { return (int)(unsigned)(b & 0xffffffffull); }

// ---- the one definition of a point's cell ----------------------------------------------------------------------------
// u is a monotone function of x (a subtraction, then a product with a positive number); the termination test of the
// grid query relies on that and on nothing finer.  The clamp keeps every index inside the grid whatever x is.
__device__ __forceinline__ float nn_cell_coord(float x, float mn, float inv_h) { return (x - mn) * inv_h; }
__device__ __forceinline__ int nn_cell_clamp(float u, int dim) { return (int)fminf(fmaxf(u, 0.f), (float)(dim - 1)); }
__device__ __forceinline__ unsigned long long nn_key(int cx, int cy, int cz) {
    return ((unsigned long long)cx << (2 * kNnAxisBits)) | ((unsigned long long)cy << kNnAxisBits) | (unsigned long long)cz;
}

// ---- (1) per-axis min / max of the finite points ---------------------------------------------------------------------
__global__ void __launch_bounds__(kNnThreads)
nn_minmax_kernel(int n, const float* __restrict__ points, float* __restrict__ part, int* __restrict__ part_bad) {
    __shared__ float s_m[kNnThreads / 64][6];
    __shared__ int s_bad[kNnThreads / 64];
    Bounds3 b;
    for (long long i = (long long)blockIdx.x * kNnThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kNnThreads) {
        const float f[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        bounds3_add(b, f);
    }
    bounds3_block<kNnThreads>(b, s_m, s_bad);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[6 * blockIdx.x + a] = b.mn[a]; part[6 * blockIdx.x + 3 + a] = b.mx[a]; }
        part_bad[blockIdx.x] = b.bad;
    }
}

// the cell size in use, the grid's dimensions and the margin, from the bounds and a wanted cell size
__device__ __forceinline__ void nn_set_cell(NnHeader* hdr, float h) {
    const float h_min = hdr->max_ext * (1.0001f / (float)(1 << (kNnAxisBits - 1)));     // at most 2^20 cells on an axis
    if (!(h >= h_min)) h = h_min;
    if (!(h > 0.f)) h = 1.f;                                                            // (a cloud of one position)
    hdr->h = h;
    hdr->inv_h = 1.f / h;
    hdr->slop = 2e-6f * (hdr->max_ext + h);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float cells = hdr->ext[a] * hdr->inv_h;                                   // = the cell coordinate of the maximum
        hdr->dims[a] = cells >= 0.f ? min((int)fminf(cells, 4e6f) + 1, 1 << kNnAxisBits) : 1;
    }
}

// ---- (2) fold the partials; the first cell size -----------------------------------------------------------------------
// status[0]: 0; status[1]: points with a non-finite coordinate (the caller must not pass any: their results are
// unspecified, though every access stays in bounds)
__global__ void __launch_bounds__(kNnThreads)
nn_fold_kernel(int n, int n_parts, const float* __restrict__ part, const int* __restrict__ part_bad, float cell_size,
               NnHeader* __restrict__ hdr, int* __restrict__ status) {
    __shared__ float s_m[kNnThreads / 64][6];
    __shared__ int s_bad[kNnThreads / 64];
    Bounds3 b;
    for (int i = threadIdx.x; i < n_parts; i += kNnThreads) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.mn[a] = fminf(b.mn[a], part[6 * i + a]); b.mx[a] = fmaxf(b.mx[a], part[6 * i + 3 + a]); }
        b.bad += part_bad[i];
    }
    bounds3_block<kNnThreads>(b, s_m, s_bad);
    if (threadIdx.x == 0) {
        float max_ext = 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (b.bad == n) { b.mn[a] = 0.f; b.mx[a] = 0.f; }
            hdr->mn[a] = b.mn[a];
            hdr->ext[a] = b.mx[a] - b.mn[a];
            max_ext = fmaxf(max_ext, hdr->ext[a]);
        }
        hdr->max_ext = max_ext;
        nn_set_cell(hdr, cell_size > 0.f ? cell_size : max_ext / kNnAutoCells);
        hdr->n_sort = n;
        hdr->n_cells = 0;
        hdr->scan_status[0] = 0;
        status[0] = 0;
        status[1] = b.bad;
        status[2] = 0;
        status[3] = 0;
    }
}

// ---- (3) keys of the target points, or of the queries (clamped into the target's grid) --------------------------------
__global__ void __launch_bounds__(kNnThreads)
nn_key_kernel(int n, const float* __restrict__ points, const NnHeader* __restrict__ hdr,
              unsigned long long* __restrict__ keys, int* __restrict__ vals, int* __restrict__ n_dev) {
    const long long i = (long long)blockIdx.x * kNnThreads + threadIdx.x;
    if (i == 0 && n_dev) n_dev[0] = n;
    if (i >= n) return;
    const float inv_h = hdr->inv_h;
    const int cx = nn_cell_clamp(nn_cell_coord(points[3 * i], hdr->mn[0], inv_h), hdr->dims[0]);
    const int cy = nn_cell_clamp(nn_cell_coord(points[3 * i + 1], hdr->mn[1], inv_h), hdr->dims[1]);
    const int cz = nn_cell_clamp(nn_cell_coord(points[3 * i + 2], hdr->mn[2], inv_h), hdr->dims[2]);
    keys[i] = nn_key(cx, cy, cz);
    vals[i] = (int)i;
}

// ---- (5) heads per 64-entry chunk of the sorted list ------------------------------------------------------------------
__global__ void __launch_bounds__(kNnThreads)
nn_count_kernel(int n, int n_chunks, const unsigned long long* __restrict__ keys, int* __restrict__ chunk_heads) {
    const int chunk = blockIdx.x * (kNnThreads / 64) + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const long long i = (long long)chunk * kNnChunk + (threadIdx.x & 63);
    const bool head = i < n && (i == 0 || keys[i - 1] != keys[i]);
    const unsigned long long hb = __ballot(head);
    if ((threadIdx.x & 63) == 0) chunk_heads[chunk] = __popcll(hb);
}

// ---- (7) the occupied cells and the points in sorted order ------------------------------------------------------------
__global__ void __launch_bounds__(kNnThreads)
nn_compact_kernel(int n, int n_chunks, const float* __restrict__ points, const unsigned long long* __restrict__ keys,
                  const int* __restrict__ vals, const int* __restrict__ chunk_base,
                  unsigned long long* __restrict__ cell_key, int* __restrict__ cell_start, float4* __restrict__ sorted_pts) {
    const int chunk = blockIdx.x * (kNnThreads / 64) + (threadIdx.x >> 6);
    if (chunk >= n_chunks) return;
    const int lane = threadIdx.x & 63;
    const long long i = (long long)chunk * kNnChunk + lane;
    const bool valid = i < n;
    const unsigned long long key = valid ? keys[i] : kNnNone;
    const bool head = valid && (i == 0 || keys[i - 1] != key);
    const unsigned long long hb = __ballot(head);
    if (!valid) return;
    const int slot = chunk_base[chunk] + __popcll(hb & ((2ull << lane) - 1ull)) - 1;     // the cell this entry belongs to
    if (head) { cell_key[slot] = key; cell_start[slot] = (int)i; }
    if (i == n - 1) cell_start[slot + 1] = n;                                           // slot + 1 = the number of cells
    const int row = vals[i];
    sorted_pts[i] = make_float4(points[3 * (long long)row], points[3 * (long long)row + 1], points[3 * (long long)row + 2],
                                __int_as_float(row));
}

// ---- (8) automatic cell size: scale the first guess by the occupancy it gave ------------------------------------------
__global__ void nn_refine_kernel(int n, NnHeader* __restrict__ hdr) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const float occupancy = (float)n / (float)max(hdr->n_cells, 1);
    nn_set_cell(hdr, hdr->h * sqrtf(kNnAutoOccupancy / occupancy));
    hdr->scan_status[0] = 0;
}

// ---- grid query ---------------------------------------------------------------------------------------------------
// first occupied cell whose key is >= key
__device__ __forceinline__ int nn_lower_bound(const unsigned long long* __restrict__ cell_key, int n_cells, unsigned long long key) {
    int lo = 0, hi = n_cells;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cell_key[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the cells (x, y, za .. zb): neighbours in the list of occupied cells
__device__ __forceinline__ void nn_visit_run(int x, int y, int za, int zb, float qx, float qy, float qz, int n_cells,
                                             const unsigned long long* __restrict__ cell_key, const int* __restrict__ cell_start,
                                             const float4* __restrict__ sorted_pts, unsigned long long& best) {
    const unsigned long long klo = nn_key(x, y, za), khi = nn_key(x, y, zb);
    int j = nn_lower_bound(cell_key, n_cells, klo);
    if (j >= n_cells || cell_key[j] > khi) return;
    const int p0 = cell_start[j];
    ++j;
    while (j < n_cells && cell_key[j] <= khi) ++j;               // at most zb - za further cells
    const int p1 = cell_start[j];
    for (int p = p0; p < p1; ++p) {
        const float4 t = sorted_pts[p];
        const unsigned long long cand = nn_pack(nn_dist2(qx, qy, qz, t.x, t.y, t.z), __float_as_int(t.w));
        best = cand < best ? cand : best;
    }
}

__global__ void __launch_bounds__(kNnThreads)
nn_grid_query_kernel(int nq, const float* __restrict__ query, const int* __restrict__ perm, const NnHeader* __restrict__ hdr,
                     const unsigned long long* __restrict__ cell_key, const int* __restrict__ cell_start,
                     const float4* __restrict__ sorted_pts, int max_rings, float* __restrict__ dist, int* __restrict__ idx,
                     int* __restrict__ fallback) {
    const long long i = (long long)blockIdx.x * kNnThreads + threadIdx.x;
    if (i >= nq) return;
    int row = perm ? perm[i] : (int)i;
    row = min(max(row, 0), nq - 1);
    const float q[3] = {query[3 * (long long)row], query[3 * (long long)row + 1], query[3 * (long long)row + 2]};
    const int n_cells = hdr->n_cells;
    const float h = hdr->h, inv_h = hdr->inv_h, slop = hdr->slop;
    const int dims[3] = {hdr->dims[0], hdr->dims[1], hdr->dims[2]};
    float u[3];
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = nn_cell_coord(q[a], hdr->mn[a], inv_h);
        c[a] = nn_cell_clamp(u[a], dims[a]);
    }
    unsigned long long best = kNnNone;
    bool done = false;
    for (int r = 0; r < max_rings && !done; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, dims[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, dims[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, dims[2] - 1);
        const int zl = c[2] - r, zh = c[2] + r;
        for (int x = x0; x <= x1; ++x) {
            const bool xb = x - c[0] == r || c[0] - x == r;
            for (int y = y0; y <= y1; ++y) {
                if (xb || y - c[1] == r || c[1] - y == r) {                    // a column of the shell's wall
                    nn_visit_run(x, y, z0, z1, q[0], q[1], q[2], n_cells, cell_key, cell_start, sorted_pts, best);
                } else {                                                       // the two caps (r >= 1 here)
                    if (zl >= 0) nn_visit_run(x, y, zl, zl, q[0], q[1], q[2], n_cells, cell_key, cell_start, sorted_pts, best);
                    if (zh < dims[2]) nn_visit_run(x, y, zh, zh, q[0], q[1], q[2], n_cells, cell_key, cell_start, sorted_pts, best);
                }
            }
        }
        // the visited box is cells [c - r, c + r]: unvisited points have a cell coordinate < c - r or >= c + r + 1
        bool covered = true;
        float lb = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int lo = c[a] - r, hi = c[a] + r + 1;
            if (lo > 0) { covered = false; lb = fminf(lb, fmaxf((u[a] - (float)lo) * h * (1.f - 1e-5f) - slop, 0.f)); }
            if (hi < dims[a]) { covered = false; lb = fminf(lb, fmaxf(((float)hi - u[a]) * h * (1.f - 1e-5f) - slop, 0.f)); }
        }
        done = best != kNnNone && (covered || __uint_as_float((unsigned)(best >> 32)) < lb * lb);
    }
    if (done) {
        dist[row] = nn_unpack_dist(best);
        idx[row] = nn_unpack_row(best);
    } else {
        const int slot = atomicAdd(&fallback[0], 1);                          // (integer: the list's order is arbitrary,
        if (slot < nq) fallback[1 + slot] = row;                              // the results do not depend on it)
    }
}

// ---- brute force --------------------------------------------------------------------------------------------------
// rows: NULL = all n_query rows, or rows[0] = count (device), rows[1 ..] = row ids
__global__ void __launch_bounds__(kNnThreads)
nn_brute_kernel(int nq, const float* __restrict__ query, int nt, const float* __restrict__ target,
                const int* __restrict__ rows, int per_slice, unsigned long long* __restrict__ best) {
    __shared__ float4 tile[kBruteTile];
    const int count = rows ? min(max(rows[0], 0), nq) : nq;
    const long long t_begin = (long long)blockIdx.y * per_slice;
    const long long t_end = t_begin + per_slice < nt ? t_begin + per_slice : nt;
    if (t_begin >= t_end) return;
    constexpr int kPerBlock = kNnThreads * kBruteQ;
    for (long long base = (long long)blockIdx.x * kPerBlock; base < count; base += (long long)gridDim.x * kPerBlock) {
        float q[kBruteQ][3];
        int row[kBruteQ];
        unsigned bd[kBruteQ];
        int bi[kBruteQ];
#pragma unroll
        for (int k = 0; k < kBruteQ; ++k) {
            const long long qi = base + k * kNnThreads + threadIdx.x;
            row[k] = -1;
            if (qi < count) row[k] = rows ? min(max(rows[1 + qi], 0), nq - 1) : (int)qi;
            const long long r = row[k] >= 0 ? row[k] : 0;
            q[k][0] = query[3 * r]; q[k][1] = query[3 * r + 1]; q[k][2] = query[3 * r + 2];
            bd[k] = 0xffffffffu;
            bi[k] = 0;
        }
        for (long long t0 = t_begin; t0 < t_end; t0 += kBruteTile) {
            const int cnt = (int)(t_end - t0 < kBruteTile ? t_end - t0 : kBruteTile);
            __syncthreads();
            for (int j = threadIdx.x; j < cnt; j += kNnThreads)
                tile[j] = make_float4(target[3 * (t0 + j)], target[3 * (t0 + j) + 1], target[3 * (t0 + j) + 2], 0.f);
            __syncthreads();
            for (int j = 0; j < cnt; ++j) {
                const float4 t = tile[j];                                      // one address for the wave: a broadcast
#pragma unroll
                for (int k = 0; k < kBruteQ; ++k) {
                    const unsigned d = __float_as_uint(nn_dist2(q[k][0], q[k][1], q[k][2], t.x, t.y, t.z));
                    // rows ascend inside a slice: on equal bits the earlier (smaller) row stays
                    if (d < bd[k]) { bd[k] = d; bi[k] = (int)(t0 + j); }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kBruteQ; ++k)
            if (row[k] >= 0) atomicMin(&best[row[k]], ((unsigned long long)bd[k] << 32) | (unsigned)bi[k]);
    }
}

__global__ void __launch_bounds__(kNnThreads)
nn_finish_kernel(int nq, const int* __restrict__ rows, const unsigned long long* __restrict__ best,
                 float* __restrict__ dist, int* __restrict__ idx) {
    const int count = rows ? min(max(rows[0], 0), nq) : nq;
    for (long long i = (long long)blockIdx.x * kNnThreads + threadIdx.x; i < count; i += (long long)gridDim.x * kNnThreads) {
        const int row = rows ? min(max(rows[1 + i], 0), nq - 1) : (int)i;
        const unsigned long long b = best[row];
        dist[row] = nn_unpack_dist(b);
        idx[row] = nn_unpack_row(b);
    }
}

// ---- k nearest neighbours (qed_knn_query, qed_knn_brute) -----------------------------------------------------------
// The answer of a query is its KK smallest packed candidates in ascending order of the packed word (KK = k, or k + 1
// with QED_KNN_SKIP_FIRST, of which the smallest is then dropped): the k = 1 definition applied KK times.  Both paths
// look at every target at most once, so the list never holds a candidate twice, and "the KK smallest of a set" does not
// depend on the order in which the set is walked or on how it is cut into parts that are merged later.
// The list lives in registers: KK is a template parameter and every index is a compile-time constant.
constexpr int kKnnMaxK = 8;                          // held: up to 9 words with QED_KNN_SKIP_FIRST
constexpr int kKnnBruteMaxGrid = 4096;               // workgroups of the brute force (four queries each per round)

// one compare-exchange per slot: the list stays ascending, the largest of the KK + 1 words falls off the end
template <int KK>
__device__ __forceinline__ void knn_insert(unsigned long long (&c)[KK], unsigned long long cand) {
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        const unsigned long long lo = cand < c[j] ? cand : c[j];
        cand = cand < c[j] ? c[j] : cand;
        c[j] = lo;
    }
}

template <int KK>
__device__ __forceinline__ void knn_write(const unsigned long long (&c)[KK], int skip, int k, long long row,
                                          float* __restrict__ dist, int* __restrict__ idx) {
#pragma unroll
    for (int j = 0; j < KK; ++j)
        if (j >= skip) {                                                       // (skip = KK - k: 0 or 1)
            dist[row * k + (j - skip)] = nn_unpack_dist(c[j]);
            idx[row * k + (j - skip)] = nn_unpack_row(c[j]);
        }
}

template <int KK>
__device__ __forceinline__ void knn_visit_run(int x, int y, int za, int zb, float qx, float qy, float qz, int n_cells,
                                              const unsigned long long* __restrict__ cell_key, const int* __restrict__ cell_start,
                                              const float4* __restrict__ sorted_pts, unsigned long long (&c)[KK]) {
    const unsigned long long klo = nn_key(x, y, za), khi = nn_key(x, y, zb);
    int j = nn_lower_bound(cell_key, n_cells, klo);
    if (j >= n_cells || cell_key[j] > khi) return;
    const int p0 = cell_start[j];
    ++j;
    while (j < n_cells && cell_key[j] <= khi) ++j;
    const int p1 = cell_start[j];
    for (int p = p0; p < p1; ++p) {
        const float4 t = sorted_pts[p];
        const unsigned long long cand = nn_pack(nn_dist2(qx, qy, qz, t.x, t.y, t.z), __float_as_int(t.w));
        if (cand < c[KK - 1]) knn_insert<KK>(c, cand);
    }
}

// nn_grid_query_kernel's walk (walls, caps, clipped box, face distance with its margin); a shell's cells are those at
// Chebyshev distance exactly r, so every cell -- every target -- is visited once.  After shell r every unvisited point is
// at least lb away: the list is final once it is full and its LARGEST entry is closer than that.
template <int KK>
__global__ void __launch_bounds__(kNnThreads)
knn_grid_query_kernel(int nq, const float* __restrict__ query, const int* __restrict__ perm, const NnHeader* __restrict__ hdr,
                      const unsigned long long* __restrict__ cell_key, const int* __restrict__ cell_start,
                      const float4* __restrict__ sorted_pts, int max_rings, int k, float* __restrict__ dist,
                      int* __restrict__ idx, int* __restrict__ fallback) {
    const long long i = (long long)blockIdx.x * kNnThreads + threadIdx.x;
    if (i >= nq) return;
    int row = perm ? perm[i] : (int)i;
    row = min(max(row, 0), nq - 1);
    const float q[3] = {query[3 * (long long)row], query[3 * (long long)row + 1], query[3 * (long long)row + 2]};
    const int n_cells = hdr->n_cells;
    const float h = hdr->h, inv_h = hdr->inv_h, slop = hdr->slop;
    const int dims[3] = {hdr->dims[0], hdr->dims[1], hdr->dims[2]};
    float u[3];
    int c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        u[a] = nn_cell_coord(q[a], hdr->mn[a], inv_h);
        c[a] = nn_cell_clamp(u[a], dims[a]);
    }
    unsigned long long best[KK];
#pragma unroll
    for (int j = 0; j < KK; ++j) best[j] = kNnNone;
    bool done = false;
    for (int r = 0; r < max_rings && !done; ++r) {
        const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, dims[0] - 1);
        const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, dims[1] - 1);
        const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, dims[2] - 1);
        const int zl = c[2] - r, zh = c[2] + r;
        for (int x = x0; x <= x1; ++x) {
            const bool xb = x - c[0] == r || c[0] - x == r;
            for (int y = y0; y <= y1; ++y) {
                if (xb || y - c[1] == r || c[1] - y == r) {
                    knn_visit_run<KK>(x, y, z0, z1, q[0], q[1], q[2], n_cells, cell_key, cell_start, sorted_pts, best);
                } else {
                    if (zl >= 0) knn_visit_run<KK>(x, y, zl, zl, q[0], q[1], q[2], n_cells, cell_key, cell_start, sorted_pts, best);
                    if (zh < dims[2]) knn_visit_run<KK>(x, y, zh, zh, q[0], q[1], q[2], n_cells, cell_key, cell_start, sorted_pts, best);
                }
            }
        }
        bool covered = true;
        float lb = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int lo = c[a] - r, hi = c[a] + r + 1;
            if (lo > 0) { covered = false; lb = fminf(lb, fmaxf((u[a] - (float)lo) * h * (1.f - 1e-5f) - slop, 0.f)); }
            if (hi < dims[a]) { covered = false; lb = fminf(lb, fmaxf(((float)hi - u[a]) * h * (1.f - 1e-5f) - slop, 0.f)); }
        }
        done = best[KK - 1] != kNnNone && (covered || __uint_as_float((unsigned)(best[KK - 1] >> 32)) < lb * lb);
    }
    if (done) {
        knn_write<KK>(best, KK - k, k, row, dist, idx);
    } else {
        const int slot = atomicAdd(&fallback[0], 1);
        if (slot < nq) fallback[1 + slot] = row;
    }
}

// Brute force: one WAVE per query.  The target is cut into 64 interleaved slices, one per lane, each with a list of its
// own; the lists meet in a butterfly of 64-bit shuffles (after a step a lane and its partner hold the same list, and
// the next partner's list was built from other targets: still no candidate twice).  The four waves of a workgroup
// share each LDS tile; consecutive lanes read consecutive float4s of it.
template <int KK>
__global__ void __launch_bounds__(kNnThreads)
knn_brute_kernel(int nq, const float* __restrict__ query, int nt, const float* __restrict__ target,
                 const int* __restrict__ rows, int k, float* __restrict__ dist, int* __restrict__ idx) {
    __shared__ float4 tile[kBruteTile];
    const int count = rows ? min(max(rows[0], 0), nq) : nq;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    constexpr int kWaves = kNnThreads / 64;
    for (long long base = (long long)blockIdx.x * kWaves; base < count; base += (long long)gridDim.x * kWaves) {
        const long long qi = base + wid;                                       // (base is the same for the whole workgroup)
        const bool live = qi < count;
        const long long row = live ? (rows ? min(max(rows[1 + qi], 0), nq - 1) : (int)qi) : 0;
        const float qx = query[3 * row], qy = query[3 * row + 1], qz = query[3 * row + 2];
        unsigned long long c[KK];
#pragma unroll
        for (int j = 0; j < KK; ++j) c[j] = kNnNone;
        for (long long t0 = 0; t0 < nt; t0 += kBruteTile) {
            const int cnt = (int)(nt - t0 < kBruteTile ? nt - t0 : kBruteTile);
            __syncthreads();
            for (int j = threadIdx.x; j < cnt; j += kNnThreads)
                tile[j] = make_float4(target[3 * (t0 + j)], target[3 * (t0 + j) + 1], target[3 * (t0 + j) + 2], 0.f);
            __syncthreads();
            for (int j = lane; j < cnt; j += 64) {
                const float4 t = tile[j];
                const unsigned long long cand = nn_pack(nn_dist2(qx, qy, qz, t.x, t.y, t.z), (int)(t0 + j));
                if (cand < c[KK - 1]) knn_insert<KK>(c, cand);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            unsigned long long other[KK];
#pragma unroll
            for (int j = 0; j < KK; ++j) other[j] = __shfl_xor(c[j], o, 64);
#pragma unroll
            for (int j = 0; j < KK; ++j) knn_insert<KK>(c, other[j]);
        }
        if (live && lane == 0) knn_write<KK>(c, KK - k, k, row, dist, idx);
    }
}

// ---- PDMetrics' reductions ----------------------------------------------------------------------------------------
// keys = the distances' bits (non-negative floats order like their bit patterns); count of distances under the threshold,
// compared in float64 as the reference compares its float64 distances
__global__ void __launch_bounds__(kNnThreads)
pd_prepare_kernel(int n, const float* __restrict__ dist, double threshold, unsigned long long* __restrict__ keys,
                  int* __restrict__ vals, int* __restrict__ n_dev, unsigned long long* __restrict__ count) {
    int under = 0;
    for (long long i = (long long)blockIdx.x * kNnThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kNnThreads) {
        const float d = dist[i];
        keys[i] = (unsigned long long)__float_as_uint(d);
        vals[i] = (int)i;
        under += (double)d < threshold ? 1 : 0;
    }
    under = wave_sum_i(under);
    if ((threadIdx.x & 63) == 0 && under) atomicAdd(count, (unsigned long long)under);      // integers: exact in any order
    if (blockIdx.x == 0 && threadIdx.x == 0) n_dev[0] = n;
}

__global__ void pd_pick_kernel(int n, const unsigned long long* __restrict__ sorted_keys, long long k0,
                               float* __restrict__ order_stats) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long k1 = k0 + 1 < n ? k0 + 1 : n - 1;
    order_stats[0] = __uint_as_float((unsigned)sorted_keys[k0]);
    order_stats[1] = __uint_as_float((unsigned)sorted_keys[k1]);
}

struct PdWorkspace {
    int* hdr;                               // [8]: n (the sort's n_dev), the sort's status
    unsigned long long *keys, *keys_alt;
    int *vals, *vals_alt;
    void* sort_ws;
    long long sort_ws_bytes;
    long long total_bytes;
};

static PdWorkspace pd_layout(void* base, long long n) {
    PdWorkspace w;
    n = n > 0 ? n : 1;
    char* p = (char*)base;
    long long o = 0;
    auto take = [&](long long bytes) { char* r = p + o; o += nn_align(bytes); return r; };
    w.hdr = (int*)take(8 * 4);
    w.keys = (unsigned long long*)take(n * 8);
    w.keys_alt = (unsigned long long*)take(n * 8);
    w.vals = (int*)take(n * 4);
    w.vals_alt = (int*)take(n * 4);
    w.sort_ws_bytes = qed_sort_workspace_bytes(n);
    w.sort_ws = take(w.sort_ws_bytes);
    w.total_bytes = o;
    return w;
}

// one pass of the build with the cell size that is in the header
static int nn_build_pass(int n, const float* target, const NnWorkspace& w, hipStream_t st) {
    const int n_chunks = (n + kNnChunk - 1) / kNnChunk;
    const unsigned grid_n = (unsigned)(((long long)n + kNnThreads - 1) / kNnThreads);
    const unsigned grid_c = (unsigned)((n_chunks + kNnThreads / 64 - 1) / (kNnThreads / 64));
    hipLaunchKernelGGL(nn_key_kernel, dim3(grid_n), dim3(kNnThreads), 0, st, n, target, (const NnHeader*)w.hdr, w.keys,
                       w.vals, (int*)nullptr);
    const int side = qed_sort_pairs((uint64_t*)w.keys, w.vals, (uint64_t*)w.keys_alt, w.vals_alt, &w.hdr->n_sort, n,
                                    3 * kNnAxisBits, w.sort_ws, w.sort_ws_bytes, w.hdr->scan_status, (void*)st);
    if (side < 0) return side;
    const unsigned long long* keys = side ? w.keys_alt : w.keys;
    const int* vals = side ? w.vals_alt : w.vals;
    hipLaunchKernelGGL(nn_count_kernel, dim3(grid_c), dim3(kNnThreads), 0, st, n, n_chunks, keys, w.chunk_heads);
    const int rc = qed_isect_scan(w.chunk_heads, n_chunks, w.chunk_base, &w.hdr->n_cells, n, w.hdr->scan_status, (void*)st);
    if (rc != QED_OK) return rc;
    hipLaunchKernelGGL(nn_compact_kernel, dim3(grid_c), dim3(kNnThreads), 0, st, n, n_chunks, target, keys, vals,
                       (const int*)w.chunk_base, w.cell_key, w.cell_start, w.sorted_pts);
    return QED_OK;
}

}  // namespace qed

using namespace qed;

extern "C" int64_t qed_nn_workspace_bytes(int64_t n_target, int64_t n_query) {
    if (n_target < 0 || n_query < 0 || n_target >= (1ll << 30) || n_query >= (1ll << 30)) return QED_E_INVALID_ARG;
    return nn_layout(nullptr, n_target, n_query).total_bytes;
}

extern "C" int qed_nn_build(int32_t n_target, const float* target, float cell_size, int32_t flags, void* workspace,
                            int64_t workspace_bytes, int64_t n_query_capacity, int32_t* status, void* stream) {
    QED_REQUIRE(n_target >= 1 && n_target < (1 << 30), "n_target out of range (an index needs at least one point)");
    QED_REQUIRE(n_query_capacity >= 0 && n_query_capacity < (1ll << 30), "n_query_capacity out of range");
    QED_REQUIRE((flags & ~QED_NN_AUTO_CELL) == 0, "unknown flags");
    const bool auto_cell = (flags & QED_NN_AUTO_CELL) != 0;
    QED_REQUIRE(auto_cell || (isfinite(cell_size) && cell_size > 0.f), "cell_size must be finite and > 0");
    QED_REQUIRE(target && workspace && status, "null buffers");
    const NnWorkspace w = nn_layout(workspace, n_target, n_query_capacity);
    if (workspace_bytes < w.total_bytes) {
        set_error("qed_nn_build: workspace too small (%lld < %lld)", (long long)workspace_bytes, w.total_bytes);
        return QED_E_WORKSPACE;
    }
    QED_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid_mm = stream_grid(n_target, kNnMaxGrid);
    hipLaunchKernelGGL(nn_minmax_kernel, dim3(grid_mm), dim3(kNnThreads), 0, st, n_target, target, w.part, w.part_bad);
    hipLaunchKernelGGL(nn_fold_kernel, dim3(1), dim3(kNnThreads), 0, st, n_target, (int)grid_mm, (const float*)w.part,
                       (const int*)w.part_bad, auto_cell ? 0.f : cell_size, w.hdr, status);
    int rc = nn_build_pass(n_target, target, w, st);
    if (rc != QED_OK) return rc;
    if (auto_cell) {
        hipLaunchKernelGGL(nn_refine_kernel, dim3(1), dim3(64), 0, st, n_target, w.hdr);
        rc = nn_build_pass(n_target, target, w, st);
        if (rc != QED_OK) return rc;
    }
    return check_launch("qed_nn_build");
}

extern "C" int qed_nn_query(int32_t n_query, const float* query, int32_t n_target, void* workspace,
                            int64_t workspace_bytes, int64_t n_query_capacity, int32_t max_rings, int32_t flags,
                            float* dist, int32_t* idx, int32_t* fallback, void* stream) {
    QED_REQUIRE(n_query >= 0 && n_query < (1 << 30), "n_query out of range");
    QED_REQUIRE(n_target >= 1 && n_target < (1 << 30), "n_target out of range (the index holds at least one point)");
    QED_REQUIRE(n_query_capacity >= n_query && n_query_capacity < (1ll << 30), "n_query_capacity out of range");
    QED_REQUIRE(max_rings >= 0 && max_rings <= kNnMaxRings, "max_rings must be in [0, 64]");
    QED_REQUIRE((flags & ~QED_NN_NATURAL_ORDER) == 0, "unknown flags");
    QED_REQUIRE(fallback, "null buffers (fallback)");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(fallback, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("qed_nn_query: memset failed");
        return QED_E_LAUNCH;
    }
    if (n_query == 0) return QED_OK;
    QED_REQUIRE(query && workspace && dist && idx, "null buffers");
    const NnWorkspace w = nn_layout(workspace, n_target, n_query_capacity);
    if (workspace_bytes < w.total_bytes) {
        set_error("qed_nn_query: workspace too small (%lld < %lld)", (long long)workspace_bytes, w.total_bytes);
        return QED_E_WORKSPACE;
    }
    QED_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    const unsigned grid_q = (unsigned)(((long long)n_query + kNnThreads - 1) / kNnThreads);
    const int* perm = nullptr;
    if (!(flags & QED_NN_NATURAL_ORDER)) {
        hipLaunchKernelGGL(nn_key_kernel, dim3(grid_q), dim3(kNnThreads), 0, st, n_query, query, (const NnHeader*)w.hdr,
                           w.qkeys, w.qvals, w.q_n);
        const int side = qed_sort_pairs((uint64_t*)w.qkeys, w.qvals, (uint64_t*)w.qkeys_alt, w.qvals_alt, w.q_n, n_query,
                                        3 * kNnAxisBits, w.qsort_ws, w.qsort_ws_bytes, w.q_n + 4, stream);
        if (side < 0) return side;
        perm = side ? w.qvals_alt : w.qvals;
    }
    hipLaunchKernelGGL(nn_grid_query_kernel, dim3(grid_q), dim3(kNnThreads), 0, st, n_query, query, perm,
                       (const NnHeader*)w.hdr, (const unsigned long long*)w.cell_key, (const int*)w.cell_start,
                       (const float4*)w.sorted_pts, max_rings, dist, idx, fallback);
    return check_launch("qed_nn_query");
}

extern "C" int qed_nn_brute(int32_t n_query, const float* query, int32_t n_target, const float* target,
                            const int32_t* rows, float* dist, int32_t* idx, void* workspace, int64_t workspace_bytes,
                            void* stream) {
    QED_REQUIRE(n_query >= 0 && n_query < (1 << 30), "n_query out of range");
    QED_REQUIRE(n_target >= 1 && n_target < (1 << 30), "n_target out of range (at least one target point)");
    if (n_query == 0) return QED_OK;
    QED_REQUIRE(query && target && dist && idx && workspace, "null buffers");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    if (workspace_bytes < 8ll * n_query) {
        set_error("qed_nn_brute: workspace too small (%lld < %lld)", (long long)workspace_bytes, 8ll * n_query);
        return QED_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* best = (unsigned long long*)workspace;
    if (hipMemsetAsync(best, 0xff, 8ull * n_query, st) != hipSuccess) {
        set_error("qed_nn_brute: memset failed");
        return QED_E_LAUNCH;
    }
    const long long tiles = ((long long)n_target + kBruteTile - 1) / kBruteTile;
    const int slices = (int)(tiles < kBruteMaxSlices ? tiles : kBruteMaxSlices);
    const int per_slice = (int)((tiles + slices - 1) / slices) * kBruteTile;
    long long gx = ((long long)n_query + kNnThreads * kBruteQ - 1) / (kNnThreads * kBruteQ);
    if (gx > kBruteMaxGridX) gx = kBruteMaxGridX;
    hipLaunchKernelGGL(nn_brute_kernel, dim3((unsigned)gx, (unsigned)slices), dim3(kNnThreads), 0, st, n_query, query,
                       n_target, target, rows, per_slice, best);
    hipLaunchKernelGGL(nn_finish_kernel, dim3(stream_grid(n_query)), dim3(kNnThreads), 0, st, n_query, rows,
                       (const unsigned long long*)best, dist, idx);
    return check_launch("qed_nn_brute");
}

extern "C" int64_t qed_pd_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (1ll << 30)) return QED_E_INVALID_ARG;
    return pd_layout(nullptr, n).total_bytes;
}

extern "C" int qed_pd_reduce(int32_t n, const float* dist, double threshold, int64_t k0, int64_t* count_under,
                             float* order_stats, void* workspace, int64_t workspace_bytes, void* stream) {
    QED_REQUIRE(n >= 1 && n < (1 << 30), "n out of range (at least one distance)");
    QED_REQUIRE(threshold == threshold, "threshold must not be NaN");
    QED_REQUIRE(k0 >= 0 && k0 < n, "k0 must be in [0, n)");
    QED_REQUIRE(dist && count_under && order_stats && workspace, "null buffers");
    QED_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
    const PdWorkspace w = pd_layout(workspace, n);
    if (workspace_bytes < w.total_bytes) {
        set_error("qed_pd_reduce: workspace too small (%lld < %lld)", (long long)workspace_bytes, w.total_bytes);
        return QED_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(count_under, 0, sizeof(int64_t), st) != hipSuccess) {
        set_error("qed_pd_reduce: memset failed");
        return QED_E_LAUNCH;
    }
    hipLaunchKernelGGL(pd_prepare_kernel, dim3(stream_grid(n)), dim3(kNnThreads), 0, st, n, dist, threshold, w.keys,
                       w.vals, w.hdr, (unsigned long long*)count_under);
    const int side = qed_sort_pairs((uint64_t*)w.keys, w.vals, (uint64_t*)w.keys_alt, w.vals_alt, w.hdr, n, 32, w.sort_ws,
                                    w.sort_ws_bytes, w.hdr + 4, stream);
    if (side < 0) return side;
    hipLaunchKernelGGL(pd_pick_kernel, dim3(1), dim3(64), 0, st, n, (const unsigned long long*)(side ? w.keys_alt : w.keys),
                       (long long)k0, order_stats);
    return check_launch("qed_pd_reduce");
}

// ---- k nearest neighbours ----------------------------------------------------------------------------------------
namespace qed {

template <int KK>
static void knn_launch_grid(unsigned grid_q, hipStream_t st, int nq, const float* query, const int* perm, const NnWorkspace& w,
                            int max_rings, int k, float* dist, int* idx, int* fallback) {
    hipLaunchKernelGGL(knn_grid_query_kernel<KK>, dim3(grid_q), dim3(kNnThreads), 0, st, nq, query, perm,
                       (const NnHeader*)w.hdr, (const unsigned long long*)w.cell_key, (const int*)w.cell_start,
                       (const float4*)w.sorted_pts, max_rings, k, dist, idx, fallback);
}

template <int KK>
static void knn_launch_brute(unsigned grid, hipStream_t st, int nq, const float* query, int nt, const float* target,
                             const int* rows, int k, float* dist, int* idx) {
    hipLaunchKernelGGL(knn_brute_kernel<KK>, dim3(grid), dim3(kNnThreads), 0, st, nq, query, nt, target, rows, k, dist, idx);
}

#define QED_KNN_DISPATCH(held, fn, ...)                                                                      \
    switch (held) {                                                                                          \
        case 1: fn<1>(__VA_ARGS__); break;                                                                   \
        case 2: fn<2>(__VA_ARGS__); break;                                                                   \
        case 3: fn<3>(__VA_ARGS__); break;                                                                   \
        case 4: fn<4>(__VA_ARGS__); break;                                                                   \
        case 5: fn<5>(__VA_ARGS__); break;                                                                   \
        case 6: fn<6>(__VA_ARGS__); break;                                                                   \
        case 7: fn<7>(__VA_ARGS__); break;                                                                   \
        case 8: fn<8>(__VA_ARGS__); break;                                                                   \
        default: fn<9>(__VA_ARGS__); break;                                                                  \
    }

}  // namespace qed

extern "C" int qed_knn_query(int32_t n_query, const float* query, int32_t n_target, void* workspace,
                             int64_t workspace_bytes, int64_t n_query_capacity, int32_t k, int32_t max_rings,
                             int32_t flags, float* dist, int32_t* idx, int32_t* fallback, void* stream) {
    QED_REQUIRE(n_query >= 0 && n_query < (1 << 30), "n_query out of range");
    QED_REQUIRE(k >= 1 && k <= kKnnMaxK, "k must be in [1, 8]");
    QED_REQUIRE((flags & ~(QED_NN_NATURAL_ORDER | QED_KNN_SKIP_FIRST)) == 0, "unknown flags");
    const int held = k + ((flags & QED_KNN_SKIP_FIRST) ? 1 : 0);
    QED_REQUIRE(n_target >= held && n_target < (1 << 30),
                "n_target out of range (at least k target points, k + 1 with QED_KNN_SKIP_FIRST)");
    QED_REQUIRE(n_query_capacity >= n_query && n_query_capacity < (1ll << 30), "n_query_capacity out of range");
    QED_REQUIRE(max_rings >= 0 && max_rings <= kNnMaxRings, "max_rings must be in [0, 64]");
    QED_REQUIRE(fallback, "null buffers (fallback)");
    hipStream_t st = (hipStream_t)stream;
    if (n_query > 0) {
        QED_REQUIRE(query && workspace && dist && idx, "null buffers");
        if (workspace_bytes < nn_layout(nullptr, n_target, n_query_capacity).total_bytes) {
            set_error("qed_knn_query: workspace too small (%lld < %lld)", (long long)workspace_bytes,
                      nn_layout(nullptr, n_target, n_query_capacity).total_bytes);
            return QED_E_WORKSPACE;
        }
        QED_REQUIRE(((uintptr_t)workspace & 15) == 0, "workspace must be 16-byte aligned");
    }
    if (hipMemsetAsync(fallback, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("qed_knn_query: memset failed");
        return QED_E_LAUNCH;
    }
    if (n_query == 0) return QED_OK;
    const NnWorkspace w = nn_layout(workspace, n_target, n_query_capacity);
    const unsigned grid_q = (unsigned)(((long long)n_query + kNnThreads - 1) / kNnThreads);
    const int* perm = nullptr;
    if (!(flags & QED_NN_NATURAL_ORDER)) {
        hipLaunchKernelGGL(nn_key_kernel, dim3(grid_q), dim3(kNnThreads), 0, st, n_query, query, (const NnHeader*)w.hdr,
                           w.qkeys, w.qvals, w.q_n);
        const int side = qed_sort_pairs((uint64_t*)w.qkeys, w.qvals, (uint64_t*)w.qkeys_alt, w.qvals_alt, w.q_n, n_query,
                                        3 * kNnAxisBits, w.qsort_ws, w.qsort_ws_bytes, w.q_n + 4, stream);
        if (side < 0) return side;
        perm = side ? w.qvals_alt : w.qvals;
    }
    QED_KNN_DISPATCH(held, knn_launch_grid, grid_q, st, n_query, query, perm, w, max_rings, k, dist, idx, fallback);
    return check_launch("qed_knn_query");
}

extern "C" int qed_knn_brute(int32_t n_query, const float* query, int32_t n_target, const float* target,
                             const int32_t* rows, int32_t k, int32_t flags, float* dist, int32_t* idx, void* stream) {
    QED_REQUIRE(n_query >= 0 && n_query < (1 << 30), "n_query out of range");
    QED_REQUIRE(k >= 1 && k <= kKnnMaxK, "k must be in [1, 8]");
    QED_REQUIRE((flags & ~QED_KNN_SKIP_FIRST) == 0, "unknown flags");
    const int held = k + ((flags & QED_KNN_SKIP_FIRST) ? 1 : 0);
    QED_REQUIRE(n_target >= held && n_target < (1 << 30),
                "n_target out of range (at least k target points, k + 1 with QED_KNN_SKIP_FIRST)");
    if (n_query == 0) return QED_OK;
    QED_REQUIRE(query && target && dist && idx, "null buffers");
    long long g = ((long long)n_query + kNnThreads / 64 - 1) / (kNnThreads / 64);
    if (g > kKnnBruteMaxGrid) g = kKnnBruteMaxGrid;
    QED_KNN_DISPATCH(held, knn_launch_brute, (unsigned)g, (hipStream_t)stream, n_query, query, n_target, target, rows, k,
                     dist, idx);
    return check_launch("qed_knn_brute");
}
