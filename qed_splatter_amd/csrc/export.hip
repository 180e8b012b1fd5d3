// Trained Gaussians to and from the rows of a standard 3DGS PLY file (qed_splatter_amd/gaussian_ply.py states the file
// format): qed_pack_gaussians turns the six SoA parameter tensors into compacted AoS rows, qed_unpack_gaussians turns
// the rows of a file back into the six tensors.  Both can move the Gaussians through a similarity p' = s (R p + t) on
// the way: means through the map, log-scales plus log s, quaternions left-multiplied by the quaternion of R, the SH
// coefficients of bands 1-3 through the three band matrices the host fitted for R.  Without a similarity every value
// is moved bit for bit.
//
// One workgroup of 256 threads owns kPackRows = 128 consecutive Gaussians and one tile of LDS [kPackRows][RF] in the ROW layout
// (pack: the file's column order; unpack: the model's group order).
//   load       every SoA array is read along itself -- lane i takes element i of the workgroup's range -- and scattered
//              into the tile; features_rest [N,K,3] lands channel-major here, that is the whole transpose.  (unpack:
//              element (row, column) of the tile reads row_bytes * row + offset[column] of the file body; for files in
//              this package's own column order neighbouring lanes read neighbouring addresses.)
//   transform  (only with a similarity) work items (row, task) with the task uniform per wave: the geometry of a row, or
//              the 15 coefficients of one colour channel.  Every new element is one dot product of at most seven terms,
//              accumulated in float64 from float64 matrix entries and rounded to float32 once.
//   classify   (pack) a row is dropped if one of its values is not finite, else if its opacity logit is below
//              kMinOpacityLogit.  Kept rows are ranked by ballot + prefix of the wave totals: input order.
//   store      (pack) the workgroup's kept rows are one contiguous byte range of the row buffer.  It is cut at the 16-byte
//              boundaries of the BUFFER: a lane assembles one such chunk from the tile and stores it whole; the (at most
//              two) chunks the workgroup shares with its neighbours are stored unit by unit (dwords; bytes in rgb mode,
//              whose rows are 59 bytes long).  (unpack) each of the six arrays is written along itself.
// The position of a workgroup's rows in the buffer is the exclusive scan of the kept counts of the workgroups before it:
// pack_count (this same kernel, stopping after classify) -> pack_scan (one workgroup walks the counts 256 at a time and
// carries the running total; it also writes the three result words) -> pack.  No atomics anywhere, nothing depends on
// scheduling, and the parameters are read twice (2 x 248 B in, 248 B out per Gaussian at degree 3).
#include <cmath>

#include "qed_common.h"

namespace qed {

constexpr int kPackRows = 128;               // Gaussians per workgroup
constexpr int kPackThreads = 256;
constexpr float kMinOpacityLogit = -5.5373f;  // logit(1 / 255): the rasteriser skips what lies below
constexpr int kShMatDoubles = 9 + 25 + 49;

__host__ __device__ constexpr int sh_rest_count(int deg) { return (deg + 1) * (deg + 1) - 1; }
__host__ __device__ constexpr int pack_row_floats(int deg) { return 17 + 3 * sh_rest_count(deg); }

// the similarity as the kernels apply it: p' = M p + b (M = s R, b = s t), log-scales + dls, q' = qr (x) q
struct FrameChange {
    int active;
    double M[9], b[3], dls, qr[4];
    double sh[kShMatDoubles];                // band 1 (3 x 3), band 2 (5 x 5), band 3 (7 x 7), row-major
};

// where a row of the tile keeps what: first columns of means, scales, quats; coefficient k (1 .. K) of channel c sits
// at rest + (k - 1) * rest_k + c * rest_c
struct RowCols {
    int means, scales, quats, rest, rest_k, rest_c;
};

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the transform phase on `rows` rows of the tile (row stride RF floats)
template <int DEG>
__device__ __forceinline__ void frame_change_tile(float* __restrict__ tile, int RF, int rows, const RowCols& L,
                                                  const FrameChange& fc) {
    constexpr int K = sh_rest_count(DEG);
    constexpr int n_tasks = DEG > 0 ? 4 : 1;
    for (int item = threadIdx.x; item < n_tasks * kPackRows; item += kPackThreads) {
        const int task = item / kPackRows, r = item % kPackRows;            // (kPackRows is a multiple of the wave)
        if (r >= rows) continue;
        float* row = tile + r * RF;
        if (task == 0) {
            const double p0 = row[L.means], p1 = row[L.means + 1], p2 = row[L.means + 2];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                row[L.means + i] = (float)(fc.M[3 * i] * p0 + fc.M[3 * i + 1] * p1 + fc.M[3 * i + 2] * p2 + fc.b[i]);
#pragma unroll
            for (int i = 0; i < 3; ++i) row[L.scales + i] = (float)((double)row[L.scales + i] + fc.dls);
            const double w = row[L.quats], x = row[L.quats + 1], y = row[L.quats + 2], z = row[L.quats + 3];
            const double a = fc.qr[0], b = fc.qr[1], c = fc.qr[2], d = fc.qr[3];
            row[L.quats] = (float)(a * w - b * x - c * y - d * z);
            row[L.quats + 1] = (float)(a * x + b * w + c * z - d * y);
            row[L.quats + 2] = (float)(a * y - b * z + c * w + d * x);
            row[L.quats + 3] = (float)(a * z + b * y - c * x + d * w);
        } else if constexpr (DEG > 0) {
            const int c = task - 1;
            float* co = row + L.rest + c * L.rest_c;
            double v[K];
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = co[k * L.rest_k];
            int base = 0, mat = 0;
#pragma unroll
            for (int l = 1; l <= DEG; ++l) {
                const int n = 2 * l + 1;
#pragma unroll
                for (int i = 0; i < n; ++i) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < n; ++j) acc += fc.sh[mat + i * n + j] * v[base + j];
                    co[(base + i) * L.rest_k] = (float)acc;
                }
                base += n;
                mat += n * n;
            }
        }
    }
}

struct PackArgs {
    int N;
    const float* means;
    const float* scales;
    const float* quats;
    const float* opacities;
    const float* features_dc;
    const float* features_rest;
    int sigmoid_colors;                      // rgb mode of a degree-0 model
    int* block_counts;                       // [3][n_blocks]: kept, dropped non-finite, dropped transparent
    const int* block_base;                   // [n_blocks]: kept rows of all workgroups before this one
    unsigned char* rows;                     // the row buffer (16-byte aligned)
};

// one SoA array of `width` floats per Gaussian into columns col(comp) of the tile
template <typename ColOf>
__device__ __forceinline__ void load_group(float* __restrict__ tile, int RF, const float* __restrict__ src, long long row0,
                                           int rows, int width, ColOf col) {
    const float* s = src + row0 * width;
    for (int e = threadIdx.x; e < rows * width; e += kPackThreads) {
        const int r = e / width, comp = e - r * width;
        tile[r * RF + col(comp)] = s[e];
    }
}

// DEG 0..3: sh_coeffs rows of 17 + 3 K floats; DEG -1: rgb rows (the tile is that of degree 0, the store packs it into
// 59 bytes)
template <int DEG, bool COUNT_ONLY>
__global__ void __launch_bounds__(kPackThreads) pack_kernel(PackArgs a, FrameChange fc) {
    constexpr bool RGB = DEG < 0;
    constexpr int D = RGB ? 0 : DEG;
    constexpr int K = sh_rest_count(D);
    constexpr int RF = pack_row_floats(D);
    __shared__ float tile[kPackRows * RF];
    __shared__ int kept_list[kPackRows];
    __shared__ int wave_cnt[3][kPackThreads / kWave];
    const long long row0 = (long long)blockIdx.x * kPackRows;
    const int rows = (int)min((long long)kPackRows, (long long)a.N - row0);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const RowCols L{0, 10 + 3 * K, 13 + 3 * K, 9, 1, K};

    // ---- load
    load_group(tile, RF, a.means, row0, rows, 3, [](int c) { return c; });
    for (int e = tid; e < rows * 3; e += kPackThreads) tile[(e / 3) * RF + 3 + e % 3] = 0.f;       // nx ny nz
    load_group(tile, RF, a.features_dc, row0, rows, 3, [](int c) { return 6 + c; });
    if constexpr (K > 0 && !RGB)
        load_group(tile, RF, a.features_rest, row0, rows, 3 * K, [](int c) { return 9 + (c % 3) * K + c / 3; });
    load_group(tile, RF, a.opacities, row0, rows, 1, [](int) { return 9 + 3 * K; });
    load_group(tile, RF, a.scales, row0, rows, 3, [](int c) { return 10 + 3 * K + c; });
    load_group(tile, RF, a.quats, row0, rows, 4, [](int c) { return 13 + 3 * K + c; });
    __syncthreads();
    if (fc.active) {
        if constexpr (RGB) frame_change_tile<0>(tile, RF, rows, L, fc);
        else frame_change_tile<D>(tile, RF, rows, L, fc);
        __syncthreads();
    }

    // ---- classify and rank (thread r owns row r; threads kPackRows.. hold no row)
    int keep = 0, bad = 0, faint = 0;
    if (tid < rows) {
        const float* row = tile + tid * RF;
        bool fin = true;
#pragma unroll 1
        for (int c = 0; c < RF; ++c) fin = fin && finite_bits(row[c]);
        bad = !fin;
        faint = fin && row[9 + 3 * K] < kMinOpacityLogit;
        keep = fin && !faint;
    }
    const unsigned long long m_keep = __ballot(keep), m_bad = __ballot(bad), m_faint = __ballot(faint);
    if (lane == 0) {
        wave_cnt[0][wid] = __popcll(m_keep);
        wave_cnt[1][wid] = __popcll(m_bad);
        wave_cnt[2][wid] = __popcll(m_faint);
    }
    __syncthreads();
    int before = 0, n_keep = 0;
#pragma unroll
    for (int w = 0; w < kPackThreads / kWave; ++w) {
        before += w < wid ? wave_cnt[0][w] : 0;
        n_keep += wave_cnt[0][w];
    }
    if constexpr (COUNT_ONLY) {
        if (tid < 3) {
            int t = 0;
#pragma unroll
            for (int w = 0; w < kPackThreads / kWave; ++w) t += wave_cnt[tid][w];
            a.block_counts[(long long)tid * gridDim.x + blockIdx.x] = t;
        }
        return;
    } else {
        if (keep) kept_list[before + __popcll(m_keep & ((1ull << lane) - 1ull))] = tid;
        if constexpr (RGB) {
            // the colour bytes, once per kept or dropped row: clamp(SH_C0 f + 0.5, 0, 1) * 255 (degree 0: the sigmoid)
            // truncated, evaluated in float64
            for (int e = tid; e < rows * 3; e += kPackThreads) {
                float* p = tile + (e / 3) * RF + 6 + e % 3;
                const double f = *p;
                const double c = a.sigmoid_colors ? 1.0 / (1.0 + exp(-f)) : 0.28209479177387814 * f + 0.5;
                const double q = fmin(fmax(c, 0.0), 1.0) * 255.0;          // (fmax(NaN, 0) = 0: a dropped row's, never stored)
                *p = __uint_as_float((unsigned)q);
            }
        }
        __syncthreads();
        if (n_keep == 0) return;

        // ---- store
        const unsigned* t32 = reinterpret_cast<const unsigned*>(tile);
        constexpr int UNIT = RGB ? 1 : 4;                                   // bytes per unit
        constexpr int ROW_UNITS = RGB ? 59 : RF;
        constexpr int PER = 16 / UNIT;                                      // units per 16-byte chunk
        const long long g0 = (long long)a.block_base[blockIdx.x] * ROW_UNITS;   // first unit of this workgroup's rows
        const int n = n_keep * ROW_UNITS;
        const long long c0 = g0 / PER;
        const int n_chunks = (int)((g0 + n + PER - 1) / PER - c0);
        auto unit_at = [&](int u) -> unsigned {                              // unit u of the workgroup's compacted rows
            const int k = u / ROW_UNITS, w = u - k * ROW_UNITS;
            const unsigned* row = t32 + kept_list[k] * RF;
            if constexpr (!RGB) return row[w];
            else {
                if (w < 24) return (row[w >> 2] >> (8 * (w & 3))) & 255u;
                if (w < 27) return row[6 + (w - 24)] & 255u;
                const int w2 = w - 27;
                return (row[9 + (w2 >> 2)] >> (8 * (w2 & 3))) & 255u;
            }
        };
        for (int lc = tid; lc < n_chunks; lc += kPackThreads) {
            const long long first = (c0 + lc) * PER;                        // global unit index of the chunk's first unit
            const int u0 = (int)(first - g0);                               // may be negative in the first chunk
            if (u0 >= 0 && u0 + PER <= n) {
                unsigned w[4];
                if constexpr (!RGB) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[j] = unit_at(u0 + j);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        w[j] = 0;
#pragma unroll
                        for (int b = 0; b < 4; ++b) w[j] |= unit_at(u0 + 4 * j + b) << (8 * b);
                    }
                }
                *reinterpret_cast<uint4*>(a.rows + (c0 + lc) * 16) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
#pragma unroll 1
                for (int j = 0; j < PER; ++j) {
                    const int u = u0 + j;
                    if (u < 0 || u >= n) continue;
                    if constexpr (!RGB) reinterpret_cast<unsigned*>(a.rows)[first + j] = unit_at(u);
                    else a.rows[first + j] = (unsigned char)unit_at(u);
                }
            }
        }
    }
}

// exclusive scan of the kept counts, 256 workgroups at a time with a carried total; totals[0..2] = rows written,
// dropped as non-finite, dropped as transparent
__global__ void __launch_bounds__(256) pack_scan_kernel(const int* __restrict__ block_counts, int n_blocks,
                                                        int* __restrict__ block_base, int* __restrict__ totals) {
    __shared__ int wave_tot[4];
    __shared__ int drop_tot[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int carry = 0, bad = 0, faint = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += 256) {
        const int b = b0 + tid;
        const int v = b < n_blocks ? block_counts[b] : 0;
        if (b < n_blocks) {
            bad += block_counts[(long long)n_blocks + b];
            faint += block_counts[2ll * n_blocks + b];
        }
        int sc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(sc, o, 64); if (lane >= o) sc += y; }
        if (lane == 63) wave_tot[wid] = sc;
        __syncthreads();
        int base = carry, all = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { base += w < wid ? wave_tot[w] : 0; all += wave_tot[w]; }
        if (b < n_blocks) block_base[b] = base + sc - v;
        carry += all;
        __syncthreads();
    }
    // the two drop counts: per-thread partials -> wave sums -> thread 0
    bad = wave_sum_i(bad); faint = wave_sum_i(faint);
    if (lane == 0) { drop_tot[0][wid] = bad; drop_tot[1][wid] = faint; }
    __syncthreads();
    if (tid == 0) {
        totals[0] = carry;
        totals[1] = drop_tot[0][0] + drop_tot[0][1] + drop_tot[0][2] + drop_tot[0][3];
        totals[2] = drop_tot[1][0] + drop_tot[1][1] + drop_tot[1][2] + drop_tot[1][3];
    }
}

struct UnpackArgs {
    int N;
    const unsigned char* rows;
    long long row_bytes;
    int offsets[14 + 45];                    // byte offset inside a row of every model-order column
    int aligned;                             // every address is a multiple of 4
    float* means;
    float* scales;
    float* quats;
    float* opacities;
    float* features_dc;
    float* features_rest;
};

template <int DEG>
__global__ void __launch_bounds__(kPackThreads) unpack_kernel(UnpackArgs a, FrameChange fc) {
    constexpr int K = sh_rest_count(DEG);
    constexpr int RF = 14 + 3 * K;                                          // means scales quats opacity dc rest[K][3]
    __shared__ float tile[kPackRows * RF];
    const long long row0 = (long long)blockIdx.x * kPackRows;
    const int rows = (int)min((long long)kPackRows, (long long)a.N - row0);
    const int tid = threadIdx.x;
    const unsigned char* src = a.rows + row0 * a.row_bytes;
    for (int e = tid; e < rows * RF; e += kPackThreads) {
        const int r = e / RF, c = e - r * RF;
        const unsigned char* p = src + r * a.row_bytes + a.offsets[c];
        float v;
        if (a.aligned) v = *reinterpret_cast<const float*>(p);
        else __builtin_memcpy(&v, p, 4);
        tile[e] = v;
    }
    __syncthreads();
    if (fc.active) {
        const RowCols L{0, 3, 6, 14, 3, 1};
        frame_change_tile<DEG>(tile, RF, rows, L, fc);
        __syncthreads();
    }
    auto store_group = [&](float* dst, int width, int col0) {
        float* d = dst + row0 * width;
        for (int e = tid; e < rows * width; e += kPackThreads) {
            const int r = e / width;
            d[e] = tile[r * RF + col0 + (e - r * width)];
        }
    };
    store_group(a.means, 3, 0);
    store_group(a.scales, 3, 3);
    store_group(a.quats, 4, 6);
    store_group(a.opacities, 1, 10);
    store_group(a.features_dc, 3, 11);
    if constexpr (K > 0) store_group(a.features_rest, 3 * K, 14);
}

// h_similarity: R[9] row-major, t[3], s, quaternion of R (wxyz) -- 17 doubles; h_sh: the three band matrices
static int make_frame_change(const double* h_similarity, const double* h_sh, FrameChange& fc) {
    fc = FrameChange{};
    if (h_similarity == nullptr && h_sh == nullptr) return QED_OK;
    if (h_similarity == nullptr || h_sh == nullptr) return QED_E_INVALID_ARG;
    const double s = h_similarity[12];
    if (!(s > 0.0) || !std::isfinite(s)) return QED_E_INVALID_ARG;
    fc.active = 1;
    for (int i = 0; i < 9; ++i) fc.M[i] = s * h_similarity[i];
    for (int i = 0; i < 3; ++i) fc.b[i] = s * h_similarity[9 + i];
    fc.dls = log(s);
    for (int i = 0; i < 4; ++i) fc.qr[i] = h_similarity[13 + i];
    for (int i = 0; i < kShMatDoubles; ++i) fc.sh[i] = h_sh[i];
    return QED_OK;
}

static long long pack_blocks(long long N) { return (N + kPackRows - 1) / kPackRows; }

template <int DEG>
static void launch_pack(const PackArgs& a, const FrameChange& fc, unsigned grid, int* totals, hipStream_t st) {
    hipLaunchKernelGGL((pack_kernel<DEG, true>), dim3(grid), dim3(kPackThreads), 0, st, a, fc);
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(256), 0, st, a.block_counts, (int)grid,
                       const_cast<int*>(a.block_base), totals);
    hipLaunchKernelGGL((pack_kernel<DEG, false>), dim3(grid), dim3(kPackThreads), 0, st, a, fc);
}

}  // namespace qed

using namespace qed;

extern "C" int64_t qed_pack_workspace_bytes(int64_t N) {
    if (N < 1) return QED_E_INVALID_ARG;
    return 4 * pack_blocks(N) * (int64_t)sizeof(int);
}

extern "C" int qed_pack_gaussians(int32_t N, int32_t sh_degree, int32_t color_mode, const float* means, const float* scales,
                                  const float* quats, const float* opacities, const float* features_dc,
                                  const float* features_rest, const double* h_similarity, const double* h_sh, uint8_t* rows,
                                  int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
    QED_REQUIRE(N >= 1, "N must be at least 1");
    QED_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "SH degree must be in [0, 3]");
    QED_REQUIRE(color_mode == 0 || color_mode == 1, "color_mode must be 0 (sh_coeffs) or 1 (rgb)");
    QED_REQUIRE(means && scales && quats && opacities && features_dc && rows && counts && workspace, "null buffers");
    QED_REQUIRE(features_rest || sh_degree == 0 || color_mode == 1, "features_rest is null");
    QED_REQUIRE(((uintptr_t)rows & 15u) == 0, "the row buffer must be 16-byte aligned");
    if (workspace_bytes < qed_pack_workspace_bytes(N)) {
        set_error("qed_pack_gaussians: workspace too small (see qed_pack_workspace_bytes)");
        return QED_E_WORKSPACE;
    }
    FrameChange fc;
    QED_REQUIRE(make_frame_change(h_similarity, h_sh, fc) == QED_OK,
                "h_similarity and h_sh come together, and the scale must be positive and finite");
    const unsigned grid = (unsigned)pack_blocks(N);
    PackArgs a;
    a.N = N;
    a.means = means; a.scales = scales; a.quats = quats; a.opacities = opacities;
    a.features_dc = features_dc; a.features_rest = features_rest;
    a.sigmoid_colors = color_mode == 1 && sh_degree == 0;
    a.block_counts = static_cast<int*>(workspace);
    a.block_base = a.block_counts + 3ll * grid;
    a.rows = rows;
    hipStream_t st = (hipStream_t)stream;
    if (color_mode == 1) launch_pack<-1>(a, fc, grid, counts, st);
    else if (sh_degree == 0) launch_pack<0>(a, fc, grid, counts, st);
    else if (sh_degree == 1) launch_pack<1>(a, fc, grid, counts, st);
    else if (sh_degree == 2) launch_pack<2>(a, fc, grid, counts, st);
    else launch_pack<3>(a, fc, grid, counts, st);
    return check_launch("qed_pack_gaussians");
}

extern "C" int qed_unpack_gaussians(int32_t N, int32_t sh_degree, const uint8_t* rows, int64_t row_bytes,
                                    const int32_t* h_offsets, const double* h_similarity, const double* h_sh, float* means,
                                    float* scales, float* quats, float* opacities, float* features_dc,
                                    float* features_rest, void* stream) {
    QED_REQUIRE(N >= 1, "N must be at least 1");
    QED_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "SH degree must be in [0, 3]");
    QED_REQUIRE(rows && h_offsets && means && scales && quats && opacities && features_dc, "null buffers");
    QED_REQUIRE(features_rest || sh_degree == 0, "features_rest is null");
    QED_REQUIRE(row_bytes >= 4 && row_bytes <= (1 << 20), "row_bytes out of range");
    const int n_cols = 14 + 3 * sh_rest_count(sh_degree);
    UnpackArgs a;
    a.aligned = ((uintptr_t)rows & 3u) == 0 && (row_bytes & 3) == 0;
    for (int c = 0; c < n_cols; ++c) {
        QED_REQUIRE(h_offsets[c] >= 0 && (int64_t)h_offsets[c] + 4 <= row_bytes, "a column offset lies outside the row");
        a.offsets[c] = h_offsets[c];
        a.aligned = a.aligned && (h_offsets[c] & 3) == 0;
    }
    for (int c = n_cols; c < 14 + 45; ++c) a.offsets[c] = 0;
    FrameChange fc;
    QED_REQUIRE(make_frame_change(h_similarity, h_sh, fc) == QED_OK,
                "h_similarity and h_sh come together, and the scale must be positive and finite");
    a.N = N;
    a.rows = rows;
    a.row_bytes = row_bytes;
    a.means = means; a.scales = scales; a.quats = quats; a.opacities = opacities;
    a.features_dc = features_dc; a.features_rest = features_rest;
    const unsigned grid = (unsigned)pack_blocks(N);
    hipStream_t st = (hipStream_t)stream;
    if (sh_degree == 0) hipLaunchKernelGGL(unpack_kernel<0>, dim3(grid), dim3(kPackThreads), 0, st, a, fc);
    else if (sh_degree == 1) hipLaunchKernelGGL(unpack_kernel<1>, dim3(grid), dim3(kPackThreads), 0, st, a, fc);
    else if (sh_degree == 2) hipLaunchKernelGGL(unpack_kernel<2>, dim3(grid), dim3(kPackThreads), 0, st, a, fc);
    else hipLaunchKernelGGL(unpack_kernel<3>, dim3(grid), dim3(kPackThreads), 0, st, a, fc);
    return check_launch("qed_unpack_gaussians");
}
