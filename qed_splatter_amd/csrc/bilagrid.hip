// Bilateral-grid appearance correction (splatfacto's use_bilateral_grid; nerfstudio 1.1.x lib_bilagrid).
//
// One grid slab [12, L, Y, X] per training image holds a 3x4 affine colour transform at every lattice vertex.  Pixel
// (i, j) of an H x W image is corrected by the transform trilinearly sliced at
//   ix = j (X-1)/(W-1),  iy = i (Y-1)/(H-1),  iz = gray (L-1),  gray = 0.299 r + 0.587 g + 0.114 b,
// which is F.grid_sample(align_corners=True, padding_mode="border") at the coordinates (linspace(0,1,W)-0.5)*2,
// (linspace(0,1,H)-0.5)*2 and 2 gray - 1: out = A[:, :3] rgb + A[:, 3].  The x and y coordinates are implicit (derived
// from the pixel index), so a pixel reads nothing but its rgb.  iz is clipped to [0, L-1]; as in PyTorch the clipped
// coordinate passes no gradient at or beyond either end (gray <= 0 or >= 1).
//
// Slice: a workgroup owns a 64 x 16 pixel tile (4 waves, each a 64-pixel row at a time).  The xy vertices the tile
// touches (all L levels, channel-last [vy][vx][L][12]) are staged in LDS once, so every pixel's 8 x 12 corner reads hit
// LDS.  Backward: the grid gradient is summed on chip before it reaches memory -- inside a wave by a loop over the
// distinct (x cell, z cell) keys of its row (few in a natural image; the row shares its y cell) with a reduce-scatter
// butterfly of the 4 x 12 (x corner, z corner, channel) products, then by LDS atomics into the tile's sub-volume, which
// is flushed with global float atomics (non-zero entries only, 12 L contiguous floats per vertex) into a channel-last
// workspace [Y][X][L][12]; a last pass writes the slab in the Parameter's [12][L][Y][X] layout.  Float atomics: the
// grid gradient is not bitwise reproducible from run to run (it differs in the last bits).  When the tile's sub-volume
// would not fit (grids much finer than the image), the same kernels read the grid and add into the workspace directly.
//
// Total variation: tv = (1/N) sum_{d in L,Y,X} sum((g[d+1] - g[d])^2) / numel(diff_d) over all N grids -- block partials
// and a fixed-order fold (deterministic); its gradient is scaled by a device-resident upstream gradient.
#include "qed_common.h"

namespace qed {

constexpr int kBgTW = 64;              // tile columns: one wave row
constexpr int kBgTH = 16;              // tile rows: 4 waves x 4 rows
constexpr int kBgThreads = 256;
constexpr int kBgStageFloats = 8192;   // largest staged sub-volume (32 KiB); the backward holds two
constexpr int kBgTvBlocks = 1024;      // == QED_BILAGRID_TV_WS_DOUBLES

struct BgArgs {
    int H, W, X, Y, L;
    float sx, sy;                      // (X-1)/(W-1), (Y-1)/(H-1); 0 for a single column / row
    int tiles_x;
    int stage;                         // floats of the largest tile window (the dynamic LDS of one staged volume)
};

__device__ __forceinline__ int bg_cell(float u, int n) { return min((int)u, n - 2); }   // u >= 0: (int) is floor

// The tile's vertex window: [vx0, vx0 + nx) x [vy0, vy0 + ny), all L levels.
struct BgTile {
    int c0, r0, c1, r1;                // pixel columns / rows, inclusive ends
    int vx0, vy0, nx, ny;
};

__device__ __forceinline__ BgTile bg_tile(const BgArgs& a) {
    BgTile t;
    const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    t.c0 = tx * kBgTW; t.r0 = ty * kBgTH;
    t.c1 = min(t.c0 + kBgTW, a.W) - 1; t.r1 = min(t.r0 + kBgTH, a.H) - 1;
    t.vx0 = bg_cell((float)t.c0 * a.sx, a.X);
    t.vy0 = bg_cell((float)t.r0 * a.sy, a.Y);
    t.nx = bg_cell((float)t.c1 * a.sx, a.X) + 2 - t.vx0;
    t.ny = bg_cell((float)t.r1 * a.sy, a.Y) + 2 - t.vy0;
    return t;
}

// Copy the tile's vertices of a [12][L][Y][X] slab into LDS, channel-last.  Consecutive threads read along x.
__device__ __forceinline__ void bg_stage(const float* __restrict__ grid, const BgArgs& a, const BgTile& t,
                                         float* s_vol) {
    const int n = t.nx * t.ny * a.L * 12;
    for (int i = threadIdx.x; i < n; i += kBgThreads) {
        const int vx = i % t.nx;
        int q = i / t.nx;
        const int vy = q % t.ny; q /= t.ny;
        const int l = q % a.L, c = q / a.L;
        s_vol[((vy * t.nx + vx) * a.L + l) * 12 + c] = grid[((size_t)(c * a.L + l) * a.Y + t.vy0 + vy) * a.X + t.vx0 + vx];
    }
}

// The 12 values of vertex (vy, vx, l): from the staged LDS window, or from the slab in global memory.
template <bool STAGED>
__device__ __forceinline__ void bg_load12(const float* vol, const BgArgs& a, const BgTile& t, int vy, int vx, int l,
                                          float v[12]) {
    if (STAGED) {
        const float4* p = reinterpret_cast<const float4*>(vol + (((vy - t.vy0) * t.nx + (vx - t.vx0)) * a.L + l) * 12);
        const float4 u0 = p[0], u1 = p[1], u2 = p[2];
        v[0] = u0.x; v[1] = u0.y; v[2] = u0.z; v[3] = u0.w;
        v[4] = u1.x; v[5] = u1.y; v[6] = u1.z; v[7] = u1.w;
        v[8] = u2.x; v[9] = u2.y; v[10] = u2.z; v[11] = u2.w;
    } else {
        const size_t plane = (size_t)a.L * a.Y * a.X;
        const float* p = vol + ((size_t)l * a.Y + vy) * a.X + vx;
#pragma unroll
        for (int c = 0; c < 12; ++c) v[c] = p[c * plane];
    }
}

// A pixel's lattice cell and fractions.  zgrad: the clipped z coordinate is strictly inside (0, L-1).
struct BgPix {
    int x0, y0, z0;
    float tx, ty, tz;
    bool zgrad;
};

__device__ __forceinline__ BgPix bg_pixel(const BgArgs& a, int row, int col, float r, float g, float b) {
    BgPix p;
    const float ix = (float)col * a.sx, iy = (float)row * a.sy;
    p.x0 = bg_cell(ix, a.X); p.tx = ix - (float)p.x0;
    p.y0 = bg_cell(iy, a.Y); p.ty = iy - (float)p.y0;
    const float z = 2.f * (0.299f * r + 0.587f * g + 0.114f * b) - 1.f;
    float iz = (z + 1.f) * 0.5f * (float)(a.L - 1);
    const float zmax = (float)(a.L - 1);
    p.zgrad = iz > 0.f && iz < zmax;
    iz = iz > 0.f ? (iz < zmax ? iz : zmax) : 0.f;          // (a NaN gray lands on 0, as PyTorch's clip does)
    p.z0 = bg_cell(iz, a.L); p.tz = iz - (float)p.z0;
    return p;
}

// lo / hi: the bilinear xy interpolation at levels z0 and z0 + 1.
template <bool STAGED>
__device__ __forceinline__ void bg_corners(const float* vol, const BgArgs& a, const BgTile& t, const BgPix& p,
                                           float lo[12], float hi[12]) {
    const float w00 = (1.f - p.tx) * (1.f - p.ty), w01 = p.tx * (1.f - p.ty);
    const float w10 = (1.f - p.tx) * p.ty, w11 = p.tx * p.ty;
#pragma unroll
    for (int zc = 0; zc < 2; ++zc) {
        float* acc = zc ? hi : lo;
        float v[12];
        bg_load12<STAGED>(vol, a, t, p.y0, p.x0, p.z0 + zc, v);
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[c] = w00 * v[c];
        bg_load12<STAGED>(vol, a, t, p.y0, p.x0 + 1, p.z0 + zc, v);
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[c] += w01 * v[c];
        bg_load12<STAGED>(vol, a, t, p.y0 + 1, p.x0, p.z0 + zc, v);
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[c] += w10 * v[c];
        bg_load12<STAGED>(vol, a, t, p.y0 + 1, p.x0 + 1, p.z0 + zc, v);
#pragma unroll
        for (int c = 0; c < 12; ++c) acc[c] += w11 * v[c];
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(kBgThreads)
bilagrid_slice_fwd_kernel(const float* __restrict__ rgb, const float* __restrict__ grid, BgArgs a,
                          float* __restrict__ out) {
    extern __shared__ float4 s_dyn[];
    float* s_vol = reinterpret_cast<float*>(s_dyn);
    const BgTile t = bg_tile(a);
    if (STAGED) {
        bg_stage(grid, a, t, s_vol);
        __syncthreads();
    }
    const float* vol = STAGED ? s_vol : grid;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = t.c0 + lane;
    for (int row = t.r0 + wave; row <= t.r1; row += 4) {
        if (col > t.c1) continue;
        const size_t px = (size_t)row * a.W + col;
        const float r = rgb[3 * px], g = rgb[3 * px + 1], b = rgb[3 * px + 2];
        const BgPix p = bg_pixel(a, row, col, r, g, b);
        float lo[12], hi[12];
        bg_corners<STAGED>(vol, a, t, p, lo, hi);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float A[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) A[j] = lo[4 * i + j] + p.tz * (hi[4 * i + j] - lo[4 * i + j]);
            out[3 * px + i] = A[0] * r + A[1] * g + A[2] * b + A[3];
        }
    }
}

// One halving step of the wave's reduce-scatter: lanes with bit M set keep the upper H values, the others the lower H;
// each adds its partner's copy of the half it keeps (lane bits 3 and 2; bits 5 and 4: bg_rs_swap below).
template <int H, int M>
__device__ __forceinline__ void bg_rs_step(float* v, int lane) {
    const bool up = (lane & M) != 0;
#pragma unroll
    for (int i = 0; i < H; ++i) {
        const float send = up ? v[i] : v[i + H];
        const float keep = up ? v[i + H] : v[i];
        v[i] = keep + __shfl_xor(send, M);
    }
}

// The halving steps over lane bits 5 and 4 through v_permlane32_swap / v_permlane16_swap (VALU, no LDS, no select): with
// A = v[i], B = v[i + H] the swap exchanges one half of A's lanes with the partner half of B's, so A' + B' is, in every
// lane, the pair's sum of one of the two values.  Which one a lane keeps follows from the swap's lane convention; it is
// read off once with a probe (0 for a lower-half value, 1 for an upper one) rather than assumed.
template <bool X32>
__device__ __forceinline__ float bg_swap_sum(float a, float b) {
    const auto r = X32 ? __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false)
                       : __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

template <int H, bool X32>
__device__ __forceinline__ void bg_rs_swap(float* v) {
#pragma unroll
    for (int i = 0; i < H; ++i) v[i] = bg_swap_sum<X32>(v[i], v[i + H]);
}

template <bool STAGED>
__global__ void __launch_bounds__(kBgThreads)
bilagrid_slice_bwd_kernel(const float* __restrict__ rgb, const float* __restrict__ grid,
                          const float* __restrict__ v_out, BgArgs a, float* __restrict__ v_rgb,
                          float* __restrict__ ws) {
    extern __shared__ float4 s_dyn[];
    const BgTile t = bg_tile(a);
    const int LC = a.L * 12;
    float* s_vol = reinterpret_cast<float*>(s_dyn);
    float* s_acc = s_vol + a.stage;
    if (STAGED) {
        const int n = t.nx * t.ny * LC;
        for (int i = threadIdx.x; i < n; i += kBgThreads) s_acc[i] = 0.f;
        bg_stage(grid, a, t, s_vol);
        __syncthreads();
    }
    const float* vol = STAGED ? s_vol : grid;
    // accumulation target, channel-last: the tile's LDS window, or the whole workspace [Y][X][L][12]
    float* acc = STAGED ? s_acc : ws;
    const int acc_vx0 = STAGED ? t.vx0 : 0, acc_vy0 = STAGED ? t.vy0 : 0, acc_nx = STAGED ? t.nx : a.X;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = t.c0 + lane;
    const bool in_col = col <= t.c1;
    const int upper32 = bg_swap_sum<true>(0.f, 1.f) > 0.5f, upper16 = bg_swap_sum<false>(0.f, 1.f) > 0.5f;
    const float zscale = (float)(a.L - 1);
    for (int row = t.r0 + wave; row <= t.r1; row += 4) {          // (wave-uniform)
        float r = 0.f, g = 0.f, b = 0.f, g0 = 0.f, g1 = 0.f, g2 = 0.f;
        size_t px = 0;
        if (in_col) {
            px = (size_t)row * a.W + col;
            r = rgb[3 * px]; g = rgb[3 * px + 1]; b = rgb[3 * px + 2];
            g0 = v_out[3 * px]; g1 = v_out[3 * px + 1]; g2 = v_out[3 * px + 2];
        }
        const BgPix p = bg_pixel(a, row, in_col ? col : t.c1, r, g, b);
        float lo[12], hi[12];
        bg_corners<STAGED>(vol, a, t, p, lo, hi);
        const float gv[3] = {g0, g1, g2};
        const float rh[4] = {r, g, b, 1.f};
        float vr[3] = {0.f, 0.f, 0.f};
        float gz = 0.f;                                            // d out / d iz, contracted with v_out
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d = hi[4 * i + j] - lo[4 * i + j];
                gz += gv[i] * d * rh[j];
                if (j < 3) vr[j] += gv[i] * (lo[4 * i + j] + p.tz * d);
            }
        }
        if (in_col) {
            const float gzz = p.zgrad ? gz * zscale : 0.f;         // d iz / d gray = L - 1
            v_rgb[3 * px] = vr[0] + gzz * 0.299f;
            v_rgb[3 * px + 1] = vr[1] + gzz * 0.587f;
            v_rgb[3 * px + 2] = vr[2] + gzz * 0.114f;
        }
        // grid gradient: corner (x0 + xa, y0 + yb, z0 + zc), channel k = 4 i + j gets wx_xa wy_yb wz_zc g_i rh_j.  The
        // row shares y0 and ty, so wy factors out; the wave sums the 4 x 12 (xa, zc, k) products per (x0, z0) key.
        const int key = in_col ? p.x0 * a.L + p.z0 : -1;
        unsigned long long todo = __ballot(in_col);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k_lead = __shfl(key, leader);
            const bool mine = key == k_lead;
            todo &= ~__ballot(mine);
            const float wxz[4] = {(1.f - p.tx) * (1.f - p.tz), (1.f - p.tx) * p.tz, p.tx * (1.f - p.tz), p.tx * p.tz};
            float v[48];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[q * 12 + 4 * i + j] = mine ? wxz[q] * gv[i] * rh[j] : 0.f;
            bg_rs_swap<24, true>(v);
            bg_rs_swap<12, false>(v);
            bg_rs_step<6, 8>(v, lane);
            bg_rs_step<3, 4>(v, lane);
#pragma unroll
            for (int m = 0; m < 3; ++m) {
                v[m] += __shfl_xor(v[m], 2);
                v[m] += __shfl_xor(v[m], 1);
            }
            // lane (lane & 3) == 0 now holds the wave's sums of products base .. base + 2
            const int x0 = __shfl(p.x0, leader), z0 = __shfl(p.z0, leader);
            if ((lane & 3) == 0) {
                const int base = upper32 * 24 + upper16 * 12 + ((lane >> 3) & 1) * 6 + ((lane >> 2) & 1) * 3;
#pragma unroll
                for (int m = 0; m < 3; ++m) {
                    const int idx = base + m, q = idx / 12, k = idx - 12 * q;
                    const int vx = x0 + (q >> 1), l = z0 + (q & 1);
#pragma unroll
                    for (int yb = 0; yb < 2; ++yb) {
                        const float wy = yb ? p.ty : 1.f - p.ty;
                        float* dst = acc + (((p.y0 + yb - acc_vy0) * acc_nx + (vx - acc_vx0)) * a.L + l) * 12 + k;
                        atomicAdd(dst, wy * v[m]);
                    }
                }
            }
        }
    }
    if (STAGED) {
        __syncthreads();
        const int n = t.nx * t.ny * LC;
        for (int i = threadIdx.x; i < n; i += kBgThreads) {
            const float s = s_acc[i];
            if (s == 0.f) continue;
            const int vtx = i / LC, rem = i - vtx * LC;
            const int vx = t.vx0 + vtx % t.nx, vy = t.vy0 + vtx / t.nx;
            atomicAdd(ws + ((size_t)vy * a.X + vx) * LC + rem, s);
        }
    }
}

// workspace [Y][X][L][12] -> slab [12][L][Y][X]
__global__ void __launch_bounds__(256)
bilagrid_grad_layout_kernel(const float* __restrict__ ws, int X, int Y, int L, float* __restrict__ v_grid) {
    const int n = 12 * L * Y * X;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
        const int x = e % X, y = (e / X) % Y, l = (e / (X * Y)) % L, c = e / (X * Y * L);
        v_grid[e] = ws[((y * X + x) * L + l) * 12 + c];
    }
}

// A workgroup iteration covers kTvPlanes (grid, channel, level) planes of Y X floats: every load of the four planes is
// issued before any is used (the pass is bound by memory latency otherwise).  Neighbour offsets are clamped to 0 at an
// edge, where the difference then vanishes, so no load is conditional.
constexpr int kTvPlanes = 4;
static_assert(12 % kTvPlanes == 0, "the plane count 12 N L must be a multiple of kTvPlanes");

struct TvArgs {
    int planes;                        // N 12 L
    int X, Y, L;
    float wx, wy, wl;                  // 1 / (N numel(diff_d)) per direction
};

__global__ void __launch_bounds__(256)
bilagrid_tv_fwd_kernel(const float* __restrict__ g, TvArgs a, double* __restrict__ partials) {
    const int XY = a.X * a.Y;
    float sx = 0.f, sy = 0.f, sl = 0.f;
    for (int p0 = blockIdx.x * kTvPlanes; p0 < a.planes; p0 += gridDim.x * kTvPlanes) {
        for (int i = threadIdx.x; i < XY; i += 256) {
            const int y = i / a.X, x = i - y * a.X;
            const int ox = x + 1 < a.X ? 1 : 0, oy = y + 1 < a.Y ? a.X : 0;
            float v[kTvPlanes], nx[kTvPlanes], ny[kTvPlanes], nl[kTvPlanes];
#pragma unroll
            for (int q = 0; q < kTvPlanes; ++q) {
                const int p = p0 + q;
                const float* gp = g + (size_t)p * XY + i;
                v[q] = gp[0]; nx[q] = gp[ox]; ny[q] = gp[oy]; nl[q] = gp[(p % a.L) + 1 < a.L ? XY : 0];
            }
#pragma unroll
            for (int q = 0; q < kTvPlanes; ++q) {
                const float dx = nx[q] - v[q], dy = ny[q] - v[q], dl = nl[q] - v[q];
                sx += dx * dx; sy += dy * dy; sl += dl * dl;
            }
        }
    }
    const double v[1] = {(double)sx * a.wx + (double)sy * a.wy + (double)sl * a.wl};
    __shared__ double s_w[1][4];
    __shared__ double s[1];
    block_sum_d(v, s_w, s);
    if (threadIdx.x == 0) partials[blockIdx.x] = s[0];
}

// Fixed-order fold of the block partials (one workgroup).
__global__ void __launch_bounds__(256)
bilagrid_tv_fold_kernel(const double* __restrict__ partials, int n, float* __restrict__ out) {
    double v[1] = {0.0};
    for (int i = threadIdx.x; i < n; i += 256) v[0] += partials[i];
    __shared__ double s_w[1][4];
    __shared__ double s[1];
    block_sum_d(v, s_w, s);
    if (threadIdx.x == 0) out[0] = (float)s[0];
}

__global__ void __launch_bounds__(256)
bilagrid_tv_bwd_kernel(const float* __restrict__ g, TvArgs a, const float* __restrict__ v_tv,
                       float* __restrict__ v_g) {
    const int XY = a.X * a.Y;
    const float s = 2.f * v_tv[0];
    for (int p0 = blockIdx.x * kTvPlanes; p0 < a.planes; p0 += gridDim.x * kTvPlanes) {
        for (int i = threadIdx.x; i < XY; i += 256) {
            const int y = i / a.X, x = i - y * a.X;
            const int oxm = x > 0 ? -1 : 0, oxp = x + 1 < a.X ? 1 : 0;
            const int oym = y > 0 ? -a.X : 0, oyp = y + 1 < a.Y ? a.X : 0;
            float r[kTvPlanes];
#pragma unroll
            for (int q = 0; q < kTvPlanes; ++q) {
                const int p = p0 + q, l = p % a.L;
                const float* gp = g + (size_t)p * XY + i;
                const float v = gp[0];
                const float dx = (v - gp[oxm]) - (gp[oxp] - v);
                const float dy = (v - gp[oym]) - (gp[oyp] - v);
                const float dl = (v - gp[l > 0 ? -XY : 0]) - (gp[l + 1 < a.L ? XY : 0] - v);
                r[q] = s * (a.wx * dx + a.wy * dy + a.wl * dl);
            }
#pragma unroll
            for (int q = 0; q < kTvPlanes; ++q) v_g[(size_t)(p0 + q) * XY + i] = r[q];
        }
    }
}

// The fused route's grid step: TV gradient + one slab's data gradient + Adam, all grids in ONE launch.
//
// A workgroup owns one (grid, channel) volume [L][Y][X] -- TV differences never leave it.  It stages the volume in LDS,
// synchronises, forms every element's gradient from the staged (old) values and updates p, m, v in global memory in
// place: each is read once and written once, and no other workgroup reads what this one writes.  The slab workspace
// (the slice backward's channel-last [Y][X][L][12]) is read and zeroed by the 12 workgroups of grid `row`, one channel
// each; with row = -1 the workgroups of grid 0 only zero it.  The arithmetic of the TV gradient is
// bilagrid_tv_bwd_kernel's with v_tv = tv_weight, Adam's is adam.hip's adam_update.
constexpr int kBgStepMaxVolume = QED_BILAGRID_STEP_MAX_VOLUME;   // floats of one staged volume: 64 KiB of LDS

struct BgAdam {
    float beta1, beta2, omb1, omb2, eps, inv_bc1, inv_bc2_sqrt, lr;
};

__device__ __forceinline__ float bg_adam_update(const BgAdam& a, float pp, float gg, float& mm, float& vv) {
    mm = a.beta1 * mm + a.omb1 * gg;
    vv = a.beta2 * vv + a.omb2 * gg * gg;
    const float denom = sqrtf(vv) * a.inv_bc2_sqrt + a.eps;
    return pp - a.lr * a.inv_bc1 * mm / denom;
}

// VEC: X % 4 == 0 and 16-byte aligned buffers -- a thread owns four consecutive x of one row and moves p, m, v as float4.
template <bool VEC>
__global__ void __launch_bounds__(256)
bilagrid_step_kernel(float* __restrict__ grids, float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq, TvArgs a,
                     float tv_scale, int row, float* __restrict__ slab_ws, BgAdam co, float* __restrict__ grad_out,
                     const int* __restrict__ skip) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    extern __shared__ float4 s_dyn[];
    float* s_vol = reinterpret_cast<float*>(s_dyn);
    constexpr int W = VEC ? 4 : 1;
    const int XY = a.X * a.Y, V = XY * a.L;
    const int grid = blockIdx.x / 12, c = blockIdx.x - 12 * grid;
    const size_t base = (size_t)blockIdx.x * V;
    const bool skipped = skip != nullptr && skip[0] != 0;              // (uniform over the launch)
    if (skipped || row < 0) {
        // no slab gradient is consumed: the workspace is handed back zeroed all the same
        if (grid == (row >= 0 ? row : 0))
            for (int i = threadIdx.x; i < V; i += 256) slab_ws[(size_t)i * 12 + c] = 0.f;
        if (skipped) return;
    }
    const bool slab = grid == row;
    if (VEC) {
        const float4* src = reinterpret_cast<const float4*>(grids + base);
        for (int i = threadIdx.x; i < V / 4; i += 256) reinterpret_cast<float4*>(s_vol)[i] = src[i];
    } else {
        for (int i = threadIdx.x; i < V; i += 256) s_vol[i] = grids[base + i];
    }
    __syncthreads();
    for (int i0 = threadIdx.x * W; i0 < V; i0 += 256 * W) {
        float pp[4], mm[4], vv[4], gg[4];
        float* const pm = exp_avg + base + i0;
        float* const pv = exp_avg_sq + base + i0;
        if (VEC) {
            // the moments are touched once per step and by nobody else: non-temporal, as in adam.hip, so that 2 x the
            // grids' size does not displace the Gaussians' parameters from the last-level cache
            const v4f m4 = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(pm));
            const v4f v4 = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(pv));
            mm[0] = m4.x; mm[1] = m4.y; mm[2] = m4.z; mm[3] = m4.w;
            vv[0] = v4.x; vv[1] = v4.y; vv[2] = v4.z; vv[3] = v4.w;
        } else {
            mm[0] = pm[0]; vv[0] = pv[0];
        }
        const int l = i0 / XY, r = i0 - l * XY;
        const int y = r / a.X, x0 = r - y * a.X;
        const int oym = y > 0 ? -a.X : 0, oyp = y + 1 < a.Y ? a.X : 0;
        const int olm = l > 0 ? -XY : 0, olp = l + 1 < a.L ? XY : 0;
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int x = x0 + k;
            const int oxm = x > 0 ? -1 : 0, oxp = x + 1 < a.X ? 1 : 0;
            const float* sp = s_vol + i0 + k;
            const float v = sp[0];
            const float dx = (v - sp[oxm]) - (sp[oxp] - v);
            const float dy = (v - sp[oym]) - (sp[oyp] - v);
            const float dl = (v - sp[olm]) - (sp[olp] - v);
            float g = tv_scale * (a.wx * dx + a.wy * dy + a.wl * dl);
            if (slab) {
                float* w = slab_ws + ((size_t)(y * a.X + x) * a.L + l) * 12 + c;
                g += w[0];
                w[0] = 0.f;
            }
            gg[k] = g;
            pp[k] = bg_adam_update(co, v, g, mm[k], vv[k]);
        }
        if (VEC) {
            *reinterpret_cast<float4*>(grids + base + i0) = make_float4(pp[0], pp[1], pp[2], pp[3]);
            __builtin_nontemporal_store((v4f){mm[0], mm[1], mm[2], mm[3]}, reinterpret_cast<v4f*>(pm));
            __builtin_nontemporal_store((v4f){vv[0], vv[1], vv[2], vv[3]}, reinterpret_cast<v4f*>(pv));
            if (grad_out != nullptr)
                *reinterpret_cast<float4*>(grad_out + base + i0) = make_float4(gg[0], gg[1], gg[2], gg[3]);
        } else {
            grids[base + i0] = pp[0]; pm[0] = mm[0]; pv[0] = vv[0];
            if (grad_out != nullptr) grad_out[base + i0] = gg[0];
        }
    }
}

// Host side ---------------------------------------------------------------------------------------------------------

static int bg_args(int32_t H, int32_t W, int32_t X, int32_t Y, int32_t L, BgArgs& a, bool& staged) {
    QED_REQUIRE(H > 0 && W > 0, "image height and width must be positive");
    QED_REQUIRE((long long)H * W <= (1ll << 30), "image too large");
    QED_REQUIRE(X >= 2 && Y >= 2 && L >= 2, "grid_shape (X, Y, L): every extent must be >= 2");
    QED_REQUIRE((long long)12 * L * Y * X <= (1ll << 30), "grid too large");
    a.H = H; a.W = W; a.X = X; a.Y = Y; a.L = L;
    a.sx = W > 1 ? (float)(X - 1) / (float)(W - 1) : 0.f;
    a.sy = H > 1 ? (float)(Y - 1) / (float)(H - 1) : 0.f;
    a.tiles_x = (W + kBgTW - 1) / kBgTW;
    // the largest vertex window of any tile (bg_tile): floor() moves by at most ceil(span) over a tile, +1 for rounding
    const long long nx = std::min<long long>(X, (long long)ceilf((kBgTW - 1) * a.sx) + 3);
    const long long ny = std::min<long long>(Y, (long long)ceilf((kBgTH - 1) * a.sy) + 3);
    staged = nx * ny * L * 12 <= kBgStageFloats;
    a.stage = staged ? (int)(nx * ny * L * 12) : 0;    // (a multiple of 12 floats: the second volume stays 16-B aligned)
    return QED_OK;
}

}  // namespace qed

using namespace qed;

extern "C" int qed_bilagrid_slice_fwd(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx,
                                      int32_t gy, int32_t gl, float* out, void* stream) {
    BgArgs a;
    bool staged;
    const int rc = bg_args(height, width, gx, gy, gl, a, staged);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(rgb && grid && out, "null buffers");
    const unsigned blocks = (unsigned)(a.tiles_x * ((height + kBgTH - 1) / kBgTH));
    hipStream_t st = (hipStream_t)stream;
    if (staged)
        hipLaunchKernelGGL(bilagrid_slice_fwd_kernel<true>, dim3(blocks), dim3(kBgThreads), a.stage * 4, st,
                           rgb, grid, a, out);
    else
        hipLaunchKernelGGL(bilagrid_slice_fwd_kernel<false>, dim3(blocks), dim3(kBgThreads), 0, st, rgb, grid, a, out);
    return check_launch("qed_bilagrid_slice_fwd");
}

// The slice backward launch: v_rgb written, the slab's gradient ADDED into the channel-last workspace [Y][X][L][12].
static int bg_slice_bwd_launch(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx, int32_t gy,
                               int32_t gl, const float* v_out, float* v_rgb, float* workspace, bool clear, hipStream_t st,
                               const char* who) {
    BgArgs a;
    bool staged;
    const int rc = bg_args(height, width, gx, gy, gl, a, staged);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(rgb && grid && v_out && v_rgb && workspace, "null buffers");
    const unsigned blocks = (unsigned)(a.tiles_x * ((height + kBgTH - 1) / kBgTH));
    if (clear && hipMemsetAsync(workspace, 0, (size_t)12 * gl * gy * gx * sizeof(float), st) != hipSuccess) {
        set_error("%s: memset failed", who);
        return QED_E_LAUNCH;
    }
    if (staged)
        hipLaunchKernelGGL(bilagrid_slice_bwd_kernel<true>, dim3(blocks), dim3(kBgThreads), 2 * a.stage * 4, st,
                           rgb, grid, v_out, a, v_rgb, workspace);
    else
        hipLaunchKernelGGL(bilagrid_slice_bwd_kernel<false>, dim3(blocks), dim3(kBgThreads), 0, st, rgb, grid, v_out, a,
                           v_rgb, workspace);
    return QED_OK;
}

extern "C" int qed_bilagrid_slice_bwd(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx,
                                      int32_t gy, int32_t gl, const float* v_out, float* v_rgb, float* v_grid,
                                      float* workspace, void* stream) {
    QED_REQUIRE(v_grid, "null buffers");
    hipStream_t st = (hipStream_t)stream;
    const int rc = bg_slice_bwd_launch(height, width, rgb, grid, gx, gy, gl, v_out, v_rgb, workspace, true, st,
                                       "qed_bilagrid_slice_bwd");
    if (rc != QED_OK) return rc;
    const int n_grid = 12 * gl * gy * gx;
    hipLaunchKernelGGL(bilagrid_grad_layout_kernel, dim3((unsigned)std::min(1024, (n_grid + 255) / 256)), dim3(256), 0,
                       st, (const float*)workspace, gx, gy, gl, v_grid);
    return check_launch("qed_bilagrid_slice_bwd");
}

extern "C" int qed_bilagrid_slice_bwd_acc(int32_t height, int32_t width, const float* rgb, const float* grid, int32_t gx,
                                          int32_t gy, int32_t gl, const float* v_out, float* v_rgb, float* slab_ws,
                                          void* stream) {
    const int rc = bg_slice_bwd_launch(height, width, rgb, grid, gx, gy, gl, v_out, v_rgb, slab_ws, false,
                                       (hipStream_t)stream, "qed_bilagrid_slice_bwd_acc");
    return rc != QED_OK ? rc : check_launch("qed_bilagrid_slice_bwd_acc");
}

static int tv_args(int32_t n_grids, int32_t gx, int32_t gy, int32_t gl, TvArgs& a) {
    QED_REQUIRE(n_grids > 0, "n_grids must be positive");
    QED_REQUIRE(gx >= 2 && gy >= 2 && gl >= 2, "grid_shape (X, Y, L): every extent must be >= 2");
    QED_REQUIRE((long long)n_grids * 12 * gl < (1ll << 30) && (long long)gy * gx < (1ll << 30), "grids too large");
    const double per = 12.0 * n_grids;
    a.planes = n_grids * 12 * gl;
    a.X = gx; a.Y = gy; a.L = gl;
    a.wx = (float)(1.0 / (n_grids * per * gl * gy * (gx - 1)));
    a.wy = (float)(1.0 / (n_grids * per * gl * (gy - 1) * gx));
    a.wl = (float)(1.0 / (n_grids * per * (gl - 1) * gy * gx));
    return QED_OK;
}

extern "C" int qed_bilagrid_tv_fwd(int32_t n_grids, const float* grids, int32_t gx, int32_t gy, int32_t gl, float* out,
                                   double* workspace, void* stream) {
    TvArgs a;
    const int rc = tv_args(n_grids, gx, gy, gl, a);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(grids && out && workspace, "null buffers");
    const unsigned nb = (unsigned)std::min(kBgTvBlocks, a.planes / kTvPlanes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(bilagrid_tv_fwd_kernel, dim3(nb), dim3(256), 0, st, grids, a, workspace);
    hipLaunchKernelGGL(bilagrid_tv_fold_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, (int)nb, out);
    return check_launch("qed_bilagrid_tv_fwd");
}

extern "C" int qed_bilagrid_tv_bwd(int32_t n_grids, const float* grids, int32_t gx, int32_t gy, int32_t gl,
                                   const float* v_tv, float* v_grids, void* stream) {
    TvArgs a;
    const int rc = tv_args(n_grids, gx, gy, gl, a);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(grids && v_tv && v_grids, "null buffers");
    const unsigned nb = (unsigned)std::min(8 * kBgTvBlocks, a.planes / kTvPlanes);
    hipLaunchKernelGGL(bilagrid_tv_bwd_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, grids, a, v_tv, v_grids);
    return check_launch("qed_bilagrid_tv_bwd");
}

extern "C" int qed_bilagrid_step(int32_t n_grids, float* grids, float* exp_avg, float* exp_avg_sq, int32_t gx, int32_t gy,
                                 int32_t gl, float tv_weight, int32_t row, float* slab_ws, float lr, double beta1,
                                 double beta2, float eps, int32_t step, float* grad_out, const int32_t* skip_flag,
                                 void* stream) {
    TvArgs a;
    const int rc = tv_args(n_grids, gx, gy, gl, a);
    if (rc != QED_OK) return rc;
    QED_REQUIRE((long long)gl * gy * gx <= kBgStepMaxVolume,
                "qed_bilagrid_step: a grid channel (L * Y * X) may hold at most 16384 floats (64 KiB of LDS)");
    QED_REQUIRE(n_grids < (1 << 24), "n_grids < 2^24 required");
    QED_REQUIRE(grids && exp_avg && exp_avg_sq && slab_ws, "null buffers");
    QED_REQUIRE(row >= -1 && row < n_grids, "row must be -1 (no slab gradient this step) or a grid's index");
    QED_REQUIRE(step >= 1, "step is 1-based");
    const BgAdam co{(float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps,
                    (float)(1.0 / (1.0 - pow(beta1, (double)step))), (float)(1.0 / sqrt(1.0 - pow(beta2, (double)step))), lr};
    const int V = gl * gy * gx;
    const uintptr_t bits = (uintptr_t)grids | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)grad_out;
    const bool vec = gx % 4 == 0 && bits % 16 == 0;
    const float tv_scale = 2.f * tv_weight;                       // bilagrid_tv_bwd_kernel's 2 v_tv
    hipStream_t st = (hipStream_t)stream;
    const dim3 blocks((unsigned)n_grids * 12u);
    if (vec)
        hipLaunchKernelGGL(bilagrid_step_kernel<true>, blocks, dim3(256), (size_t)V * 4, st, grids, exp_avg, exp_avg_sq, a,
                           tv_scale, row, slab_ws, co, grad_out, skip_flag);
    else
        hipLaunchKernelGGL(bilagrid_step_kernel<false>, blocks, dim3(256), (size_t)V * 4, st, grids, exp_avg, exp_avg_sq, a,
                           tv_scale, row, slab_ws, co, grad_out, skip_flag);
    return check_launch("qed_bilagrid_step");
}
