// Depth spread of the blending weights along every pixel's ray, its backward pass, and the depth distortion loss on it
// (qed_depth_spread_fwd / qed_depth_spread_bwd / qed_depth_distortion_loss), for gfx950 (wave64).  include/qed_splat.h
// states the definitions: per pixel, over the Gaussians the colour pass applied there, with w_i = alpha_i T_i and z_i the
// record's depth,  A = sum w_i,  m = sum w_i z_i / A,  S = sum w_i (z_i - m)^2,  spread L = A S = sum_{i<j} w_i w_j
// (z_i - z_j)^2 (Mip-NeRF 360's distortion loss in the squared form 2DGS uses for splats),  depth_std = sqrt(S / A).
//
// Why a walk of its own and not two more passes of the compositing kernels with (z, z^2) in the colour slots: L = A D2 - D^2
// from raw moments cancels in float32 exactly where training converges -- on a thin surface (depths 4 +- 0.02) the loss is
// wrong by 20-100 %.  Here every pixel carries a running (A, m_u, S) by the weighted Welford update
//     A' = A + w,  delta = u - m_u,  m_u' = m_u + (w / A') delta,  S' = S + w delta (u - m_u')
// on ANCHORED depths u_i = z_i - z_ref, z_ref = the depth of the tile's first list entry (wave-uniform; the subtraction is
// exact while z_i lies within a factor of two of z_ref, and a tile's Gaussians that matter lie far closer).  Measured
// against float64 on random alpha chains of 5 to 257 entries (numpy float32, depths 4 +- 0.02 and 4 +- 0.5): the loss within
// 1.2e-6 relative, the depth gradient within 1.9e-6; plain Welford on z keeps the loss (3e-5 .. 3e-4) but not the depth
// gradient's bound once m is taken from z.  Chosen over double accumulators: four pixels per lane would hold twelve doubles,
// and fp64 adds issue at a fraction of the fp32 rate in a loop that is issue bound.  Every term added to S is >= 0, the
// first contributor sets m_u = u by a select (not by w / w, which v_rcp_f32 does not make 1), so a pixel with one
// contributor has S = 0 exactly.
//
// Forward: the walk of the compositing forward (composite.hip) without its colours, as importance.hip restates it: one wave
// per 16x16 tile, four pixels per lane (one per 8x8 quadrant), exact-conservative culling per quadrant by ballot, the
// batch's records parked in LDS and fetched by broadcast reads, the two alpha forms chosen per Gaussian by gaussian_is_fast,
// the conic pre-scaled by -log2(e)/2.  The device functions are RESTATED here (not moved to a shared header: the
// compositing kernels' register allocation is tuned to the statement and this file must not be able to move it).  Every
// accept / skip / terminate decision is the one the render made.  A culled or skipped visit leaves (A, m_u, S) bit for bit
// (w = 0 adds exact zeros), so the planes do not depend on QED_CL_NO_CULL.
//
// Backward: back to front from the colour pass's last_ids with its t_final, as K7 walks (T before Gaussian i is T after it
// times 1 / (1 - alpha_i)).  With the upstream per-pixel factor v:  g_i = d / d w_i = v (S + A (u_i - m_u)^2),
// d / d z_i = 2 v A w_i (u_i - m_u),  d / d alpha_i = T_i g_i - (sum_{j>i} w_j g_j) / (1 - alpha_i) -- K7's v_alpha with g_i
// in the place of colour . v_render and no term from T_final (L is a function of the w_i alone) -- then K7's chain to the
// opacity, the conic and the 2-D mean.  A clamped alpha passes nothing.  g_i depends on the pixel, which is why it cannot
// ride in a per-Gaussian colour slot of the compositing backward.
// How the per-Gaussian sums leave the wave: K7's way, not importance.hip's.  The output is a ROW of seven floats per
// Gaussian (slots 0, 1, 4..7, 11 of qed_project_bwd's layout), so the lanes' partials of up to four Gaussians are parked in
// LDS as 28 (Gaussian, value) rows of 64; two lanes per row add them in a fixed order with 16-byte reads, one DPP step joins
// the halves, and the wave issues the rows' atomics in one request.  importance.hip's fold (eight Gaussians, one value each,
// finished inside 8-lane groups, flushed per batch by lane = Gaussian) suits two scalars per Gaussian; with seven values it
// would need seven folds per park and leave each Gaussian's row to one lane, seven single-lane atomics.
// tile_cost / order_ws: taken as qed_composite_bwd takes them (costliest tiles first; QED_CL_ORDER_READY skips the ordering
// launch), but every tile is one whole-tile wave: the walk has half K7's per-visit arithmetic and no colour rows, and the
// quadrant split of the heaviest tiles stages and culls a tile's list four times.
//
// Loss: a reduce pass (masked sum and count per workgroup, as doubles, into the workspace) and a pass that folds those
// partials in a fixed order in every workgroup (qed_reduce.h), writes v = lambda mask / count and, in workgroup 0, the loss.
// No float atomics, no host read-back: the same bits on every run.
#include "qed_common.h"

namespace qed {
namespace {

typedef unsigned long long u64;
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f3 __attribute__((ext_vector_type(3)));

constexpr int kBatch = 64;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kConicScale = -0.5f * kLog2e;
constexpr int kFwdRecFloats = 8;    // {x, y, k a, k b | k b, k c, opacity or its log2, u}
constexpr int kBwdRecFloats = 12;   // {x, y, k a, k b | k b, k c, opacity or its log2, u | list id, -, -, -}
constexpr int kVals = 7;            // per-Gaussian sums of the backward: k v_x, k v_y, conic a, b, c, sum v_sigma, v_depth
constexpr int kParkSlots = 4;       // Gaussians parked per flush: 28 rows, two lanes each
constexpr int kParkStride = 68;     // floats per (Gaussian, value) row: 64 partials + 4 pad (composite.hip's choice: the
                                    // 16-byte reads of the flush then spread over the banks)
constexpr int kParkSlot = kVals * kParkStride;

// ---- restated from composite.hip (same operations in the same order: bit-identical alphas) --------------------------
__device__ __forceinline__ float sel(u64 m, float a, float b) {
    float d;
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(d) : "v"(b), "v"(a), "s"(m));
    return d;
}
__device__ __forceinline__ u64 uniform_u64(u64 v) {
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ bool quadrant_may_touch(const CullGauss& g, int i, int j) {
    const float xl = g.X0 + (float)(8 * i), xh = xl + 7.f, yl = g.Y0 + (float)(8 * j), yh = yl + 7.f;
    auto vline = [&](float X) { const float bb = g.b * X; return edge_min(g.ha * X * X, bb, -bb * g.ic, g.hc, yl, yh); };
    auto hline = [&](float Y) { const float bb = g.b * Y; return edge_min(g.hc * Y * Y, bb, -bb * g.ia, g.ha, xl, xh); };
    const float m = fminf(fminf(vline(xl), vline(xh)), fminf(hline(yl), hline(yh)));
    const bool inside = (xl <= 0.f) & (xh >= 0.f) & (yl <= 0.f) & (yh >= 0.f);
    return inside | !(m > g.thr);
}
__device__ __forceinline__ f2 conic_times_d(f2 R0, f2 R1, f2 d) {
    return __builtin_elementwise_fma(R0, (f2){d.x, d.x}, R1 * (f2){d.y, d.y});
}
__device__ __forceinline__ f3 load_rec_tail(const float4* __restrict__ splats, size_t g) {
    return *reinterpret_cast<const f3*>(&splats[3 * g + 2]);
}
__device__ __forceinline__ bool gaussian_is_fast(float ca, float cb, float cc, float op) {
    return (op <= 0.998f) & (cb * cb <= 0.998f * (ca * cc));
}
__device__ __forceinline__ f2 quadrant_delta(f2 d0, int q) {
    f2 d = d0;
    if (q & 1) d.x -= 8.f;
    if (q >> 1) d.y -= 8.f;
    return d;
}
// per-quadrant survivor masks of the 64 staged Gaussians (one per lane)
__device__ __forceinline__ void quadrant_masks(bool present, const float4& r0, const float4& r1, float tau, float ox,
                                               float oy, bool keep_all, u64* mq) {
    const CullGauss g = cull_setup(r0, r1, tau, ox, oy);
#pragma unroll
    for (int q = 0; q < 4; ++q) mq[q] = __ballot(present & (keep_all | quadrant_may_touch(g, q & 1, q >> 1)));
}

// ================================================================================================
// forward
// ================================================================================================
struct SpreadPixel { float T, A, mu, S; };

// one pixel of one quadrant against the current Gaussian: composite.hip's fwd_quadrant with the Welford update in the place
// of the colours
template <bool MIXED>
__device__ __forceinline__ void spread_quadrant(f2 d, f2 R0, f2 R1, float lo, float u, unsigned slow, u64& done,
                                                SpreadPixel& s) {
    const f2 md = conic_times_d(R0, R1, d);
    float a;
    u64 m_ok;
    if constexpr (MIXED) asm volatile("" : "+s"(slow));
    if (!MIXED || __builtin_expect(slow == 0, 1)) {
        a = __builtin_amdgcn_exp2f(__builtin_fmaf(d.x, md.x, __builtin_fmaf(d.y, md.y, lo)));
        m_ok = __ballot(a >= kAlphaMin) & ~done;
    } else {
        const float p = __builtin_fmaf(d.x, md.x, d.y * md.y);
        a = fminf(kAlphaMax, lo * __builtin_amdgcn_exp2f(p));
        m_ok = __ballot(p <= 0.f) & __ballot(a >= kAlphaMin) & ~done;
    }
    const float at = a * s.T;
    const float nT = s.T - at;
    const u64 m_term = m_ok & __ballot(nT <= kTMin);
    done |= m_term;
    const u64 m_acc = m_ok & ~m_term;
    const float w = sel(m_acc, at, 0.f);
    s.T -= w;
    // weighted Welford on the anchored depth.  The first contributor (A == 0) SETS the mean: w / w through v_rcp_f32 is not
    // 1, and a mean an ulp off u would leave S != 0 at a pixel with one contributor.  A visit with w = 0 changes nothing:
    // r = 0 where A > 0; where A == 0 the mean takes a value that the first contributor overwrites (r may be NaN there: it
    // is not selected)
    const bool first = s.A == 0.f;
    const float An = s.A + w;
    const float r = w * __builtin_amdgcn_rcpf(An);
    const float delta = u - s.mu;
    const float mu_n = first ? u : __builtin_fmaf(r, delta, s.mu);
    s.S = __builtin_fmaf(w * delta, u - mu_n, s.S);
    s.mu = mu_n;
    s.A = An;
}

struct FwdState {
    u64 km, mq[4], done[4];
    SpreadPixel px[4];
};

template <bool MIXED>
__device__ __forceinline__ void fwd_walk(FwdState& w, f2 p0, u64 m_slow, const float (*s_rec)[kFwdRecFloats]) {
    while (w.km) {
        const int t = __builtin_ctzll(w.km);
        const u64 bit = 1ull << t;
        w.km &= ~bit;
        const float4 q0 = *reinterpret_cast<const float4*>(&s_rec[t][0]);      // broadcast: every lane the same record
        const float4 q1 = *reinterpret_cast<const float4*>(&s_rec[t][4]);
        const f2 XY = {q0.x, q0.y}, R0 = {q0.z, q0.w}, R1 = {q1.x, q1.y};
        const f2 d0 = XY - p0;
        const unsigned slow = MIXED ? __builtin_amdgcn_readfirstlane((unsigned)(m_slow >> t) & 1u) : 0u;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(w.mq[q] & bit)) continue;             // wave-uniform: this quadrant cannot see Gaussian t
            spread_quadrant<MIXED>(quadrant_delta(d0, q), R0, R1, q1.z, q1.w, slow, w.done[q], w.px[q]);
            if (w.done[q] == ~0ull) {                   // quadrant finished: drop it from the masks
                w.mq[q] = 0;
                w.km &= w.mq[0] | w.mq[1] | w.mq[2] | w.mq[3];
            }
        }
    }
}

__global__ void __launch_bounds__(64)
depth_spread_fwd_kernel(int C, const float4* __restrict__ splats, const int* __restrict__ flatten_ids,
                        const int* __restrict__ offsets, int width, int height, int tile_w, int tile_h,
                        float* __restrict__ spread, float* __restrict__ mean_u, float* __restrict__ acc,
                        float* __restrict__ depth_std, int keep_all) {
    __shared__ __attribute__((aligned(16))) float s_rec[kBatch][kFwdRecFloats];
    const int n_tiles = tile_w * tile_h;
    const int tile = xcd_remap(blockIdx.x, C * n_tiles);
    const int start = offsets[tile], end = offsets[tile + 1];
    const int cam = tile / n_tiles;
    const int t_in = tile - cam * n_tiles;
    const int ty = t_in / tile_w, tx = t_in - ty * tile_w;
    const int lane = threadIdx.x;
    const int lx = lane & 7, ly = lane >> 3;
    const float ox = (float)(tx * QED_TILE), oy = (float)(ty * QED_TILE);
    const f2 p0 = {(float)(tx * QED_TILE + lx) + 0.5f, (float)(ty * QED_TILE + ly) + 0.5f};

    FwdState w;
    bool inside[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ix = tx * QED_TILE + ((q & 1) << 3) + lx, iy = ty * QED_TILE + ((q >> 1) << 3) + ly;
        inside[q] = ix < width && iy < height;
        w.done[q] = __ballot(!inside[q]);
        w.px[q] = SpreadPixel{1.f, 0.f, 0.f, 0.f};
    }

    // an empty tile reads no list entry (flatten_ids may be NULL) and writes zeros
    if (end > start) {
        const int nb = (end - start + kBatch - 1) / kBatch;
        // the anchor: the depth of the tile's first list entry (wave-uniform; the backward pass reads the same word)
        const float z_ref = reinterpret_cast<const float*>(splats)[12 * (size_t)flatten_ids[start] + 9];
        // the two-deep software pipeline of composite.hip's fwd_tile: unconditional loads from clamped indices
        auto id_at = [&](int idx) { return flatten_ids[idx < end ? idx : end - 1]; };
        int rid_n = id_at(start + kBatch + lane);
        float4 r0, r1;
        f3 r2;
        {
            const size_t g = (size_t)id_at(start + lane);
            r0 = splats[3 * g]; r1 = splats[3 * g + 1]; r2 = load_rec_tail(splats, g);
        }
        bool present = start + lane < end;
        auto all_done = [&]() { return (w.done[0] & w.done[1] & w.done[2] & w.done[3]) == ~0ull; };
        for (int b = 0; b < nb && !all_done(); ++b) {
            // ---- stage this lane's Gaussian: cull per quadrant, pre-scale the conic, anchor the depth ----
            quadrant_masks(present, r0, r1, r2.z, ox, oy, keep_all != 0, w.mq);
#pragma unroll
            for (int q = 0; q < 4; ++q) w.mq[q] = w.done[q] == ~0ull ? 0ull : uniform_u64(w.mq[q]);
            w.km = w.mq[0] | w.mq[1] | w.mq[2] | w.mq[3];
            const bool fast = gaussian_is_fast(r0.z, r0.w, r1.x, r1.y);
            const u64 m_slow = uniform_u64(__ballot(!fast));
            if (w.km) {
                const float bh = kConicScale * r0.w;
                *reinterpret_cast<float4*>(&s_rec[lane][0]) = make_float4(r0.x, r0.y, kConicScale * r0.z, bh);
                *reinterpret_cast<float4*>(&s_rec[lane][4]) =
                    make_float4(bh, kConicScale * r1.x, fast ? __builtin_amdgcn_logf(r1.y) : r1.y, r2.y - z_ref);
            }
            __syncthreads();                            // single wave: orders the stores before the reads below
            // the gather of the next batch (its ids arrived a batch ago) and the id load of the one after
            const size_t g_n = (size_t)rid_n;
            const float4 n0 = splats[3 * g_n], n1 = splats[3 * g_n + 1];
            const f3 n2 = load_rec_tail(splats, g_n);
            const int rid_nn = id_at(start + (b + 2) * kBatch + lane);
            if (m_slow == 0) fwd_walk<false>(w, p0, m_slow, s_rec);
            else fwd_walk<true>(w, p0, m_slow, s_rec);
            r0 = n0; r1 = n1; r2 = n2;                  // rotate the pipeline
            rid_n = rid_nn;
            present = start + (b + 1) * kBatch + lane < end;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!inside[q]) continue;
        const int ix = tx * QED_TILE + ((q & 1) << 3) + lx, iy = ty * QED_TILE + ((q >> 1) << 3) + ly;
        const size_t pix = ((size_t)cam * height + iy) * width + ix;
        const float A = w.px[q].A, S = w.px[q].S;
        spread[pix] = A * S;
        mean_u[pix] = A > 0.f ? w.px[q].mu : 0.f;
        acc[pix] = A;
        if (depth_std != nullptr) depth_std[pix] = A > 0.f ? sqrtf(S / A) : 0.f;
    }
}

// ================================================================================================
// backward
// ================================================================================================
// per-Gaussian gradient accumulators of one lane (summed over its four pixels), in K7's units
struct GradAcc {
    f2 vxy;        // k x (v_x, v_y)            (x 1/k at the flush)
    f2 c01;        // sum v_sigma dx^2 (x 1/2 at the flush), sum v_sigma dx dy
    float c2;      // sum v_sigma dy^2          (x 1/2 at the flush)
    float s0;      // sum v_sigma               (x -1/opacity at the flush)
    float gz;      // v_depth
};

struct BwdPixel {
    float T, bufv;         // transmittance behind the current Gaussian; sum_{j > i} w_j g_j
    float c0, c1, mu;      // v S, v A, m_u
    int bin_final;
};

template <bool MIXED>
__device__ __forceinline__ void bwd_quadrant(f2 d, f2 R0, f2 R1, float lo, float u, int idx, unsigned slow, BwdPixel& s,
                                             u64& any_valid, GradAcc& g) {
    const f2 w = conic_times_d(R0, R1, d);
    float opv, a;
    u64 m_valid, m_vs;
    if constexpr (MIXED) asm volatile("" : "+s"(slow));
    if (!MIXED || __builtin_expect(slow == 0, 1)) {
        opv = a = __builtin_amdgcn_exp2f(__builtin_fmaf(d.x, w.x, __builtin_fmaf(d.y, w.y, lo)));
        m_vs = m_valid = __ballot(s.bin_final >= idx) & __ballot(a >= kAlphaMin);
    } else {
        const float p = __builtin_fmaf(d.x, w.x, d.y * w.y);
        opv = lo * __builtin_amdgcn_exp2f(p);
        a = fminf(kAlphaMax, opv);
        m_valid = __ballot(s.bin_final >= idx) & __ballot(p <= 0.f) & __ballot(a >= kAlphaMin);
        m_vs = m_valid & __ballot(opv <= kAlphaMax);
    }
    any_valid |= m_valid;
    // branch-free, as K7: an invalid pixel has alpha 0, v_rcp_f32(1) = 1 exactly, so its T stays and its weight is 0
    const float a_eff = sel(m_valid, a, 0.f);
    const float ra = __builtin_amdgcn_rcpf(1.f - a_eff);
    const float Tn = s.T * ra;
    s.T = Tn;
    const float fac = a_eff * Tn;                                   // w_i
    const float du = u - s.mu;
    const float cdu = s.c1 * du;
    const float cv = __builtin_fmaf(cdu, du, s.c0);                  // g_i = v (S + A (u_i - m_u)^2)
    g.gz = __builtin_fmaf(2.f * cdu, fac, g.gz);                     // 2 v A w_i (u_i - m_u)
    const float v_a = __builtin_fmaf(Tn, cv, -(ra * s.bufv));
    s.bufv = __builtin_fmaf(fac, cv, s.bufv);
    float vs;
    if (!MIXED || __builtin_expect(slow == 0, 1)) vs = -a_eff * v_a;
    else vs = sel(m_vs, -opv * v_a, 0.f);
    const f2 vv = {vs, vs};
    const f2 sv = d * vv;
    g.vxy += w * vv;
    g.c01 += d * (f2){sv.x, sv.x};
    g.c2 = __builtin_fmaf(sv.y, d.y, g.c2);
    g.s0 += vs;
}

// value k of a parked Gaussian -> its slot of the gradient row, and the conversion K7's flush applies
__device__ __forceinline__ int row_slot(int k) { return k < 2 ? k : (k < 6 ? k + 2 : 11); }
__device__ __forceinline__ float flush_scale(int k, float v, float lo, bool slow) {
    if (k < 2) v *= 1.f / kConicScale;
    else if (k == 2 || k == 4) v *= 0.5f;
    else if (k == 5) v = -v * (slow ? __builtin_amdgcn_rcpf(lo) : __builtin_amdgcn_exp2f(-lo));
    return v;
}

// Flush of the parked Gaussians: two lanes per (Gaussian, value) row add its 64 partials in a fixed order, one lane
// converts, and the wave issues the rows in a single atomic request.  slots: byte s = the batch position of parked Gaussian s.
__device__ __forceinline__ void flush_parked(int n_parked, unsigned slots, u64 m_slow, const float* __restrict__ s_part,
                                             const float (*s_rec)[kBwdRecFloats], float* __restrict__ rows,
                                             unsigned n_rows, int lane) {
    __syncthreads();                                    // single wave: orders the parking stores before these reads
    const int row = lane >> 1, half = lane & 1;         // row = kVals slot + value; lanes 2 row, 2 row + 1 share it
    const int slot = row / kVals, k = row - kVals * slot;
    const bool mine = row < kVals * n_parked;
    float v = 0.f;
    if (mine) {
        const float4* src = reinterpret_cast<const float4*>(s_part + row * kParkStride + 32 * half);
        const float4 a0 = src[0], a1 = src[1], a2 = src[2], a3 = src[3], a4 = src[4], a5 = src[5], a6 = src[6], a7 = src[7];
        const float4 b0 = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
        const float4 b1 = make_float4(a2.x + a3.x, a2.y + a3.y, a2.z + a3.z, a2.w + a3.w);
        const float4 b2 = make_float4(a4.x + a5.x, a4.y + a5.y, a4.z + a5.z, a4.w + a5.w);
        const float4 b3 = make_float4(a6.x + a7.x, a6.y + a7.y, a6.z + a7.z, a6.w + a7.w);
        const float4 c0 = make_float4(b0.x + b1.x, b0.y + b1.y, b0.z + b1.z, b0.w + b1.w);
        const float4 c1 = make_float4(b2.x + b3.x, b2.y + b3.y, b2.z + b3.z, b2.w + b3.w);
        v = ((c0.x + c1.x) + (c0.y + c1.y)) + ((c0.z + c1.z) + (c0.w + c1.w));
    }
    // the other half's 32 partials: lanes l and l ^ 1 (quad_perm [1, 0, 3, 2]); every lane takes part
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, false));
    if (mine && half == 0) {
        const int tg = (int)((slots >> (8 * slot)) & 63u);
        const unsigned id = (unsigned)__float_as_int(s_rec[tg][8]);
        v = flush_scale(k, v, s_rec[tg][6], (m_slow >> tg) & 1);
        if (v != 0.f && id < n_rows) atomicAdd(&rows[(size_t)id * QED_VSPLAT_FLOATS + row_slot(k)], v);
    }
}

struct ParkState { int n; unsigned slots; };

template <bool MIXED>
__device__ __forceinline__ void bwd_walk(u64 km, const u64 (&mq)[4], f2 p0, BwdPixel (&px)[4], int batch_hi, u64 m_slow,
                                         ParkState& park, float* __restrict__ s_part,
                                         const float (*s_rec)[kBwdRecFloats], float* __restrict__ rows, unsigned n_rows,
                                         int lane) {
    while (km) {
        const int t = __builtin_ctzll(km);
        const u64 bit = 1ull << t;
        km &= ~bit;
        const float4 q0 = *reinterpret_cast<const float4*>(&s_rec[t][0]);
        const float4 q1 = *reinterpret_cast<const float4*>(&s_rec[t][4]);
        const f2 XY = {q0.x, q0.y}, R0 = {q0.z, q0.w}, R1 = {q1.x, q1.y};
        const f2 d0 = XY - p0;
        const int idx = batch_hi - t;
        const unsigned slow = MIXED ? __builtin_amdgcn_readfirstlane((unsigned)(m_slow >> t) & 1u) : 0u;
        GradAcc g;
        g.vxy = g.c01 = (f2){0.f, 0.f};
        g.c2 = g.s0 = g.gz = 0.f;
        u64 any_valid = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!(mq[q] & bit)) continue;               // wave-uniform: this quadrant cannot see Gaussian t
            bwd_quadrant<MIXED>(quadrant_delta(d0, q), R0, R1, q1.z, q1.w, idx, slow, px[q], any_valid, g);
        }
        if (any_valid == 0) continue;
        {
            const float gv[kVals] = {g.vxy.x, g.vxy.y, g.c01.x, g.c01.y, g.c2, g.s0, g.gz};
            float* dst = s_part + park.n * kParkSlot + lane;           // [slot][value][lane]
#pragma unroll
            for (int i = 0; i < kVals; ++i) dst[i * kParkStride] = gv[i];
        }
        park.slots |= (unsigned)t << (8 * park.n);
        if (++park.n == kParkSlots) {
            flush_parked(kParkSlots, park.slots, m_slow, s_part, s_rec, rows, n_rows, lane);
            park.n = 0;
            park.slots = 0;
        }
    }
}

__global__ void __launch_bounds__(64)
depth_spread_bwd_kernel(int C, const float4* __restrict__ splats, const int* __restrict__ flatten_ids,
                        const int* __restrict__ offsets, int width, int height, int tile_w, int tile_h,
                        const float* __restrict__ t_final, const int* __restrict__ last_ids,
                        const float* __restrict__ spread, const float* __restrict__ mean_u, const float* __restrict__ acc,
                        const float* __restrict__ v, float* __restrict__ rows, unsigned n_rows, int keep_all,
                        const int* __restrict__ tile_order) {
    __shared__ __attribute__((aligned(16))) float s_part[kParkSlots * kParkSlot];
    __shared__ __attribute__((aligned(16))) float s_rec[kBatch][kBwdRecFloats];
    const int n_tiles = tile_w * tile_h;
    const int n_total = C * n_tiles;
    // costliest first when the caller handed an order (greedy longest-processing-time scheduling, as K7)
    const int tile = tile_order != nullptr ? tile_order[blockIdx.x] : xcd_remap(blockIdx.x, n_total);
    if ((unsigned)tile >= (unsigned)n_total) return;    // (an order that is not a permutation of the tiles)
    const int start = offsets[tile], end = offsets[tile + 1];
    if (end <= start) return;
    const int cam = tile / n_tiles;
    const int t_in = tile - cam * n_tiles;
    const int ty = t_in / tile_w, tx = t_in - ty * tile_w;
    const int lane = threadIdx.x;
    const int lx = lane & 7, ly = lane >> 3;
    const float ox = (float)(tx * QED_TILE), oy = (float)(ty * QED_TILE);
    const f2 p0 = {(float)(tx * QED_TILE + lx) + 0.5f, (float)(ty * QED_TILE + ly) + 0.5f};

    BwdPixel px[4];
    int quad_last[4];
    int tile_last = -1;
    // every load of every quadrant from a CLAMPED pixel address first (all in flight together), then the arithmetic
    bool inside[4];
    float t_in_[4], sp_in[4], mu_in[4], a_in[4], v_in[4];
    int last_in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int ix = tx * QED_TILE + ((q & 1) << 3) + lx, iy = ty * QED_TILE + ((q >> 1) << 3) + ly;
        inside[q] = ix < width && iy < height;
        const size_t pix = ((size_t)cam * height + min(iy, height - 1)) * width + min(ix, width - 1);
        t_in_[q] = t_final[pix];
        last_in[q] = last_ids[pix];
        sp_in[q] = spread[pix];
        mu_in[q] = mean_u[pix];
        a_in[q] = acc[pix];
        v_in[q] = v[pix];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const bool live = inside[q] && a_in[q] > 0.f;
        const float vp = live ? v_in[q] : 0.f;
        px[q].T = inside[q] ? t_in_[q] : 1.f;
        px[q].bufv = 0.f;                               // L is a function of the w_i alone: nothing comes from T_final
        px[q].c0 = live ? vp * (sp_in[q] / a_in[q]) : 0.f;             // v S, S = spread / A
        px[q].c1 = vp * a_in[q];
        px[q].mu = mu_in[q];
        px[q].bin_final = inside[q] ? last_in[q] : -1;
        quad_last[q] = __builtin_amdgcn_readfirstlane(wave_max_i(px[q].bin_final));
        tile_last = max(tile_last, quad_last[q]);
    }
    const int eff_end = min(end, tile_last + 1);
    if (eff_end <= start) return;
    const int nb = (eff_end - start + kBatch - 1) / kBatch;
    const float z_ref = reinterpret_cast<const float*>(splats)[12 * (size_t)flatten_ids[start] + 9];

    // batches run back to front; lane l of batch b gathers sorted index eff_end - 1 - 64 b - l, valid while >= start; the
    // two-deep pipeline of the forward pass (unconditional loads from clamped indices, rotated at the end of the batch)
    auto id_at = [&](int idx) { return flatten_ids[idx > start ? idx : start]; };
    int rid = id_at(eff_end - 1 - lane);
    int rid_n = id_at(eff_end - 1 - kBatch - lane);
    float4 r0 = splats[3 * (size_t)rid], r1 = splats[3 * (size_t)rid + 1];
    f3 r2 = load_rec_tail(splats, (size_t)rid);
    bool present = eff_end - 1 - lane >= start;
    for (int b = 0; b < nb; ++b) {
        const int batch_hi = eff_end - 1 - b * kBatch;  // sorted index gathered by lane 0
        u64 mq[4];
        quadrant_masks(present, r0, r1, r2.z, ox, oy, keep_all != 0, mq);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            mq[q] = uniform_u64(mq[q]);
            // lane t holds sorted index batch_hi - t: beyond every pixel of the quadrant -> cannot be valid
            const int t0 = batch_hi - quad_last[q];
            if (t0 >= kBatch) mq[q] = 0;
            else if (t0 > 0) mq[q] &= ~0ull << t0;
        }
        const u64 km = mq[0] | mq[1] | mq[2] | mq[3];
        const bool fast = gaussian_is_fast(r0.z, r0.w, r1.x, r1.y);
        const u64 m_slow = uniform_u64(__ballot(!fast));
        if (km) {
            const float bh = kConicScale * r0.w;
            *reinterpret_cast<float4*>(&s_rec[lane][0]) = make_float4(r0.x, r0.y, kConicScale * r0.z, bh);
            *reinterpret_cast<float4*>(&s_rec[lane][4]) =
                make_float4(bh, kConicScale * r1.x, fast ? __builtin_amdgcn_logf(r1.y) : r1.y, r2.y - z_ref);
            s_rec[lane][8] = __int_as_float(rid);
        }
        __syncthreads();
        const float4 n0 = splats[3 * (size_t)rid_n], n1 = splats[3 * (size_t)rid_n + 1];
        const f3 n2 = load_rec_tail(splats, (size_t)rid_n);
        const int rid_nn = id_at(batch_hi - 2 * kBatch - lane);
        ParkState park{0, 0u};
        if (m_slow == 0) bwd_walk<false>(km, mq, p0, px, batch_hi, m_slow, park, s_part, s_rec, rows, n_rows, lane);
        else bwd_walk<true>(km, mq, p0, px, batch_hi, m_slow, park, s_part, s_rec, rows, n_rows, lane);
        if (park.n)                                     // before the next batch overwrites s_rec (ids, opacities)
            flush_parked(park.n, park.slots, m_slow, s_part, s_rec, rows, n_rows, lane);
        r0 = n0; r1 = n1; r2 = n2;                      // rotate the pipeline
        rid = rid_n; rid_n = rid_nn;
        present = batch_hi - kBatch - lane >= start;
    }
}

// costliest-first tile order (tile_order_body, qed_common.h) with no tile split: every tile is one whole-tile wave here
__global__ void __launch_bounds__(1024)
spread_tile_order_kernel(TileOrderJob job) {
    __shared__ __attribute__((aligned(8))) int lds[kOrderLdsInts];
    tile_order_body<1024>(job, lds);
}

// ================================================================================================
// the loss
// ================================================================================================
constexpr int kLossGrid = QED_DEPTH_DISTORTION_WS_DOUBLES / 2 - 1;     // workgroups of the reduce pass (256)

// pass 1: per workgroup, the sum of spread over the pixels whose mask is not 0 and their number, as doubles
__global__ void __launch_bounds__(256)
distortion_reduce_kernel(long long n_pix, const float* __restrict__ spread, const float* __restrict__ mask,
                         double* __restrict__ ws) {
    __shared__ double s_w[2][4], s[2];
    double v[2] = {0.0, 0.0};
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (long long)gridDim.x * 256) {
        if (mask == nullptr || mask[i] != 0.f) { v[0] += (double)spread[i]; v[1] += 1.0; }
    }
    block_sum_d<2, 256>(v, s_w, s);
    if (threadIdx.x == 0) { ws[2 * blockIdx.x] = s[0]; ws[2 * blockIdx.x + 1] = s[1]; }
}

// pass 2: every workgroup folds the n_part partials in the same fixed order (thread t owns partial t), then writes
// v = lambda mask / count over its pixels; workgroup 0 also writes the loss and the two totals
__global__ void __launch_bounds__(256)
distortion_finish_kernel(long long n_pix, const float* __restrict__ mask, float lambda, int n_part,
                         double* __restrict__ ws, float* __restrict__ v, float* __restrict__ loss) {
    __shared__ double s_w[2][4], s[2];
    double p[2] = {0.0, 0.0};
    if ((int)threadIdx.x < n_part) { p[0] = ws[2 * threadIdx.x]; p[1] = ws[2 * threadIdx.x + 1]; }
    block_sum_d<2, 256>(p, s_w, s);
    const double sum = s[0], count = s[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ws[2 * kLossGrid] = sum;
        ws[2 * kLossGrid + 1] = count;
        loss[0] = count > 0.0 ? (float)((double)lambda * sum / count) : 0.f;
    }
    if (v == nullptr) return;
    const float scale = count > 0.0 ? (float)((double)lambda / count) : 0.f;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_pix; i += (long long)gridDim.x * 256)
        v[i] = (mask == nullptr || mask[i] != 0.f) ? scale : 0.f;
}

int check_walk_args(const char* who, int C, int N, int width, int height, int tile_w, int tile_h) {
    if (!(C >= 1 && N >= 0 && width > 0 && height > 0)) {
        set_error("%s: bad extents", who);
        return QED_E_INVALID_ARG;
    }
    if (!(tile_w == (width + QED_TILE - 1) / QED_TILE && tile_h == (height + QED_TILE - 1) / QED_TILE)) {
        set_error("%s: tile grid does not match the image (tile size is 16)", who);
        return QED_E_INVALID_ARG;
    }
    if ((long long)C * tile_w * tile_h >= (1ll << 29) || (long long)C * N >= (1ll << 31)) {
        set_error("%s: too many tiles or records", who);
        return QED_E_INVALID_ARG;
    }
    return QED_OK;
}

}  // namespace
}  // namespace qed

using namespace qed;

extern "C" int qed_depth_spread_fwd(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids,
                                    const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                    float* spread, float* mean_u, float* acc, float* depth_std, int32_t launch_flags,
                                    void* stream) {
    const int rc = check_walk_args("qed_depth_spread_fwd", C, N, width, height, tile_w, tile_h);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(offsets && spread && mean_u && acc, "null buffers");
    QED_REQUIRE(N == 0 || splats, "null splat buffer");
    const long long n_pix = (long long)C * width * height;
    hipStream_t st = (hipStream_t)stream;
    if (N == 0 || flatten_ids == nullptr) {
        // no record or an empty sorted list (offsets are then all zero): every plane is zero
        (void)hipMemsetAsync(spread, 0, sizeof(float) * n_pix, st);
        (void)hipMemsetAsync(mean_u, 0, sizeof(float) * n_pix, st);
        (void)hipMemsetAsync(acc, 0, sizeof(float) * n_pix, st);
        if (depth_std != nullptr) (void)hipMemsetAsync(depth_std, 0, sizeof(float) * n_pix, st);
        return check_launch("qed_depth_spread_fwd");
    }
    const long long grid = (long long)C * tile_w * tile_h;
    hipLaunchKernelGGL(depth_spread_fwd_kernel, dim3((unsigned)grid), dim3(64), 0, st, C, (const float4*)splats,
                       flatten_ids, offsets, width, height, tile_w, tile_h, spread, mean_u, acc, depth_std,
                       (launch_flags & QED_CL_NO_CULL) ? 1 : 0);
    return check_launch("qed_depth_spread_fwd");
}

extern "C" int qed_depth_spread_bwd(int32_t C, int32_t N, const float* splats, const int32_t* flatten_ids,
                                    const int32_t* offsets, int32_t width, int32_t height, int32_t tile_w, int32_t tile_h,
                                    const float* t_final, const int32_t* last_ids, const float* spread,
                                    const float* mean_u, const float* acc, const float* v, float* rows,
                                    const int32_t* tile_cost, int32_t* order_ws, int32_t launch_flags, void* stream) {
    const int rc = check_walk_args("qed_depth_spread_bwd", C, N, width, height, tile_w, tile_h);
    if (rc != QED_OK) return rc;
    QED_REQUIRE(offsets && t_final && last_ids && spread && mean_u && acc && v, "null buffers");
    QED_REQUIRE((tile_cost == nullptr) == (order_ws == nullptr), "tile_cost and order_ws go together");
    QED_REQUIRE(((uintptr_t)tile_cost & 15) == 0, "tile_cost must be 16-byte aligned");
    if (N == 0 || flatten_ids == nullptr) return QED_OK;         // nothing was composited: no gradient
    QED_REQUIRE(splats && rows, "null splat buffers");
    const long long grid = (long long)C * tile_w * tile_h;
    hipStream_t st = (hipStream_t)stream;
    const int* tile_order = nullptr;
    // a forced launch shape (test hook of the compositing kernels) keeps the plain tile order, as there
    if (tile_cost != nullptr && (launch_flags & 3) == 0) {
        if (!(launch_flags & QED_CL_ORDER_READY)) {
            TileOrderJob job = tile_order_job(tile_cost, grid, order_ws);
            job.max_split = 0;                                   // no tile is split: the order is a plain permutation
            hipLaunchKernelGGL(spread_tile_order_kernel, dim3(1), dim3(1024), 0, st, job);
        }
        tile_order = order_ws;
    }
    hipLaunchKernelGGL(depth_spread_bwd_kernel, dim3((unsigned)grid), dim3(64), 0, st, C, (const float4*)splats,
                       flatten_ids, offsets, width, height, tile_w, tile_h, t_final, last_ids, spread, mean_u, acc, v, rows,
                       (unsigned)((long long)C * N), (launch_flags & QED_CL_NO_CULL) ? 1 : 0, tile_order);
    return check_launch("qed_depth_spread_bwd");
}

extern "C" int qed_depth_distortion_loss(int64_t n_pix, const float* spread, const float* mask, float lambda,
                                         double* workspace, float* v, float* loss, void* stream) {
    QED_REQUIRE(n_pix >= 0, "bad extents");
    QED_REQUIRE(workspace && loss, "null buffers");
    QED_REQUIRE(n_pix == 0 || spread, "null spread plane");
    QED_REQUIRE(lambda >= 0.f && lambda <= 3.0e38f, "lambda must be a finite number >= 0");
    hipStream_t st = (hipStream_t)stream;
    const unsigned g1 = stream_grid(n_pix, kLossGrid);
    hipLaunchKernelGGL(distortion_reduce_kernel, dim3(g1), dim3(256), 0, st, (long long)n_pix, spread, mask, workspace);
    const unsigned g2 = v != nullptr ? stream_grid(n_pix) : 1u;
    hipLaunchKernelGGL(distortion_finish_kernel, dim3(g2), dim3(256), 0, st, (long long)n_pix, mask, lambda, (int)g1,
                       workspace, v, loss);
    return check_launch("qed_depth_distortion_loss");
}
