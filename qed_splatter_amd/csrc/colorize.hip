// Colouring the initial point cloud: step 2 of the reference's `qed-init-pc` tool (create_init_pointcloud.py:264-390).
//
// Every point is projected into every RGB-D frame; a frame HITS the point when the depth measured at the pixel the
// point rounds to agrees with the point's own depth, and the point's colour is the mean of the colours sampled at its
// hits.  The reference does this frame by frame in NumPy, with index lists and a dozen full-length temporaries; here the
// branchy per-(point, frame) chain is the kernel:
//
//   p = w2c [x y z 1]           fp32; w2c = the OpenCV world-to-camera matrix, inverted on the host in float64 (:59-68)
//   valid_z = isfinite(p.z) && p.z > 1e-6;   u = fx (p.x / z_safe) + cx,  v likewise      (division first: :277-278)
//   candidate: finite u, v;  z <= depth_max;  -0.5 <= u < W - 0.5;  -0.5 <= v < H - 0.5    (:327-337)
//   ui = rint(u) (half to even), bounds re-checked                                          (:342-344)
//   measured = clean(depth[vi, ui] * depth_unit_scale_factor);  hit iff measured > 0 && |measured - z| <= max(tol, rel z)
//   hit: color_sum += (double) float(c / 255) per channel, color_count += 1                 (:358-361)
//
// Launch shape.  One thread per point, one launch per batch of up to kMaxFrames frames.  The point (12 B) and its
// accumulator (24 B of float64 sums + 4 B of count) are read once per launch and written back only if the batch hit, so
// they cost 40 B per point and BATCH, not per frame.  The cameras are kernel arguments: every lane reads the same 16
// floats of a frame, which the compiler turns into scalar loads -- no LDS traffic and no vector registers for them.
// What remains per (point, frame) is ~25 VALU operations and two dependent gathers (4 B of depth; 3 B of colour on a
// hit only): a latency-bound kernel.  So the frames are taken four at a time: the four pixel indices are computed first
// and the four depth gathers are issued UNCONDITIONALLY (a non-candidate lane reads pixel 0 of the frame, one line the
// whole wave shares) before the first is tested, which puts four loads per lane in flight where a branch per frame would
// serialise them.  ~40 VGPRs, so occupancy is bounded by the 256-thread workgroups, not by registers.
//
// Each point owns its accumulator: no atomics, and the float64 sum is taken in frame order whatever the grid or the
// batch split, so results are bit-identical for any batching of the same frame sequence.
//
// c / 255 comes from a 256-entry table of float(k) / 255.0f evaluated by the HOST compiler (IEEE division, the value
// NumPy's uint8 -> float32 / 255.0 gives), copied to LDS per workgroup.
//
// All fp32 arithmetic that decides a hit is written with contraction OFF: NumPy rounds after every operation, and an
// fma in u = fx q + cx would move points across pixel boundaries.  The 4-term dot products use the fma chain a BLAS
// sgemm runs (x m0, then fma y m1, fma z m2, then + m3).
#include "qed_common.h"

#include <cmath>
#include <vector>

namespace qed {

constexpr int kColorizeMaxFrames = 32;      // cameras per launch: 32 x 64 B of kernel arguments

struct ColorizeCam {
    float m[12];                             // rows 0-2 of the OpenCV world-to-camera matrix (fp32 of the float64 inverse)
    float fx, fy, cx, cy;
};

struct ColorizeArgs {
    int N, F, H, W;
    float scale, depth_max, tol_abs, tol_rel;
    ColorizeCam cam[kColorizeMaxFrames];
};

struct U8Table { float v[256]; };
static constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
    return t;
}
__device__ const U8Table g_u8_unit = make_u8_table();

#pragma clang fp contract(off)

// pixel index (v W + u) of the point in the frame of camera c, or -1 when the point is no candidate there; z: its depth
__device__ __forceinline__ int colorize_pixel(const ColorizeCam& c, float x, float y, float z, int H, int W,
                                              float depth_max, float& zc) {
    const float px = __builtin_fmaf(z, c.m[2], __builtin_fmaf(y, c.m[1], x * c.m[0])) + c.m[3];
    const float py = __builtin_fmaf(z, c.m[6], __builtin_fmaf(y, c.m[5], x * c.m[4])) + c.m[7];
    const float pz = __builtin_fmaf(z, c.m[10], __builtin_fmaf(y, c.m[9], x * c.m[8])) + c.m[11];
    zc = pz;
    const bool valid_z = isfinite(pz) && pz > 1e-6f;
    const float z_safe = valid_z ? pz : 1.0f;
    const float u = c.fx * __fdiv_rn(px, z_safe) + c.cx;
    const float v = c.fy * __fdiv_rn(py, z_safe) + c.cy;
    const bool cand = valid_z && isfinite(u) && isfinite(v) && pz <= depth_max && u >= -0.5f && u < (float)W - 0.5f &&
                      v >= -0.5f && v < (float)H - 0.5f;
    if (!cand) return -1;
    const int ui = (int)rintf(u), vi = (int)rintf(v);                 // half to even (np.rint)
    if (ui < 0 || ui >= W || vi < 0 || vi >= H) return -1;
    return vi * W + ui;
}

__device__ __forceinline__ bool colorize_hit(float raw, float scale, float z, float tol_abs, float tol_rel) {
    const float m = raw * scale;                                      // the cleaning of :310-312: non-finite, <= 0 -> 0 (no hit)
    if (!(isfinite(m) && m > 0.0f)) return false;
    const float tol = fmaxf(tol_abs, tol_rel * z);
    return fabsf(m - z) <= tol;
}

__global__ void __launch_bounds__(256)
colorize_accumulate_kernel(const float* __restrict__ points, const float* __restrict__ depth,
                           const unsigned char* __restrict__ color, ColorizeArgs a, double* __restrict__ color_sum,
                           int* __restrict__ color_count) {
    __shared__ float s_unit[256];
    s_unit[threadIdx.x] = g_u8_unit.v[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N) return;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int hits = 0;
    bool loaded = false;
    const size_t frame_px = (size_t)a.H * a.W;
    auto add = [&](int f, int pix) {
        if (!loaded) {                                                // the accumulator is touched only by points that are hit
            s0 = color_sum[3 * i]; s1 = color_sum[3 * i + 1]; s2 = color_sum[3 * i + 2];
            loaded = true;
        }
        const unsigned char* c = color + 3 * ((size_t)f * frame_px + (size_t)pix);
        s0 += (double)s_unit[c[0]]; s1 += (double)s_unit[c[1]]; s2 += (double)s_unit[c[2]];
        ++hits;
    };
    int f = 0;
    for (; f + 4 <= a.F; f += 4) {
        int pix[4]; float zc[4], raw[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pix[j] = colorize_pixel(a.cam[f + j], x, y, z, a.H, a.W, a.depth_max, zc[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[j] = depth[(size_t)(f + j) * frame_px + (size_t)max(pix[j], 0)];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (pix[j] >= 0 && colorize_hit(raw[j], a.scale, zc[j], a.tol_abs, a.tol_rel)) add(f + j, pix[j]);
    }
    for (; f < a.F; ++f) {
        float zc;
        const int pix = colorize_pixel(a.cam[f], x, y, z, a.H, a.W, a.depth_max, zc);
        if (pix >= 0 && colorize_hit(depth[(size_t)f * frame_px + (size_t)pix], a.scale, zc, a.tol_abs, a.tol_rel))
            add(f, pix);
    }
    if (hits) {
        color_sum[3 * i] = s0; color_sum[3 * i + 1] = s1; color_sum[3 * i + 2] = s2;
        color_count[i] += hits;
    }
}

// colors = uint8(clip(sum / count * 255, 0, 255)) in float64, TRUNCATED as NumPy's astype(uint8) does (:378-383)
__global__ void __launch_bounds__(256)
colorize_finalize_kernel(int N, const double* __restrict__ color_sum, const int* __restrict__ color_count,
                         unsigned char* __restrict__ colors, int* __restrict__ n_colored) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int cnt = i < N ? color_count[i] : 0;
    if (i < N) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            unsigned char o = 0;
            if (cnt > 0) {
                const double v = color_sum[3 * i + c] / (double)cnt * 255.0;
                o = (unsigned char)(int)fmin(fmax(v, 0.0), 255.0);
            }
            colors[3 * i + c] = o;
        }
    }
    const unsigned long long m = __ballot(cnt > 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_colored, __popcll(m));
}

// general 4x4 inverse in float64 (Gauss-Jordan, partial pivoting): what np.linalg.inv does to the flipped pose; false if singular
static bool invert4(const double* a, double* inv) {
    double w[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) { w[r][c] = a[4 * r + c]; w[r][4 + c] = r == c ? 1.0 : 0.0; }
    for (int k = 0; k < 4; ++k) {
        int p = k;
        for (int r = k + 1; r < 4; ++r) if (fabs(w[r][k]) > fabs(w[p][k])) p = r;
        if (!(fabs(w[p][k]) > 0.0) || !std::isfinite(w[p][k])) return false;
        if (p != k) for (int c = 0; c < 8; ++c) { const double t = w[k][c]; w[k][c] = w[p][c]; w[p][c] = t; }
        const double d = 1.0 / w[k][k];
        for (int c = 0; c < 8; ++c) w[k][c] *= d;
        for (int r = 0; r < 4; ++r) {
            if (r == k) continue;
            const double f = w[r][k];
            if (f != 0.0) for (int c = 0; c < 8; ++c) w[r][c] -= f * w[k][c];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) inv[4 * r + c] = w[r][4 + c];
    return true;
}

}  // namespace qed

using namespace qed;

extern "C" int qed_colorize_accumulate(int32_t N, const float* points, int32_t F, int32_t height, int32_t width,
                                       const float* depth, float depth_unit_scale_factor, const uint8_t* color,
                                       const double* h_c2w_opengl, const float* h_intrinsics, float depth_max,
                                       float depth_tolerance, float depth_tolerance_rel, double* color_sum,
                                       int32_t* color_count, void* stream) {
    QED_REQUIRE(N >= 0 && F > 0 && height > 0 && width > 0, "bad extents (N >= 0, F >= 1, H, W >= 1)");
    QED_REQUIRE((long long)height * width <= 0x7fffffffLL, "frame too large");
    QED_REQUIRE(h_c2w_opengl && h_intrinsics, "null buffers (host poses / intrinsics)");
    QED_REQUIRE(N == 0 || (points && depth && color && color_sum && color_count), "null buffers");
    for (int f = 0; f < F; ++f)
        QED_REQUIRE(h_intrinsics[4 * f] != 0.f && h_intrinsics[4 * f + 1] != 0.f, "zero focal length");
    std::vector<ColorizeCam> cams((size_t)F);                         // every pose is checked before the first launch
    for (int f = 0; f < F; ++f) {
        double c2w[16], w2c[16];
        for (int k = 0; k < 16; ++k) c2w[k] = h_c2w_opengl[16 * (size_t)f + k];
        for (int r = 0; r < 3; ++r) { c2w[4 * r + 1] = -c2w[4 * r + 1]; c2w[4 * r + 2] = -c2w[4 * r + 2]; }   // :67
        QED_REQUIRE(invert4(c2w, w2c), "singular camera pose");
        for (int k = 0; k < 12; ++k) cams[f].m[k] = (float)w2c[k];
        const float* in = h_intrinsics + 4 * (size_t)f;
        cams[f].fx = in[0]; cams[f].fy = in[1]; cams[f].cx = in[2]; cams[f].cy = in[3];
    }
    if (N == 0) return QED_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t frame_px = (size_t)height * width;
    for (int f0 = 0; f0 < F; f0 += kColorizeMaxFrames) {             // launches on one stream: frame order is kept
        ColorizeArgs a;
        a.N = N; a.F = F - f0 < kColorizeMaxFrames ? F - f0 : kColorizeMaxFrames; a.H = height; a.W = width;
        a.scale = depth_unit_scale_factor; a.depth_max = depth_max;
        a.tol_abs = depth_tolerance; a.tol_rel = depth_tolerance_rel;
        for (int j = 0; j < kColorizeMaxFrames; ++j) a.cam[j] = j < a.F ? cams[f0 + j] : ColorizeCam{};
        hipLaunchKernelGGL(colorize_accumulate_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, points,
                           depth + (size_t)f0 * frame_px, color + 3 * (size_t)f0 * frame_px, a, color_sum, color_count);
    }
    return check_launch("qed_colorize_accumulate");
}

extern "C" int qed_colorize_finalize(int32_t N, const double* color_sum, const int32_t* color_count, uint8_t* colors,
                                     int32_t* n_colored, void* stream) {
    QED_REQUIRE(N >= 0, "bad extents");
    QED_REQUIRE(n_colored && (N == 0 || (color_sum && color_count && colors)), "null buffers");
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(n_colored, 0, sizeof(int32_t), st);          // (an error surfaces in check_launch below)
    if (N == 0) return QED_OK;
    hipLaunchKernelGGL(colorize_finalize_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, N, color_sum,
                       color_count, colors, n_colored);
    return check_launch("qed_colorize_finalize");
}
