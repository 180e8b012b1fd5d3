// Finishing a rendered frame for files: get_outputs' float planes (rgb, depth, accumulation) -> the bytes an image
// writer wants, in one launch, plus the frame's depth range in a launch of its own.  The definitions of every output are
// written out at qed_present_frame in include/qed_splat.h; tests/present_ref.py restates them in NumPy and the GPU tests
// compare to the bit.
//
// qed_present_range.  Minimum and maximum of the valid depths (alpha > 0, depth finite and > 0).  The bit pattern of a
// positive finite float orders as the float does, so workgroups combine through integer atomics on range_out itself, and
// the result is the same whatever the order: a memset zeroes the two words (part of the call), every workgroup reduces
// its pixels in registers and LDS and then issues at most one atomicMax (the maximum; 0 = nothing yet) and one
// compare-and-swap minimum that reads 0 as "nothing yet" -- a valid depth's pattern is never 0.  A frame without a valid
// pixel leaves (0, 0).  Atomics on ONE address are served one after the other at the memory side: a first version with
// 1024 workgroups of 256 threads spent 25 of its 30 us at 1920 x 1080 there.  So the workgroups are few and large (at most
// kRangeMaxGrid of 1024 threads, each thread two quads per pass: kRangeBlockPixels pixels per workgroup and pass, all of
// 1080p in one pass with every load in flight at once), and a workgroup first LOOKS at the word (an agent-scope load): the
// maximum only grows and the minimum, once set, only shrinks, so a value that cannot improve what is there needs no
// atomic.  Larger frames take further passes of the same grid.
//
// qed_present_frame.  A pure stream: 20 bytes in, at most 9 out per pixel.  All planes are contiguous, so a row boundary
// means nothing to the kernel: the frame is a flat stream of n = H W pixels, and a lane's four consecutive pixels (a
// QUAD) lie on one row whenever W % 4 == 0.  What decides the speed of such a kernel is that every load and store
// instruction covers one contiguous range across the wave (ingest.hip measured a factor of five for getting this
// wrong), so:
//   * the colour plane is quantised as what it is, a flat stream of 3 n floats -> 3 n bytes: thread t turns ONE float4
//     (floats 4 t ..) into ONE dword;
//   * the first quarter of those threads (4 t < n) also own pixels 4 t .. 4 t + 3 of the other planes: one float4 of
//     depth and one of alpha in; two dwords of uint16, three dwords of depth map and one dword of alpha out.  Lane strides
//     are 16 / 8 / 12 / 4 bytes: contiguous across the wave.
// Every store on that path is a whole dword.  The last n % 4 pixels (and 3 n % 4 colour bytes) are written by the one
// thread that owns them with byte stores.  If any buffer is not aligned for this (inputs 16 bytes, outputs 4), the whole
// call takes present_pixel_kernel: one thread per pixel, element loads, byte stores, the same arithmetic.
// The colour table (768 bytes, any alignment) is staged in LDS as 256 packed dwords by the workgroups that own pixels.
#include "qed_common.h"

namespace qed {

constexpr int kRangeMaxGrid = 256;                    // workgroups of qed_present_range
constexpr int kRangeThreads = 1024;
constexpr int kRangeBlockPixels = kRangeThreads * 4 * 2;   // pixels of one workgroup per pass: two quads per thread
constexpr int kQuadBlockPixels = 256 * 4;             // pixels owned by one workgroup of present_quad_kernel

#pragma clang fp contract(off)       // every rounding below is the one the header states; the two fused ones are spelled fmaf

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }       // NaN -> 0
__device__ __forceinline__ bool depth_valid(float d, float a) { return a > 0.f && isfinite(d) && d > 0.f; }
__device__ __forceinline__ unsigned quant8(float v) { return (unsigned)floorf(__builtin_fmaf(clamp01(v), 255.f, 0.5f)); }
__device__ __forceinline__ unsigned quant16(float d, float inv_unit) {
    return (unsigned)fminf(floorf(__builtin_fmaf(d, inv_unit, 0.5f)), 65535.f);
}

// the colour of one VALID pixel of the depth map: r | g << 8 | b << 16
__device__ __forceinline__ unsigned depth_colour(float d, float a, float lo, float inv_span, const uint32_t* lut32) {
    const float t = clamp01((d - lo) * inv_span);
    const int k = min(255, (int)(t * 255.f));
    const uint32_t e = lut32[k];
    const float ac = clamp01(a);
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float c = __builtin_fmaf(ac, (float)((e >> (8 * ch)) & 255u) - 255.f, 255.f);
        out |= (unsigned)floorf(c + 0.5f) << (8 * ch);
    }
    return out;
}

struct PresentArgs {
    long long n;                     // H W
    const float* rgb;
    const float* depth;
    const float* alpha;
    const float* range_dev;          // NULL: near / far
    const unsigned char* lut;
    unsigned char* out_rgb8;
    unsigned short* out_depth16;
    unsigned char* out_depthmap8;
    unsigned char* out_alpha8;
    float inv_depth_unit, near, far;
};

__device__ __forceinline__ void stage_lut(const unsigned char* __restrict__ lut, uint32_t* lut32) {
    for (int k = threadIdx.x; k < 256; k += blockDim.x)
        lut32[k] = (uint32_t)lut[3 * k] | ((uint32_t)lut[3 * k + 1] << 8) | ((uint32_t)lut[3 * k + 2] << 16);
    __syncthreads();
}

__device__ __forceinline__ void depth_span(const PresentArgs& a, float& lo, float& inv_span) {
    float hi;
    if (a.range_dev != nullptr) { lo = a.range_dev[0]; hi = a.range_dev[1]; }
    else { lo = a.near; hi = a.far; }
    inv_span = hi > lo ? 1.0f / (hi - lo) : 0.f;
}

__global__ void __launch_bounds__(256) present_quad_kernel(PresentArgs a) {
    __shared__ uint32_t lut32[256];
    const long long n = a.n, n_rgb = 3 * n;
    const bool want_map = a.out_depthmap8 != nullptr;
    // (block-uniform: the workgroup's first quad owns pixels)
    if (want_map && (long long)blockIdx.x * kQuadBlockPixels < n) stage_lut(a.lut, lut32);
    const long long e0 = 4 * ((long long)blockIdx.x * 256 + threadIdx.x);
    // ---- colour: floats e0 .. e0 + 3 of the flat stream
    if (a.out_rgb8 != nullptr && e0 < n_rgb) {
        if (e0 + 4 <= n_rgb) {
            const float4 v = *reinterpret_cast<const float4*>(a.rgb + e0);
            *reinterpret_cast<uint32_t*>(a.out_rgb8 + e0) =
                quant8(v.x) | (quant8(v.y) << 8) | (quant8(v.z) << 16) | (quant8(v.w) << 24);
        } else {
            for (long long i = e0; i < n_rgb; ++i) a.out_rgb8[i] = (unsigned char)quant8(a.rgb[i]);
        }
    }
    if (e0 >= n) return;
    // ---- pixels e0 .. e0 + 3 of the other planes
    const int m = (int)(n - e0 < 4 ? n - e0 : 4);
    float d[4] = {0.f, 0.f, 0.f, 0.f}, al[4] = {0.f, 0.f, 0.f, 0.f};
    const bool want_depth = a.out_depth16 != nullptr || want_map;
    if (m == 4) {
        const float4 av = *reinterpret_cast<const float4*>(a.alpha + e0);
        al[0] = av.x; al[1] = av.y; al[2] = av.z; al[3] = av.w;
        if (want_depth) {
            const float4 dv = *reinterpret_cast<const float4*>(a.depth + e0);
            d[0] = dv.x; d[1] = dv.y; d[2] = dv.z; d[3] = dv.w;
        }
    } else {
        for (int j = 0; j < m; ++j) { al[j] = a.alpha[e0 + j]; if (want_depth) d[j] = a.depth[e0 + j]; }
    }
    if (a.out_alpha8 != nullptr) {
        if (m == 4) *reinterpret_cast<uint32_t*>(a.out_alpha8 + e0) =
                        quant8(al[0]) | (quant8(al[1]) << 8) | (quant8(al[2]) << 16) | (quant8(al[3]) << 24);
        else for (int j = 0; j < m; ++j) a.out_alpha8[e0 + j] = (unsigned char)quant8(al[j]);
    }
    if (a.out_depth16 != nullptr) {
        unsigned q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = depth_valid(d[j], al[j]) ? quant16(d[j], a.inv_depth_unit) : 0u;
        if (m == 4) {
            uint32_t* o = reinterpret_cast<uint32_t*>(a.out_depth16 + e0);
            o[0] = q[0] | (q[1] << 16);
            o[1] = q[2] | (q[3] << 16);
        } else {
            for (int j = 0; j < m; ++j) a.out_depth16[e0 + j] = (unsigned short)q[j];
        }
    }
    if (want_map) {
        float lo, inv_span;
        depth_span(a, lo, inv_span);
        unsigned c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            c[j] = depth_valid(d[j], al[j]) ? depth_colour(d[j], al[j], lo, inv_span, lut32) : 0xffffffu;
        if (m == 4) {
            uint32_t* o = reinterpret_cast<uint32_t*>(a.out_depthmap8 + 3 * e0);
            o[0] = c[0] | (c[1] << 24);
            o[1] = (c[1] >> 8) | (c[2] << 16);
            o[2] = (c[2] >> 16) | (c[3] << 8);
        } else {
            for (int j = 0; j < m; ++j)
                for (int ch = 0; ch < 3; ++ch) a.out_depthmap8[3 * (e0 + j) + ch] = (unsigned char)(c[j] >> (8 * ch));
        }
    }
}

// any alignment: one pixel per thread, element loads and byte stores
__global__ void __launch_bounds__(256) present_pixel_kernel(PresentArgs a) {
    __shared__ uint32_t lut32[256];
    const bool want_map = a.out_depthmap8 != nullptr;
    if (want_map) stage_lut(a.lut, lut32);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    if (a.out_rgb8 != nullptr)
        for (int ch = 0; ch < 3; ++ch) a.out_rgb8[3 * i + ch] = (unsigned char)quant8(a.rgb[3 * i + ch]);
    const float al = a.alpha[i];
    if (a.out_alpha8 != nullptr) a.out_alpha8[i] = (unsigned char)quant8(al);
    if (a.out_depth16 == nullptr && !want_map) return;
    const float d = a.depth[i];
    const bool valid = depth_valid(d, al);
    if (a.out_depth16 != nullptr) a.out_depth16[i] = (unsigned short)(valid ? quant16(d, a.inv_depth_unit) : 0u);
    if (want_map) {
        float lo, inv_span;
        depth_span(a, lo, inv_span);
        const unsigned c = valid ? depth_colour(d, al, lo, inv_span, lut32) : 0xffffffu;
        for (int ch = 0; ch < 3; ++ch) a.out_depthmap8[3 * i + ch] = (unsigned char)(c >> (8 * ch));
    }
}

// range[0] = min, range[1] = max over the valid pixels, as bit patterns (both zeroed before the launch)
__global__ void __launch_bounds__(kRangeThreads) present_range_kernel(long long n, const float* __restrict__ depth,
                                                                      const float* __restrict__ alpha,
                                                                      unsigned* __restrict__ range, int vec) {
    __shared__ unsigned s_lo[kRangeThreads / 64], s_hi[kRangeThreads / 64];
    unsigned lo = 0xffffffffu, hi = 0u;                   // patterns of valid depths lie in [1, 0x7f7fffff]
    auto take = [&](float d, float a) {
        if (depth_valid(d, a)) { const unsigned b = __float_as_uint(d); lo = min(lo, b); hi = max(hi, b); }
    };
    const long long stride = (long long)gridDim.x * kRangeBlockPixels;
    for (long long base = (long long)blockIdx.x * kRangeBlockPixels; base < n; base += stride) {
        const long long e[2] = {base + 4 * (long long)threadIdx.x, base + 4 * (long long)(kRangeThreads + threadIdx.x)};
        if (vec && e[1] + 4 <= n) {                       // both quads whole: four loads in flight
            const float4 d0 = *reinterpret_cast<const float4*>(depth + e[0]), a0 = *reinterpret_cast<const float4*>(alpha + e[0]);
            const float4 d1 = *reinterpret_cast<const float4*>(depth + e[1]), a1 = *reinterpret_cast<const float4*>(alpha + e[1]);
            take(d0.x, a0.x); take(d0.y, a0.y); take(d0.z, a0.z); take(d0.w, a0.w);
            take(d1.x, a1.x); take(d1.y, a1.y); take(d1.z, a1.z); take(d1.w, a1.w);
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q)
                for (long long i = e[q]; i < n && i < e[q] + 4; ++i) take(depth[i], alpha[i]);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, o, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, o, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { s_lo[wid] = lo; s_hi[wid] = hi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 0; w < kRangeThreads / 64; ++w) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
    if (hi == 0u) return;                                 // no valid pixel in this workgroup
    if (hi > __hip_atomic_load(&range[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&range[1], hi);
    // minimum with 0 as "nothing yet": the word only ever goes from 0 to a pattern and then down, so the loop ends
    unsigned seen = __hip_atomic_load(&range[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (seen == 0u || lo < seen) {
        const unsigned assumed = seen;
        seen = atomicCAS(&range[0], assumed, lo);
        if (seen == assumed) break;
    }
}

}  // namespace qed

using namespace qed;

extern "C" int qed_present_range(int32_t height, int32_t width, const float* depth, const float* alpha, float* range_out,
                                 void* stream) {
    QED_REQUIRE(height > 0 && width > 0, "empty frame (height and width must be positive)");
    QED_REQUIRE((long long)height * width <= 0x1fffffffLL, "frame too large");
    QED_REQUIRE(depth && alpha && range_out, "null buffers (depth, alpha, range_out)");
    QED_REQUIRE((((uintptr_t)depth | (uintptr_t)alpha | (uintptr_t)range_out) & 3u) == 0, "buffers must be float-aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)height * width;
    if (hipMemsetAsync(range_out, 0, 2 * sizeof(float), st) != hipSuccess) {
        (void)hipGetLastError();
        set_error("qed_present_range: clearing range_out failed");
        return QED_E_LAUNCH;
    }
    long long grid = (n + kRangeBlockPixels - 1) / kRangeBlockPixels;
    if (grid > kRangeMaxGrid) grid = kRangeMaxGrid;
    const int vec = (((uintptr_t)depth | (uintptr_t)alpha) & 15u) == 0;
    hipLaunchKernelGGL(present_range_kernel, dim3((unsigned)grid), dim3(kRangeThreads), 0, st, n, depth, alpha,
                       reinterpret_cast<unsigned*>(range_out), vec);
    return check_launch("qed_present_range");
}

extern "C" int qed_present_frame(int32_t height, int32_t width, const float* rgb, const float* depth, const float* alpha,
                                 float inv_depth_unit, const float* range_dev, float near, float far, const uint8_t* lut,
                                 uint8_t* out_rgb8, uint16_t* out_depth16, uint8_t* out_depthmap8, uint8_t* out_alpha8,
                                 void* stream) {
    QED_REQUIRE(height > 0 && width > 0, "empty frame (height and width must be positive)");
    QED_REQUIRE((long long)height * width <= 0x1fffffffLL, "frame too large");
    QED_REQUIRE(out_rgb8 || out_depth16 || out_depthmap8 || out_alpha8, "no output plane (all four are NULL)");
    QED_REQUIRE(alpha, "null input buffer (alpha)");
    QED_REQUIRE(!out_rgb8 || rgb, "out_rgb8 needs rgb");
    QED_REQUIRE(!(out_depth16 || out_depthmap8) || depth, "out_depth16 and out_depthmap8 need depth");
    QED_REQUIRE(!out_depthmap8 || lut, "out_depthmap8 needs lut");
    QED_REQUIRE(!out_depth16 || (inv_depth_unit > 0.f && inv_depth_unit <= 3.0e38f), "inv_depth_unit must be positive and finite");
    QED_REQUIRE(!out_depthmap8 || range_dev || (near == near && far == far), "near / far must not be NaN");
    QED_REQUIRE((((uintptr_t)rgb | (uintptr_t)depth | (uintptr_t)alpha | (uintptr_t)range_dev) & 3u) == 0 &&
                ((uintptr_t)out_depth16 & 1u) == 0, "float buffers must be float-aligned, out_depth16 uint16-aligned");
    PresentArgs a;
    a.n = (long long)height * width;
    a.rgb = rgb; a.depth = depth; a.alpha = alpha; a.range_dev = range_dev; a.lut = lut;
    a.out_rgb8 = out_rgb8; a.out_depth16 = out_depth16; a.out_depthmap8 = out_depthmap8; a.out_alpha8 = out_alpha8;
    a.inv_depth_unit = inv_depth_unit; a.near = near; a.far = far;
    hipStream_t st = (hipStream_t)stream;
    const bool in16 = (((uintptr_t)rgb | (uintptr_t)depth | (uintptr_t)alpha) & 15u) == 0;
    const bool out4 = (((uintptr_t)out_rgb8 | (uintptr_t)out_depth16 | (uintptr_t)out_depthmap8 | (uintptr_t)out_alpha8) & 3u) == 0;
    if (in16 && out4) {
        const long long quads = ((out_rgb8 ? 3 * a.n : a.n) + 3) / 4;
        hipLaunchKernelGGL(present_quad_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, a);
    } else {
        hipLaunchKernelGGL(present_pixel_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, st, a);
    }
    return check_launch("qed_present_frame");
}
