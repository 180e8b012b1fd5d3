// The per-step ground truth of a training frame, in one launch: what get_gt_img + composite_with_background + the loss
// mask make of a cached dataset frame (the parent's uint8 image cache, config.py:34-38 / model.py:210-212 of the
// reference).  A trainer hands the model a DIFFERENT uint8 image every step, so nothing of this can be memoised
// across steps; the eager chain (.float(), / 255, a box-filter conv2d with a fresh weight tensor, the RGBA composite,
// .contiguous(), and the same again for depth and mask) is several passes over the frame.  Here it is one.
//
// Outputs, for the box factor d (1..8) and Ho = H / d, Wo = W / d (remainder rows / columns dropped, as a stride-d
// convolution drops them):
//   gt_rgb  [Ho,Wo,3]  mean over the d x d block of every channel; uint8 values scaled by 1/255 (ONE multiplication of
//                      the exact integer sum by 1 / (255 d^2)); with 4 channels the four means are taken first and then
//                      rgb = a rgb + (1 - a) background -- the order of the eager path, NOT a per-pixel composite
//   gt_depth [Ho,Wo]   mean over the block, zeros included (the reference's behaviour); uint16 values are summed as
//                      integers and multiplied once by depth_scale / d^2.  Optional: a float32 depth map at d = 1 IS its
//                      ground truth, and the host layer leaves the plane out instead of copying it
//   mask    [Ho,Wo]    mean of (byte != 0) over the block, when a mask is given
// Integer sums are exact (255 x 64 and 65535 x 64 < 2^24).  At d = 1 a uint8 value k becomes float(k) * (1.0f / 255.0f):
// torch's true-divide by a host scalar multiplies by the float reciprocal, and the eager path's result is reproduced
// bit for bit.  Float inputs are summed in row-major order of the block and multiplied by 1 / d^2 (exact).
//
// Launch shape.  A streaming kernel: 6 MB in, 25 MB out at 1920 x 1080 with d = 1.  What decides its speed is that every
// load and store INSTRUCTION covers one contiguous range across the wave: a first version gave each thread four output
// pixels (12 contiguous input bytes, 48 contiguous output bytes per lane) and ran at 1 TB/s -- three dwordx4 stores at a
// lane stride of 48 B each touch three times the cache lines they fill.  So a lane moves at most 16 contiguous bytes per
// instruction and neighbouring lanes take neighbouring ranges:
//   * ingest_flat_kernel (uint8 RGB, d = 1, the full-resolution steps): the image is a flat stream, a thread turns one
//     dword into one float4; the first quarter of the threads also convert four pixels of depth and mask;
//   * ingest_kernel<image type, channels, depth type, d> for d in {1, 2, 4}: one output pixel per thread; per input row it
//     reads d C contiguous bytes (3 .. 16) and writes 12 B of gt_rgb, 4 B of gt_depth.
// uint8 rows of 3 W bytes start at any byte offset, so a thread reads the ALIGNED dwords that cover its bytes (adjacent
// dword loads, joined by the compiler where it may) and shifts the stream into place with v_alignbit; a dword that
// would straddle the end of the buffer is assembled from guarded byte loads instead.  No LDS, no atomics, plain stores.
// Any other d, or a buffer that is not dword-aligned, takes ingest_generic_kernel: one thread per output pixel,
// element-wise loads, the same sums in the same order.
#include "qed_common.h"

namespace qed {

struct IngestArgs {
    int H, W, Ho, Wo;
    const void* image;
    const void* depth;               // NULL: no depth plane
    const unsigned char* mask;       // NULL: no mask
    const float* background;         // [3]
    float* gt_rgb;
    float* gt_depth;
    float* gt_mask;
    float image_scale;               // 1 / (255 d^2) for uint8, 1 / d^2 for float
    float depth_scale;               // depth_unit_scale / d^2 for uint16, 1 / d^2 for float
    float inv_area;                  // 1 / d^2
};

constexpr int kIngestFlat = 4;       // output floats per thread of ingest_flat_kernel

#pragma clang fp contract(off)       // the composite is a x rgb + (1 - a) x background with every product rounded, as eager

// ND dwords of the byte stream that starts at byte b0 (< total) of the dword-aligned buffer `base` of `total` bytes;
// bytes at or beyond `total` read as 0
template <int ND>
__device__ __forceinline__ void load_window(const unsigned char* __restrict__ base, size_t total, size_t b0,
                                            uint32_t (&out)[ND]) {
    const size_t a0 = b0 & ~(size_t)3;
    const unsigned sh = (unsigned)(b0 & 3) * 8u;
    uint32_t w[ND + 1];
    if (a0 + 4 * (size_t)(ND + 1) <= total) {
        const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(base + a0);
#pragma unroll
        for (int k = 0; k <= ND; ++k) w[k] = p[k];
    } else {
#pragma unroll
        for (int k = 0; k <= ND; ++k) {
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t o = a0 + 4 * (size_t)k + j;
                if (o < total) v |= (uint32_t)base[o] << (8 * j);
            }
            w[k] = v;
        }
    }
#pragma unroll
    for (int k = 0; k < ND; ++k) out[k] = (uint32_t)((((uint64_t)w[k + 1] << 32) | (uint64_t)w[k]) >> sh);
}

// NF floats from element e0 (< total) of `base`; elements at or beyond `total` read as 0
template <int NF>
__device__ __forceinline__ void load_floats(const float* __restrict__ base, size_t total, size_t e0, float (&out)[NF]) {
    if (e0 + NF <= total) {
#pragma unroll
        for (int k = 0; k < NF; ++k) out[k] = base[e0 + k];
    } else {
#pragma unroll
        for (int k = 0; k < NF; ++k) out[k] = e0 + k < total ? base[e0 + k] : 0.f;
    }
}

// the channel means m[0..C) of one output pixel -> its three ground-truth colours
template <int C>
__device__ __forceinline__ void ingest_colour(const float* m, const float* bg, float* o) {
    if constexpr (C == 4) {
        const float a = m[3], na = 1.f - a;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = a * m[c] + na * bg[c];
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = m[c];
    }
}

// one output pixel (x, y) per thread: its d x d block of every plane
template <bool IMG_F32, int C, bool DEPTH_F32, int D>
__global__ void __launch_bounds__(256) ingest_kernel(IngestArgs a) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;                // (H W < 2^29: 32-bit index arithmetic)
    if (t >= (unsigned)a.Ho * (unsigned)a.Wo) return;
    const int y = (int)(t / (unsigned)a.Wo), x = (int)(t % (unsigned)a.Wo);
    const size_t n_px = (size_t)a.H * a.W;
    // first input pixel of block row dy
    auto row = [&](int dy) { return (size_t)(y * D + dy) * a.W + (size_t)x * D; };

    // ---- colour: the channel means, then the composite
    float m[C];
    if constexpr (IMG_F32) {
        float s[C] = {};
#pragma unroll
        for (int dy = 0; dy < D; ++dy) {
            float v[D * C];
            load_floats<D * C>(static_cast<const float*>(a.image), n_px * C, row(dy) * C, v);
#pragma unroll
            for (int i = 0; i < D * C; ++i) s[i % C] += v[i];
        }
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = s[c] * a.image_scale;
    } else {
        constexpr int ND = (D * C + 3) / 4;
        uint32_t s[C] = {};
#pragma unroll
        for (int dy = 0; dy < D; ++dy) {
            uint32_t w[ND];
            load_window<ND>(static_cast<const unsigned char*>(a.image), n_px * C, row(dy) * C, w);
#pragma unroll
            for (int i = 0; i < D * C; ++i) s[i % C] += (w[i >> 2] >> (8 * (i & 3))) & 255u;
        }
#pragma unroll
        for (int c = 0; c < C; ++c) m[c] = (float)s[c] * a.image_scale;
    }
    const float bg[3] = {a.background[0], a.background[1], a.background[2]};
    float rgb[3];
    ingest_colour<C>(m, bg, rgb);
    float* __restrict__ o_rgb = a.gt_rgb + (size_t)t * 3;
    o_rgb[0] = rgb[0]; o_rgb[1] = rgb[1]; o_rgb[2] = rgb[2];

    // ---- depth (without a depth plane a float32 map at d = 1 is its own ground truth: the caller keeps using it)
    if (a.depth != nullptr) {
        float dep;
        if constexpr (DEPTH_F32) {
            float s = 0.f;
#pragma unroll
            for (int dy = 0; dy < D; ++dy) {
                float v[D];
                load_floats<D>(static_cast<const float*>(a.depth), n_px, row(dy), v);
#pragma unroll
                for (int i = 0; i < D; ++i) s += v[i];
            }
            dep = s * a.depth_scale;
        } else {
            constexpr int ND = (D + 1) / 2;
            uint32_t s = 0;
#pragma unroll
            for (int dy = 0; dy < D; ++dy) {
                uint32_t w[ND];
                load_window<ND>(static_cast<const unsigned char*>(a.depth), n_px * 2, row(dy) * 2, w);
#pragma unroll
                for (int i = 0; i < D; ++i) s += (w[i >> 1] >> (16 * (i & 1))) & 0xffffu;
            }
            dep = (float)s * a.depth_scale;
        }
        a.gt_depth[t] = dep;
    }

    // ---- mask
    if (a.mask != nullptr) {
        constexpr int ND = (D + 3) / 4;
        uint32_t s = 0;
#pragma unroll
        for (int dy = 0; dy < D; ++dy) {
            uint32_t w[ND];
            load_window<ND>(a.mask, n_px, row(dy), w);
#pragma unroll
            for (int i = 0; i < D; ++i) s += ((w[i >> 2] >> (8 * (i & 3))) & 255u) != 0u ? 1u : 0u;
        }
        a.gt_mask[t] = (float)s * a.inv_area;
    }
}

// uint8 RGB at d = 1: the image is a flat stream, output float i = input byte i times 1/255.  A thread turns ONE aligned
// dword into one float4 (4 B in, 16 B out per lane, both contiguous across the wave); the first quarter of the threads
// do the same for four pixels of the depth plane (uint16: 8 B in; float32: 16 B) and of the mask (4 B in).
__global__ void __launch_bounds__(256) ingest_flat_kernel(IngestArgs a, int depth_f32) {
    const size_t n_px = (size_t)a.H * a.W, n_rgb = 3 * n_px;
    const size_t e0 = 4 * ((size_t)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= n_rgb) return;
    {
        uint32_t w[1];
        load_window<1>(static_cast<const unsigned char*>(a.image), n_rgb, e0, w);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (float)((w[0] >> (8 * j)) & 255u) * a.image_scale;
        if (e0 + 4 <= n_rgb) *reinterpret_cast<float4*>(a.gt_rgb + e0) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int j = 0; e0 + j < n_rgb; ++j) a.gt_rgb[e0 + j] = v[j];
    }
    if (e0 >= n_px) return;
    const int n = (int)(n_px - e0 < 4 ? n_px - e0 : 4);
    if (a.depth != nullptr) {
        float v[4];
        if (depth_f32) {
            load_floats<4>(static_cast<const float*>(a.depth), n_px, e0, v);
        } else {
            uint32_t w[2];
            load_window<2>(static_cast<const unsigned char*>(a.depth), 2 * n_px, 2 * e0, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = (float)((w[j >> 1] >> (16 * (j & 1))) & 0xffffu) * a.depth_scale;
        }
        if (n == 4) *reinterpret_cast<float4*>(a.gt_depth + e0) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int j = 0; j < n; ++j) a.gt_depth[e0 + j] = v[j];
    }
    if (a.mask != nullptr) {
        uint32_t w[1];
        load_window<1>(a.mask, n_px, e0, w);
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = ((w[0] >> (8 * j)) & 255u) != 0u ? 1.f : 0.f;
        if (n == 4) *reinterpret_cast<float4*>(a.gt_mask + e0) = make_float4(v[0], v[1], v[2], v[3]);
        else for (int j = 0; j < n; ++j) a.gt_mask[e0 + j] = v[j];
    }
}

// any d in 1..8, any alignment: one thread per output pixel, the same sums in the same order
__global__ void __launch_bounds__(256) ingest_generic_kernel(IngestArgs a, int d, int C, int img_f32, int depth_f32) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)a.Ho * a.Wo) return;
    const int y = (int)(i / a.Wo), x = (int)(i % a.Wo);
    const unsigned char* __restrict__ img8 = static_cast<const unsigned char*>(a.image);
    const float* __restrict__ img32 = static_cast<const float*>(a.image);
    const unsigned short* __restrict__ dep16 = static_cast<const unsigned short*>(a.depth);
    const float* __restrict__ dep32 = static_cast<const float*>(a.depth);
    uint32_t is[4] = {0, 0, 0, 0}, ids = 0, ims = 0;
    float fs[4] = {0.f, 0.f, 0.f, 0.f}, fds = 0.f;
    for (int dy = 0; dy < d; ++dy)
        for (int dx = 0; dx < d; ++dx) {
            const size_t px = (size_t)(y * d + dy) * a.W + (size_t)(x * d + dx);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) {
                    if (img_f32) fs[c] += img32[px * C + c];
                    else is[c] += img8[px * C + c];
                }
            if (a.depth != nullptr) {
                if (depth_f32) fds += dep32[px];
                else ids += dep16[px];
            }
            if (a.mask != nullptr) ims += a.mask[px] != 0 ? 1u : 0u;
        }
    float m[4], o[3];
#pragma unroll
    for (int c = 0; c < 4; ++c) m[c] = (img_f32 ? fs[c] : (float)is[c]) * a.image_scale;
    const float bg[3] = {a.background[0], a.background[1], a.background[2]};
    if (C == 4) ingest_colour<4>(m, bg, o);
    else ingest_colour<3>(m, bg, o);
    a.gt_rgb[3 * i] = o[0]; a.gt_rgb[3 * i + 1] = o[1]; a.gt_rgb[3 * i + 2] = o[2];
    if (a.depth != nullptr) a.gt_depth[i] = (depth_f32 ? fds : (float)ids) * a.depth_scale;
    if (a.mask != nullptr) a.gt_mask[i] = (float)ims * a.inv_area;
}

template <bool IMG_F32, int C, bool DEPTH_F32>
static void launch_ingest(const IngestArgs& a, int d, unsigned grid, hipStream_t st) {
    if (d == 1) hipLaunchKernelGGL((ingest_kernel<IMG_F32, C, DEPTH_F32, 1>), dim3(grid), dim3(256), 0, st, a);
    else if (d == 2) hipLaunchKernelGGL((ingest_kernel<IMG_F32, C, DEPTH_F32, 2>), dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((ingest_kernel<IMG_F32, C, DEPTH_F32, 4>), dim3(grid), dim3(256), 0, st, a);
}

}  // namespace qed

using namespace qed;

extern "C" int qed_ingest_ground_truth(int32_t height, int32_t width, int32_t d, const void* image, int32_t channels,
                                       int32_t image_is_f32, const void* depth, int32_t depth_is_f32, float depth_scale,
                                       const uint8_t* mask, const float* background, float* gt_rgb, float* gt_depth,
                                       float* gt_mask, void* stream) {
    QED_REQUIRE(d >= 1 && d <= 8, "d (the box factor) must be in 1..8");
    QED_REQUIRE(channels == 3 || channels == 4, "channels must be 3 or 4");
    QED_REQUIRE(height >= 0 && width >= 0 && height / d > 0 && width / d > 0, "empty output (height / d or width / d is 0)");
    QED_REQUIRE((long long)height * width <= 0x1fffffffLL, "frame too large");
    QED_REQUIRE(gt_rgb && (depth == nullptr || gt_depth) && (mask == nullptr || gt_mask), "null output buffers");
    QED_REQUIRE(image && background, "null input buffers (image, background)");
    IngestArgs a;
    a.H = height; a.W = width; a.Ho = height / d; a.Wo = width / d;
    a.image = image; a.depth = depth; a.mask = mask; a.background = background;
    a.gt_rgb = gt_rgb; a.gt_depth = gt_depth; a.gt_mask = gt_mask;
    a.inv_area = 1.0f / (float)(d * d);
    a.image_scale = image_is_f32 ? a.inv_area : 1.0f / (float)(255 * d * d);
    a.depth_scale = depth_is_f32 ? a.inv_area : depth_scale * a.inv_area;
    hipStream_t st = (hipStream_t)stream;
    const bool aligned = (((uintptr_t)image | (uintptr_t)depth | (uintptr_t)mask) & 3u) == 0;
    const bool out16 = (((uintptr_t)gt_rgb | (uintptr_t)gt_depth | (uintptr_t)gt_mask) & 15u) == 0;
    if (aligned && out16 && d == 1 && channels == 3 && !image_is_f32) {
        const long long threads = (3LL * height * width + kIngestFlat - 1) / kIngestFlat;
        hipLaunchKernelGGL(ingest_flat_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a,
                           (int)(depth_is_f32 != 0));
    } else if (aligned && (d == 1 || d == 2 || d == 4)) {
        const long long threads = (long long)a.Ho * a.Wo;
        const unsigned grid = (unsigned)((threads + 255) / 256);
        const int key = (image_is_f32 ? 4 : 0) | (channels == 4 ? 2 : 0) | (depth_is_f32 ? 1 : 0);
        switch (key) {
            case 0: launch_ingest<false, 3, false>(a, d, grid, st); break;
            case 1: launch_ingest<false, 3, true>(a, d, grid, st); break;
            case 2: launch_ingest<false, 4, false>(a, d, grid, st); break;
            case 3: launch_ingest<false, 4, true>(a, d, grid, st); break;
            case 4: launch_ingest<true, 3, false>(a, d, grid, st); break;
            case 5: launch_ingest<true, 3, true>(a, d, grid, st); break;
            case 6: launch_ingest<true, 4, false>(a, d, grid, st); break;
            default: launch_ingest<true, 4, true>(a, d, grid, st); break;
        }
    } else {
        const long long threads = (long long)a.Ho * a.Wo;
        hipLaunchKernelGGL(ingest_generic_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a, (int)d,
                           (int)channels, (int)(image_is_f32 != 0), (int)(depth_is_f32 != 0));
    }
    return check_launch("qed_ingest_ground_truth");
}
