// A distorted dataset frame resampled to a pinhole, once, while the image cache is filled: what nerfstudio's
// _undistort_image (cv2.undistort / cv2.fisheye + cv2.remap on the CPU) does to every cached frame, in one launch per
// frame over all of its planes.  The definitions are those of qed_splatter_amd/undistort.py (restated from memory of
// nerfstudio 1.1.x and OpenCV, not bit-compatible with either).
//
// Per output pixel (j, i).  The source position is evaluated in float64 from the float32 K, K' and coefficients the
// kernel is given, the blend in float32.  (A float32 position is good to 1-3 ulp, 4e-4 px at 1920 px, which nobody would
// see in the interior.  But taps outside the source read 0, so along the border the sampled image is a step of up to 255
// levels per pixel, and there that error decides roundings the definition fixes.  The few dozen float64 operations per
// pixel hide behind the gather.)
//   x = (j + 0.5 - cx') / fx',  y = (i + 0.5 - cy') / fy'            the ray under the NEW pinhole K'
//   (xd, yd) = distort(x, y)                                        OPENCV: radial k1 k2 k3 + tangential p1 p2;
//                                                                   OPENCV_FISHEYE: theta_d / r with k1..k4
//   u = fx xd + cx,  v = fy yd + cy                                 the source position under the file's K
//   colour (uint8, 3 or 4 channels, alpha like any channel): bilinear at (u - 0.5, v - 0.5), taps outside the source
//     read 0, result floor(value + 0.5)
//   depth (uint16 or float32) and mask (bytes): the nearest tap (floor(u), floor(v)), 0 outside the source
//
// Launch shape.  A gather on the read side and a stream on the write side; 10 MB in and 10 MB out at 1920 x 1080 with RGB
// and 16-bit depth.  As in ingest.hip, every store INSTRUCTION covers one contiguous range across the wave with at most
// 16 B per lane: a thread takes FOUR consecutive pixels of the flat output (a group may run over the end of a row), so
// that it writes 12 B of RGB (one dwordx3) or 16 B of RGBA, 8 B / 16 B of depth and one dword of mask, each at a lane
// stride equal to its width.  4 px x 3 B = 12 B also makes every group's colour dword-aligned although rows of 3 W bytes
// start at any byte offset.  The last, partial group of a frame and buffers that are not 16-byte aligned store element
// by element.
// The reads: the two taps of one source row are 2 C contiguous bytes at any byte offset, fetched as ONE 8-byte load
// (RGBA: exactly the two pixels; RGB: six bytes and two spare, the window moved back where it would pass the end of the
// buffer).  A tap outside the source keeps its address clamped inside and has its weight set to 0, so no load is
// predicated and the kernel has no divergent branch.  Neighbouring lanes read source pixels about four apart: the
// gather lives in L1 / L2 and HBM sees each source byte about once.  A thread works in three phases -- the positions of
// its four pixels, then all of its 8 to 16 loads, then the blends -- so that its loads are in flight together; with
// each pixel's loads waited for before the next pixel's position the kernel took a third longer.
// No LDS, no atomics, plain vector stores.  Measured (profiles/undistort.txt): 13 us per 1920 x 1080 frame with RGB and
// 16-bit depth, 18 us with the fisheye's atan; bound by instruction issue (180 vector instructions per pixel), not by
// the 21 MB it moves.
#include "qed_common.h"

namespace qed {

struct UndistortArgs {
    int H, W;
    const unsigned char* image;
    const void* depth;               // NULL: no depth plane
    const unsigned char* mask;       // NULL: no mask
    unsigned char* out_image;
    void* out_depth;
    unsigned char* out_mask;
    float* out_coords;               // NULL, or [H,W,2] = (u, v)
    double fx, fy, cx, cy;           // the file's K (float32 values, widened on the host)
    double inv_nfx, inv_nfy, ncx, ncy;   // K': 1 / fx', 1 / fy', cx', cy'
    double k1, k2, k3, k4, p1, p2;
};

constexpr int kUndistortPx = 4;      // output pixels per thread

template <bool FISHEYE>
__device__ __forceinline__ void undistort_source_position(const UndistortArgs& a, int j, int i, double& u, double& v) {
    const double x = ((double)j + 0.5 - a.ncx) * a.inv_nfx;
    const double y = ((double)i + 0.5 - a.ncy) * a.inv_nfy;
    const double r2 = x * x + y * y;
    double xd, yd;
    if constexpr (FISHEYE) {
        const double r = sqrt(r2);
        const double t = atan(r);
        const double t2 = t * t;
        const double td = t * (1.0 + t2 * (a.k1 + t2 * (a.k2 + t2 * (a.k3 + t2 * a.k4))));
        const double s = r > 0.0 ? td / r : 1.0;
        xd = x * s;
        yd = y * s;
    } else {
        const double rad = 1.0 + r2 * (a.k1 + r2 * (a.k2 + r2 * a.k3));
        xd = x * rad + 2.0 * a.p1 * x * y + a.p2 * (r2 + 2.0 * x * x);
        yd = y * rad + a.p1 * (r2 + 2.0 * y * y) + 2.0 * a.p2 * x * y;
    }
    u = a.fx * xd + a.cx;
    v = a.fy * yd + a.cy;
}

// floor(t) as an int clamped to [-2, n] (-2 for a NaN), and t - floor(t)
__device__ __forceinline__ int floor_clamped(double t, int n, float* frac) {
    const double f = floor(t);
    if (frac != nullptr) *frac = (float)(t - f);
    return (int)fmin(fmax(f, -2.0), (double)n);                          // (fmax(NaN, -2) = -2)
}

// byte k (0 .. 7) of the pair (lo, hi), as a float
template <int K>
__device__ __forceinline__ float pair_byte(uint32_t lo, uint32_t hi) {
    return (float)(((K < 4 ? lo : hi) >> (8 * (K & 3))) & 255u);
}

// One pixel's bilinear blend at (u - 0.5, v - 0.5), in two steps so that a thread can issue the loads of all its
// pixels before it waits for any.  No branch: the pair of columns (xa, xa + 1) and the rows that are loaded always lie
// inside the source, and a tap of the blend that does not gets the weight 0 (a position far outside, or a NaN from
// wild coefficients: all four).
struct UndistortTaps {
    uint32_t off0, off1;             // byte offsets of the pair in the upper and the lower row
    float w00, w01, w10, w11;        // weights of (upper, lower) x (column xa, xa + 1)
};

template <int C>
__device__ __forceinline__ UndistortTaps undistort_taps(const UndistortArgs& a, double u, double v) {
    float tx, ty;
    const int x0 = floor_clamped(u - 0.5, a.W, &tx), y0 = floor_clamped(v - 0.5, a.H, &ty);
    const float wl = x0 >= 0 && x0 <= a.W - 1 ? 1.f - tx : 0.f, wr = x0 >= -1 && x0 <= a.W - 2 ? tx : 0.f;
    const float wy0 = y0 >= 0 && y0 <= a.H - 1 ? 1.f - ty : 0.f, wy1 = y0 >= -1 && y0 <= a.H - 2 ? ty : 0.f;
    const int xa = min(max(x0, 0), a.W - 2);
    // column xa is the blend's left tap (x0 = xa) or its right one (x0 = -1); column xa + 1 its right tap, or its left
    // one (x0 = W - 1)
    const float wx0 = x0 == xa ? wl : (x0 + 1 == xa ? wr : 0.f), wx1 = x0 == xa ? wr : (x0 == xa + 1 ? wl : 0.f);
    const int ya = min(max(y0, 0), a.H - 1), yb = min(max(y0 + 1, 0), a.H - 1);
    UndistortTaps t;
    t.off0 = (uint32_t)(ya * a.W + xa) * C;                              // (H W < 2^29)
    t.off1 = (uint32_t)(yb * a.W + xa) * C;
    t.w00 = wy0 * wx0; t.w01 = wy0 * wx1; t.w10 = wy1 * wx0; t.w11 = wy1 * wx1;
    return t;
}

// the two pixels at byte `off` of the image of `total` >= 8 bytes: 2 C bytes, as ONE 8-byte load at any byte address
// (global memory takes unaligned accesses, and memcpy tells the compiler it is one).  RGB leaves two bytes spare: the
// window moves back where it would pass the end of the buffer, and undistort_blend shifts the load right by as much.
template <int C>
__device__ __forceinline__ uint32_t pair_start(uint32_t total, uint32_t off) {
    return C == 4 ? off : min(off, total - 8u);
}

template <int C>
__device__ __forceinline__ uint64_t load_pair(const unsigned char* __restrict__ base, uint32_t total, uint32_t off) {
    uint64_t w;
    __builtin_memcpy(&w, base + pair_start<C>(total, off), 8);
    return w;
}

// C channels packed into the low bytes of the result
template <int C>
__device__ __forceinline__ uint32_t undistort_blend(const UndistortTaps& t, uint32_t total, uint64_t r0, uint64_t r1) {
    r0 >>= 8u * (t.off0 - pair_start<C>(total, t.off0));
    r1 >>= 8u * (t.off1 - pair_start<C>(total, t.off1));
    const uint32_t lo0 = (uint32_t)r0, hi0 = (uint32_t)(r0 >> 32), lo1 = (uint32_t)r1, hi1 = (uint32_t)(r1 >> 32);
    uint32_t out = 0;
#define QED_UNDISTORT_CHANNEL(c)                                                                                      \
    {                                                                                                                 \
        const float val = (t.w00 * pair_byte<c>(lo0, hi0) + t.w01 * pair_byte<c + C>(lo0, hi0))                       \
                          + (t.w10 * pair_byte<c>(lo1, hi1) + t.w11 * pair_byte<c + C>(lo1, hi1));                   \
        out |= (uint32_t)(val + 0.5f) << (8 * c);    /* (a convex blend of bytes: 0 .. 255, truncation is floor) */    \
    }
    QED_UNDISTORT_CHANNEL(0) QED_UNDISTORT_CHANNEL(1) QED_UNDISTORT_CHANNEL(2)
    if constexpr (C == 4) QED_UNDISTORT_CHANNEL(3)
#undef QED_UNDISTORT_CHANNEL
    return out;
}

template <int C, bool FISHEYE, bool DEPTH_F32>
__global__ void __launch_bounds__(256) undistort_kernel(UndistortArgs a, int vector_stores) {
    const unsigned n_px = (unsigned)a.H * (unsigned)a.W;                 // (H W < 2^29: 32-bit index arithmetic)
    const unsigned p0 = kUndistortPx * (blockIdx.x * 256u + threadIdx.x);
    if (p0 >= n_px) return;
    const int n = (int)(n_px - p0 < (unsigned)kUndistortPx ? n_px - p0 : (unsigned)kUndistortPx);
    const uint32_t total = n_px * C;
    int i = (int)(p0 / (unsigned)a.W), j = (int)(p0 % (unsigned)a.W);
    float u[kUndistortPx], v[kUndistortPx];                               // (kept for out_coords only)
    UndistortTaps taps[kUndistortPx];
    uint32_t near[kUndistortPx];                                          // index of the nearest tap; ~0: outside
    // ---- where every pixel samples.  (The pixels of the frame's last, partial group beyond its end are computed like
    // any other -- the row index runs to H at most, everything read is clamped -- and not stored.)
#pragma unroll
    for (int k = 0; k < kUndistortPx; ++k) {
        double ud, vd;
        undistort_source_position<FISHEYE>(a, j, i, ud, vd);
        u[k] = (float)ud; v[k] = (float)vd;
        taps[k] = undistort_taps<C>(a, ud, vd);
        const int x = floor_clamped(ud, a.W, nullptr), y = floor_clamped(vd, a.H, nullptr);
        near[k] = x >= 0 && x <= a.W - 1 && y >= 0 && y <= a.H - 1 ? (uint32_t)(y * a.W + x) : ~0u;
        if (++j == a.W) { j = 0; ++i; }
    }
    // ---- all loads of the thread (nothing between them waits), then the arithmetic on them
    uint64_t r0[kUndistortPx], r1[kUndistortPx];
    uint32_t col[kUndistortPx], dep[kUndistortPx] = {}, m[kUndistortPx] = {}, msk = 0;
#pragma unroll
    for (int k = 0; k < kUndistortPx; ++k) {
        r0[k] = load_pair<C>(a.image, total, taps[k].off0);
        r1[k] = load_pair<C>(a.image, total, taps[k].off1);
    }
    if (a.depth != nullptr) {
#pragma unroll
        for (int k = 0; k < kUndistortPx; ++k) {
            const uint32_t s = near[k] != ~0u ? near[k] : 0u;
            dep[k] = DEPTH_F32 ? static_cast<const uint32_t*>(a.depth)[s]
                               : (uint32_t)static_cast<const unsigned short*>(a.depth)[s];
        }
    }
    if (a.mask != nullptr) {
#pragma unroll
        for (int k = 0; k < kUndistortPx; ++k) m[k] = a.mask[near[k] != ~0u ? near[k] : 0u];
    }
#pragma unroll
    for (int k = 0; k < kUndistortPx; ++k) col[k] = undistort_blend<C>(taps[k], total, r0[k], r1[k]);
#pragma unroll
    for (int k = 0; k < kUndistortPx; ++k) {
        dep[k] = near[k] != ~0u ? dep[k] : 0u;
        msk |= (near[k] != ~0u && m[k] != 0u ? 1u : 0u) << (8 * k);
    }

    if (n == kUndistortPx && vector_stores) {
        if constexpr (C == 4) {
            *reinterpret_cast<uint4*>(a.out_image + (size_t)p0 * 4) = make_uint4(col[0], col[1], col[2], col[3]);
        } else {                                                         // 4 x 3 bytes = 3 dwords
            uint32_t* o = reinterpret_cast<uint32_t*>(a.out_image + (size_t)p0 * 3);
            o[0] = col[0] | (col[1] << 24);
            o[1] = (col[1] >> 8) | (col[2] << 16);
            o[2] = (col[2] >> 16) | (col[3] << 8);
        }
        if (a.out_depth != nullptr) {
            if constexpr (DEPTH_F32)
                *reinterpret_cast<uint4*>(static_cast<uint32_t*>(a.out_depth) + p0) = make_uint4(dep[0], dep[1], dep[2], dep[3]);
            else
                *reinterpret_cast<uint2*>(static_cast<unsigned short*>(a.out_depth) + p0) =
                    make_uint2(dep[0] | (dep[1] << 16), dep[2] | (dep[3] << 16));
        }
        if (a.out_mask != nullptr) *reinterpret_cast<uint32_t*>(a.out_mask + p0) = msk;
        if (a.out_coords != nullptr) {
            float4* o = reinterpret_cast<float4*>(a.out_coords + (size_t)p0 * 2);
            o[0] = make_float4(u[0], v[0], u[1], v[1]);
            o[1] = make_float4(u[2], v[2], u[3], v[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kUndistortPx; ++k) {
            if (k >= n) break;
            const size_t p = (size_t)p0 + k;
#pragma unroll
            for (int c = 0; c < C; ++c) a.out_image[p * C + c] = (unsigned char)(col[k] >> (8 * c));
            if (a.out_depth != nullptr) {
                if constexpr (DEPTH_F32) static_cast<uint32_t*>(a.out_depth)[p] = dep[k];
                else static_cast<unsigned short*>(a.out_depth)[p] = (unsigned short)dep[k];
            }
            if (a.out_mask != nullptr) a.out_mask[p] = (unsigned char)((msk >> (8 * k)) & 1u);
            if (a.out_coords != nullptr) { a.out_coords[2 * p] = u[k]; a.out_coords[2 * p + 1] = v[k]; }
        }
    }
}

template <int C, bool FISHEYE>
static void launch_undistort(const UndistortArgs& a, bool depth_f32, int vector_stores, unsigned grid, hipStream_t st) {
    if (depth_f32) hipLaunchKernelGGL((undistort_kernel<C, FISHEYE, true>), dim3(grid), dim3(256), 0, st, a, vector_stores);
    else hipLaunchKernelGGL((undistort_kernel<C, FISHEYE, false>), dim3(grid), dim3(256), 0, st, a, vector_stores);
}

}  // namespace qed

using namespace qed;

extern "C" int qed_undistort_frame(int32_t height, int32_t width, const uint8_t* image, int32_t channels, const void* depth,
                                   int32_t depth_is_f32, const uint8_t* mask, const float* src_K, const float* new_K,
                                   const float* dist, int32_t model, uint8_t* out_image, void* out_depth,
                                   uint8_t* out_mask, float* out_coords, void* stream) {
    QED_REQUIRE(channels == 3 || channels == 4, "channels must be 3 or 4");
    QED_REQUIRE(height >= 2 && width >= 2, "a frame of at least 2 x 2 pixels");
    QED_REQUIRE((long long)height * width <= 0x1fffffffLL, "frame too large");
    QED_REQUIRE(model == 0 || model == 1, "model must be 0 (OPENCV) or 1 (OPENCV_FISHEYE)");
    QED_REQUIRE(image && out_image, "null image buffers");
    QED_REQUIRE((depth == nullptr) == (out_depth == nullptr) && (mask == nullptr) == (out_mask == nullptr),
                "depth / mask and their outputs come together");
    QED_REQUIRE(src_K && new_K && dist, "null host arrays (src_K, new_K, dist)");
    QED_REQUIRE(src_K[0] > 0.f && src_K[1] > 0.f && new_K[0] > 0.f && new_K[1] > 0.f, "focal lengths must be positive");
    QED_REQUIRE(model == 1 || dist[3] == 0.f, "k4 belongs to the fisheye model");
    QED_REQUIRE(model == 0 || (dist[4] == 0.f && dist[5] == 0.f), "the fisheye model has no p1 / p2");
    UndistortArgs a;
    a.H = height; a.W = width;
    a.image = image; a.depth = depth; a.mask = mask;
    a.out_image = out_image; a.out_depth = out_depth; a.out_mask = out_mask; a.out_coords = out_coords;
    a.fx = src_K[0]; a.fy = src_K[1]; a.cx = src_K[2]; a.cy = src_K[3];
    a.inv_nfx = 1.0 / (double)new_K[0]; a.inv_nfy = 1.0 / (double)new_K[1]; a.ncx = new_K[2]; a.ncy = new_K[3];
    a.k1 = dist[0]; a.k2 = dist[1]; a.k3 = dist[2]; a.k4 = dist[3]; a.p1 = dist[4]; a.p2 = dist[5];
    const uintptr_t outputs = (uintptr_t)out_image | (uintptr_t)out_depth | (uintptr_t)out_mask | (uintptr_t)out_coords;
    const int vector_stores = (outputs & 15u) == 0;
    const long long threads = ((long long)height * width + kUndistortPx - 1) / kUndistortPx;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (channels == 3) {
        if (model == 1) launch_undistort<3, true>(a, depth_is_f32 != 0, vector_stores, grid, st);
        else launch_undistort<3, false>(a, depth_is_f32 != 0, vector_stores, grid, st);
    } else {
        if (model == 1) launch_undistort<4, true>(a, depth_is_f32 != 0, vector_stores, grid, st);
        else launch_undistort<4, false>(a, depth_is_f32 != 0, vector_stores, grid, st);
    }
    return check_launch("qed_undistort_frame");
}
