// Wave and workgroup reductions shared by the streaming kernels of libqed_splat.so (device code only).
//
// The pattern: a kernel that reduces something over a grid has every workgroup write its partial results to its own
// slots of a workspace, and a second, one-workgroup launch folds them.  Same-address atomics serialise instead (~12 ns
// each; ten per workgroup made the metrics pass 103 us at 1080p instead of ~15), and their order is not fixed.  Both
// launches end in the same tail -- a cross-lane reduction, one value per wave parked in LDS, the waves' values added
// in a fixed order -- and that tail lives here once.  There are three shapes, each with its own function: a sum of
// doubles, a sum of floats carried on in double, and the 3-axis bounds of a point set.
#pragma once
#include <hip/hip_runtime.h>

namespace qed {

// ---- wave64 cross-lane helpers (DPP / shuffles; no LDS traffic) -------------------------------
// sum over the 16 lanes of each DPP row; result valid in every lane of the row
__device__ __forceinline__ float row16_sum(float v) {
    // quad_perm / row_ror rotate within a row of 16 lanes
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));  // row_ror:1
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));  // row_ror:2
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));  // row_ror:4
    // row_ror:8 as ONE instruction.  Written with the builtin, the compiler sinks this last add into a following
    // `if (lane % 16 == 0)` and leaves v_mov 0 + v_mov_dpp outside it: three instructions instead of one, per value.
    // (s_nop 1: a DPP read needs two wait states after the VALU write of its source; the compiler cannot see
    // that hazard through inline asm.)
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_ror:8 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(v));
    return v;
}

// full wave64 sum, result valid in every lane
__device__ __forceinline__ float wave_sum(float v) {
    v = row16_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// xor butterflies, result valid in every lane (and, for the double, the same bits in every lane: addition commutes)
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- workgroup sums of COLS columns, NT threads -----------------------------------------------------------------
// the W waves' values in the fixed order of a balanced tree: (w0 + w1) + (w2 + w3) for the four waves of 256 threads
template <int W>
__device__ __forceinline__ double combine_waves(const double* w) {
    static_assert(W >= 1 && (W & (W - 1)) == 0, "a power-of-two number of waves");
    if constexpr (W == 1) return w[0];
    else return combine_waves<W / 2>(w) + combine_waves<W / 2>(w + W / 2);
}

// The park-and-combine half: v[c] is wave-uniform (or valid in lane 0).  Lane 0 of each wave parks it in s_w[c][wave];
// thread c < COLS adds the waves' values into s[c].  Every thread of the workgroup must call; afterwards every thread may
// read s[c].
template <int COLS, int NT = 256>
__device__ __forceinline__ void block_combine_d(const double (&v)[COLS], double (*s_w)[NT / 64], double* s) {
    static_assert(NT % 64 == 0 && COLS <= NT, "whole waves, a thread per column");
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < COLS; ++c) s_w[c][threadIdx.x >> 6] = v[c];
    }
    __syncthreads();
    if (threadIdx.x < COLS) s[threadIdx.x] = combine_waves<NT / 64>(s_w[threadIdx.x]);
    __syncthreads();
}

// workgroup sum of each column of per-thread doubles
template <int COLS, int NT = 256>
__device__ __forceinline__ void block_sum_d(const double (&v)[COLS], double (*s_w)[NT / 64], double* s) {
    double r[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) r[c] = wave_sum_d(v[c]);
    block_combine_d<COLS, NT>(r, s_w, s);
}

// workgroup sum of each column of per-thread floats: summed as floats inside a wave, in double from there on
template <int COLS, int NT = 256>
__device__ __forceinline__ void block_sum_f(const float (&acc)[COLS], double (*s_w)[NT / 64], double* s) {
    double r[COLS];
#pragma unroll
    for (int c = 0; c < COLS; ++c) r[c] = (double)wave_sum(acc[c]);
    block_combine_d<COLS, NT>(r, s_w, s);
}

// ---- 3-axis bounds: min / max of the finite points and a count of the others ------------------------------------
struct Bounds3 {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int bad = 0;
};

__device__ __forceinline__ void bounds3_add(Bounds3& b, const float f[3]) {
    if (isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2])) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { b.mn[a] = fminf(b.mn[a], f[a]); b.mx[a] = fmaxf(b.mx[a], f[a]); }
    } else {
        ++b.bad;
    }
}

// Every thread of the workgroup must call; the workgroup's bounds and count are left in thread 0's b.
template <int NT>
__device__ __forceinline__ void bounds3_block(Bounds3& b, float (*s_m)[6], int* s_bad) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            b.mn[a] = fminf(b.mn[a], __shfl_xor(b.mn[a], o, 64));
            b.mx[a] = fmaxf(b.mx[a], __shfl_xor(b.mx[a], o, 64));
        }
        b.bad += __shfl_xor(b.bad, o, 64);
    }
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_m[wid][a] = b.mn[a]; s_m[wid][3 + a] = b.mx[a]; }
        s_bad[wid] = b.bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) {
            b.bad += s_bad[w];
#pragma unroll
            for (int a = 0; a < 3; ++a) { b.mn[a] = fminf(b.mn[a], s_m[w][a]); b.mx[a] = fmaxf(b.mx[a], s_m[w][3 + a]); }
        }
    }
}

}  // namespace qed
