// Activation element access shared by the HBM-bound kernels: they compute in fp32 on groups of four channels whatever the
// storage type of the activations (fp32, or bf16 / fp16 in the 16-bit activation modes: BASELINE configs[2] / the reference's .half() run).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace e2v {

typedef float aio_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 aio_bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 aio_f16x4 __attribute__((ext_vector_type(4)));

template <typename T> __device__ __forceinline__ aio_f32x4 ld4(const T* p);
template <> __device__ __forceinline__ aio_f32x4 ld4<float>(const float* p) { return *reinterpret_cast<const aio_f32x4*>(p); }
template <> __device__ __forceinline__ aio_f32x4 ld4<__bf16>(const __bf16* p) {
    return __builtin_convertvector(*reinterpret_cast<const aio_bf16x4*>(p), aio_f32x4);
}
template <> __device__ __forceinline__ aio_f32x4 ld4<_Float16>(const _Float16* p) {
    return __builtin_convertvector(*reinterpret_cast<const aio_f16x4*>(p), aio_f32x4);
}
template <typename T> __device__ __forceinline__ void st4(T* p, aio_f32x4 v);
template <> __device__ __forceinline__ void st4<float>(float* p, aio_f32x4 v) { *reinterpret_cast<aio_f32x4*>(p) = v; }
template <> __device__ __forceinline__ void st4<__bf16>(__bf16* p, aio_f32x4 v) {
    *reinterpret_cast<aio_bf16x4*>(p) = __builtin_convertvector(v, aio_bf16x4);
}
template <> __device__ __forceinline__ void st4<_Float16>(_Float16* p, aio_f32x4 v) {
    *reinterpret_cast<aio_f16x4*>(p) = __builtin_convertvector(v, aio_f16x4);
}
template <typename T> __device__ __forceinline__ float ld1(const T* p) { return (float)*p; }
template <typename T> __device__ __forceinline__ void st1(T* p, float v) { *p = (T)v; }

// A lane's piece of a row: VE consecutive channels of storage type T, held as VE / 4 fp32 quads.  Three instances: (float, 4), (H, 4)
// and (H, 8) with H = bf16 / fp16 -- the last is one 16-byte access of a 16-bit row.  The norm kernels are written once over this
// type, and the ORDER of every in-lane sum is fixed here (results are bit-identical at every batch only while it does not move):
//   sum()        (v0 + v1) + (v2 + v3) per quad, the low quad's plus the high quad's;
//   add_sqdev()  4 channels: acc += d d per channel in order; 8 channels: acc += d_lo d_lo + d_hi d_hi over the four channel pairs.
template <typename T, int VE>
struct RowVec {
    static_assert(VE == 4 || (VE == 8 && sizeof(T) == 2), "4 channels of any type, or 8 of a 16-bit one");
    static constexpr int NQ = VE / 4;
    typedef T packed __attribute__((ext_vector_type(VE)));
    aio_f32x4 q[NQ];

    static __device__ __forceinline__ RowVec zero() {
        RowVec r;
#pragma unroll
        for (int h = 0; h < NQ; ++h) r.q[h] = aio_f32x4{0.f, 0.f, 0.f, 0.f};
        return r;
    }
    static __device__ __forceinline__ RowVec load(const T* p) {
        RowVec r;
        if constexpr (VE == 4) {
            r.q[0] = ld4(p);
        } else {
            const packed v = *reinterpret_cast<const packed*>(p);
#pragma unroll
            for (int e = 0; e < 4; ++e) { r.q[0][e] = (float)v[e]; r.q[1][e] = (float)v[4 + e]; }
        }
        return r;
    }
    static __device__ __forceinline__ RowVec load_f32(const float* p) {      // VE fp32 parameters (gamma, beta) in the same register form
        RowVec r;
#pragma unroll
        for (int h = 0; h < NQ; ++h) r.q[h] = *reinterpret_cast<const aio_f32x4*>(p + 4 * h);
        return r;
    }
    __device__ __forceinline__ void store(T* p) const {
        if constexpr (VE == 4) {
            st4(p, q[0]);
        } else {
            packed v;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = (T)q[0][e]; v[4 + e] = (T)q[1][e]; }
            *reinterpret_cast<packed*>(p) = v;
        }
    }
    __device__ __forceinline__ float sum() const {
        if constexpr (VE == 4) return (q[0][0] + q[0][1]) + (q[0][2] + q[0][3]);
        else return ((q[0][0] + q[0][1]) + (q[0][2] + q[0][3])) + ((q[1][0] + q[1][1]) + (q[1][2] + q[1][3]));
    }
    __device__ __forceinline__ void add_sqdev(float& acc, const float mean) const {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if constexpr (VE == 4) {
                const float d = q[0][e] - mean;
                acc += d * d;
            } else {
                const float d0 = q[0][e] - mean, d1 = q[1][e] - mean;
                acc += d0 * d0 + d1 * d1;
            }
        }
    }
    // LayerNorm: (v - mean) rstd gamma + beta
    __device__ __forceinline__ RowVec ln_affine(const float mean, const float rstd, const RowVec& g, const RowVec& b) const {
        RowVec y;
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int h = 0; h < NQ; ++h) y.q[h][e] = (q[h][e] - mean) * rstd * g.q[h][e] + b.q[h][e];
        return y;
    }
    // GroupNorm: v scale + shift with the (scale, shift) pairs of the VE channels interleaved, as the fold writes them
    struct ScSh { aio_f32x4 p[2 * NQ]; };
    static __device__ __forceinline__ ScSh load_scsh(const float* sc) {
        ScSh t;
#pragma unroll
        for (int i = 0; i < 2 * NQ; ++i) t.p[i] = *reinterpret_cast<const aio_f32x4*>(sc + 4 * i);
        return t;
    }
    __device__ __forceinline__ RowVec gn_affine(const ScSh& t) const {
        RowVec y;
#pragma unroll
        for (int h = 0; h < NQ; ++h) {
            y.q[h][0] = q[h][0] * t.p[2 * h][0] + t.p[2 * h][1];
            y.q[h][1] = q[h][1] * t.p[2 * h][2] + t.p[2 * h][3];
            y.q[h][2] = q[h][2] * t.p[2 * h + 1][0] + t.p[2 * h + 1][1];
            y.q[h][3] = q[h][3] * t.p[2 * h + 1][2] + t.p[2 * h + 1][3];
        }
        return y;
    }
    template <class F>
    __device__ __forceinline__ void apply(F f) {                             // an activation, element by element
#pragma unroll
        for (int h = 0; h < NQ; ++h)
#pragma unroll
            for (int e = 0; e < 4; ++e) q[h][e] = f(q[h][e]);
    }
};

// Sum over aligned groups of N = 4 / 8 / 16 / 32 lanes, every lane of a group gets it: DPP adds inside a row of 16 lanes (no LDS, no
// ds_bpermute below 32 lanes), one shuffle across the rows of a group of 32.
template <int N>
__device__ __forceinline__ float lanes_allreduce(float x) {
    static_assert(N == 4 || N == 8 || N == 16 || N == 32, "lanes per group");
    auto dpp = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    x += dpp(x, std::integral_constant<int, 0xB1>{});                          // quad_perm [1,0,3,2]
    x += dpp(x, std::integral_constant<int, 0x4E>{});                          // quad_perm [2,3,0,1]
    if constexpr (N >= 8) x += dpp(x, std::integral_constant<int, 0x141>{});   // row_half_mirror: the other quad of the 8
    if constexpr (N >= 16) x += dpp(x, std::integral_constant<int, 0x140>{});  // row_mirror: the other 8 of the 16
    if constexpr (N >= 32) x += __shfl_xor(x, 16);
    return x;
}

// What the two attention kernels with the keys resident in LDS share (vit.hip: no mask; text.hip: the causal mask): K and V rows of
// 64 floats at a stride of 68 -- a 64-float row spans all 64 banks, so lanes reading the same column of different rows with
// ds_read_b128 would all hit one slot; at 68 the 16 lanes of a group start 4 banks apart --, 8 waves per workgroup, and the wave ops.
constexpr int kKeyLd = 68;          // LDS row stride in floats
constexpr int kKeyWaves = 8;

__device__ __forceinline__ float wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) {      // v of `lane` (wave-uniform) as a scalar
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

}  // namespace e2v
