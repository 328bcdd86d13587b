// Pieces shared by the fp32 (igemm.hip) and bf16-activation (bgemm.hip) implicit-GEMM kernels: vector typedefs, the GEGLU gate's
// erf-GELU and the epilogues that take 32x32 MFMA accumulators (WEIGHT fragment as the A operand) to memory.
#pragma once
#include "h16.h"
#include "kernels.h"

namespace e2v {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));


// erf-GELU of the GEGLU gate (diffusers GEGLU.gelu = F.gelu, exact form).  The library erff costs 38 vector instructions with
// three branches, and on gfx950 they are paid at the fp32-MFMA's own rate (the GEGLU tiles spent a fifth of their time in the
// epilogue); Abramowitz-Stegun 7.1.26 -- erf(z) = 1 - (a1 t + .. + a5 t^5) exp(-z^2), t = 1 / (1 + p z), |error| <= 1.5e-7,
// i.e. at the level of fp32 rounding of values in [-1, 1] -- is 14, branch-free.  Measured |gelu error| <= 4.6e-7.
__device__ __forceinline__ float gelu_erf(float x) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    p *= t;
    const float e = __builtin_amdgcn_exp2f(z * z * -1.44269504088896340736f);
    const float erf_abs = fmaf(-p, e, 1.0f);
    return 0.5f * x * (1.0f + copysignf(erf_abs, x));
}

// The same function on a pair: the fma / mul chain as v_pk_fma_f32 / v_pk_mul_f32 (half the vector instructions; on gfx950 they are not
// hidden behind the fp32 MFMA), v_rcp_f32 and v_exp_f32 per element.  Each element sees exactly the operations of gelu_erf.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 gelu_erf2(const f32x2 x) {
    const f32x2 z = __builtin_elementwise_abs(x) * 0.70710678118654752440f;
    const f32x2 d = __builtin_elementwise_fma(f32x2(0.3275911f), z, f32x2(1.0f));
    const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
    f32x2 p = __builtin_elementwise_fma(f32x2(1.061405429f), t, f32x2(-1.453152027f));
    p = __builtin_elementwise_fma(p, t, f32x2(1.421413741f));
    p = __builtin_elementwise_fma(p, t, f32x2(-0.284496736f));
    p = __builtin_elementwise_fma(p, t, f32x2(0.254829592f));
    p *= t;
    const f32x2 a = z * z * -1.44269504088896340736f;
    const f32x2 e = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
    const f32x2 erf_abs = __builtin_elementwise_fma(-p, e, f32x2(1.0f));
    return 0.5f * x * (1.0f + __builtin_elementwise_copysign(erf_abs, x));
}

// The same gate in the bf16-activation mode, where the product value * gelu(gate) is rounded to bf16 (2^-9 relative) on its way out:
// gelu(x) = x Phi(x) with the normal CDF as a logistic of an odd cubic, Phi(x) ~ 1 / (1 + exp(-(a x + b x^3))), a = 1.60031415,
// b = 0.06940179 (minimax fit of x Phi(x) over the real line; monotone, so no clamp): |gelu error| <= 2.8e-4 = 1/14 of the rounding
// of a bf16 value near 1 (bound restated in tests/test_oracle_anchors.py).  Five plain vector instructions + v_exp_f32 + v_rcp_f32 instead
// of thirteen + two: the GEGLU 320 -> 2560 tiles of a B = 32 pass spent as long in this epilogue (64 gates per lane) as in their five
// K steps.  fp32 mode keeps gelu_erf above.
__device__ __forceinline__ float gelu_bf16_grade(float x) {
    const float u = x * x;
    const float t = x * fmaf(-0.06940179f * 1.44269504088896340736f, u, -1.60031415f * 1.44269504088896340736f);
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(t));
}
// (fast: wave-uniform, IgemmArgs::a_bf16 -- the arithmetic mode, never the kernel or the batch, picks the form: the logistic form in
// bf16 mode only; fp16 rounds 8x finer than bf16, so the fp16 mode keeps the erf form like fp32)
__device__ __forceinline__ float gelu_gate(float x, const bool fast) { return fast ? gelu_bf16_grade(x) : gelu_erf(x); }
// (E2V_F16_FAST_GATE: a measurement build -- `make EXTRA=-DE2V_F16_FAST_GATE` -- that gives the fp16 mode the logistic gate too, to
// price the erf form: profiles/r05_fp16_gate_ab.log)
#ifdef E2V_F16_FAST_GATE
constexpr bool kF16FastGate = true;
#else
constexpr bool kF16FastGate = false;
#endif
template <typename H> __device__ __forceinline__ float gelu_gate16(float x) {       // the same choice at compile time, by the kernel's 16-bit type
    if constexpr (__is_same(H, __bf16) || kF16FastGate) return gelu_bf16_grade(x);
    else return gelu_erf(x);
}

typedef hx4<__bf16> bf16x4;        // (the split-bf16 fp32 path of igemm.hip names its operands)
typedef hx8<__bf16> bf16x8;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Buffer descriptor over [ptr, ptr + 2 GB) from a pointer forced into SGPRs: an offset of kEpiOob lies outside the window, so a masked
// lane's load returns zeros and its store is dropped by the buffer unit -- no branch, and every access of a batch is one basic block.
constexpr unsigned kEpiOob = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t epi_rsrc(const void* ptr) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(ptr);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), (short)0, 0x7FFFFFF0, 0x00020000);
}
__device__ __forceinline__ f32x4 epi_load(const __amdgpu_buffer_rsrc_t rs, const unsigned off) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}
__device__ __forceinline__ void epi_store(const f32x4 v, const __amdgpu_buffer_rsrc_t rs, const unsigned off) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, off, 0, 0);
}

// Element-wise form of the epilogues below (N, or a stride, not a multiple of 4: the VAE's 3-channel conv_out)
template <int BM, int TM, int TN, int WM, int WN>
__device__ __forceinline__ void igemm_epilogue_scalar(const IgemmArgs& p, f32x16 (&acc)[TM][TN], float* __restrict__ out, const int bm,
                                                      const int n0, const int wm, const int wn, const int lane) {
    const int mrow = lane & 31;
    const int nq = (lane >> 5) * 4;
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = bm * BM + wm * WM + mi * 32 + mrow;
        if (m >= p.M) continue;
        const float* rbp = p.rowbias ? p.rowbias + (size_t)(m / p.rows_per_sample) * p.rb_ld : nullptr;
        const float* rsp = p.resid ? p.resid + (size_t)m * p.ldr : nullptr;
        float* orow = out + (size_t)m * p.ldc;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * WN + ni * 32 + 8 * g + nq;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (n + e >= p.N) break;
                    float v = acc[mi][ni][4 * g + e] * p.alpha + (p.bias ? p.bias[n + e] : 0.f);
                    if (rbp) v += rbp[n + e];
                    if (rsp) v += rsp[n + e];
                    if (p.relu) v = fmaxf(v, 0.f);
                    orow[n + e] = v;
                }
            }
    }
}

// Epilogue of the 16-bit tiles with fp32 output (bgemm.hip), and the layout it shares with the fp32 tiles' igemm_epilogue_batched
// below (all use 32x32 MFMA results with the WEIGHT fragment as the A operand): in each 32x32 result a lane holds pixel m = lane & 31
// and output channels n = 8 g + 4 (lane >> 5) + e in register r = 4 g + e -- four consecutive channels per register quad, i.e. 16-byte
// bias / time-embedding / residual loads and 16-byte stores.
template <int BM, int TM, int TN, int WM, int WN>
__device__ __forceinline__ void igemm_epilogue(const IgemmArgs& p, f32x16 (&acc)[TM][TN], float* __restrict__ out, const int bm,
                                               const int n0, const int wm, const int wn, const int lane, float* stage) {
    const int mrow = lane & 31;
    const int nq = (lane >> 5) * 4;
    if (p.geglu) {
        if constexpr (TN == 2) {
            const int nb = n0 + wn * WN;                           // value columns nb .. nb+31, gate columns nb+32 .. nb+63
            if (nb + 64 <= p.N) {
                // v * gelu(g) in the accumulator layout, staged per wave as WM x 32 and written row-contiguously (8 lanes = one
                // 128-byte row segment) like the plain epilogue below
                constexpr int SLD = 36;
                float* st = stage + (size_t)(threadIdx.x >> 6) * 32 * SLD;
                const int col = (lane & 7) * 4;
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 bv = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + nb + 8 * g + nq) : f32x4{0.f, 0.f, 0.f, 0.f};
                        const f32x4 bg = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + nb + 32 + 8 * g + nq) : f32x4{0.f, 0.f, 0.f, 0.f};
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            y[e] = (acc[mi][0][4 * g + e] * p.alpha + bv[e]) * gelu_gate(acc[mi][1][4 * g + e] * p.alpha + bg[e], p.a_bf16 == H16_BF16 || (kF16FastGate && p.a_bf16 == H16_FP16));
                        *reinterpret_cast<f32x4*>(st + mrow * SLD + 8 * g + nq) = y;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = (lane >> 3) + 8 * i;
                        const int m = bm * BM + wm * WM + mi * 32 + row;
                        if (m < p.M)
                            *reinterpret_cast<f32x4*>(out + (size_t)m * p.ldc + nb / 2 + col) = *reinterpret_cast<const f32x4*>(st + row * SLD + col);
                    }
                }
            }
        }
        return;
    }
    const bool vec = ((p.N | p.ldc | p.ldr | p.rb_ld) & 3) == 0;   // strides of absent operands are 0
    if (vec) {
        // Row-contiguous epilogue: the wave transposes its accumulators, 32 rows at a time, through LDS (the tile buffers are dead: every
        // real fragment read precedes the last barrier of the k-loop) so that a 16-byte access instruction covers whole rows --
        // 64 / (WN / 4) rows x WN floats -- instead of 32 rows x 32 bytes.  Residual reads and stores then move full 128-byte
        // lines (+5 % on the K = 320 layers, whose output write is a tenth of their time).
        constexpr int SLD = WN + 4;                            // padded staging row: conflict-free b128 writes and reads
        constexpr int LPR = WN / 4;                            // lanes per staged row
        constexpr int RPI = 64 / LPR;                          // rows per access instruction
        float* st = stage + (size_t)(threadIdx.x >> 6) * 32 * SLD;   // one 32-row staging block per wave, reused per mi
        const int col = (lane % LPR) * 4;
        const int n = n0 + wn * WN + col;
        f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && n < p.N) bias4 = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = acc[mi][ni][4 * g + e];
                    *reinterpret_cast<f32x4*>(st + mrow * SLD + ni * 32 + 8 * g + nq) = y;
                }
#pragma unroll
            for (int i = 0; i < 32 / RPI; ++i) {
                const int row = lane / LPR + RPI * i;
                const int m = bm * BM + wm * WM + mi * 32 + row;
                if (m >= p.M || n >= p.N) continue;            // N % 4 == 0: the lane's four columns are in or out together
                f32x4 y = *reinterpret_cast<const f32x4*>(st + row * SLD + col);
                if (p.alpha != 1.0f) y *= p.alpha;             // only the VAE attention scales
                y += bias4;
                if (p.rowbias) y += *reinterpret_cast<const f32x4*>(p.rowbias + (size_t)(m / p.rows_per_sample) * p.rb_ld + n);
                if (p.resid) y += *reinterpret_cast<const f32x4*>(p.resid + (size_t)m * p.ldr + n);
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = fmaxf(y[e], 0.f);
                }
                *reinterpret_cast<f32x4*>(out + (size_t)m * p.ldc + n) = y;
            }
        }
        return;
    }
    igemm_epilogue_scalar<BM, TM, TN, WM, WN>(p, acc, out, bm, n0, wm, wn, lane);
}

// The same epilogue for the fp32 and split-bf16 tiles (igemm.hip), whose short-K launches paid a fifth of a tile for it: memory accesses
// in batches of branch-free buffer loads / stores, the GEGLU gate on packed fp32 pairs.  Per element the floating-point operations
// and their order are those of igemm_epilogue -- results are bit-identical.  (The 16-bit tiles keep the form above: with this one
// inlined their kernels fell from three / two waves per SIMD to one.)
// NREQ: residual requests per 32-row block -- how many rows' quads are in flight at once (2: 16 rows; 4: 8 rows, for the 128-register
// 16-k tile).  It moves loads only: the per-element arithmetic and its order do not depend on it.
template <int BM, int TM, int TN, int WM, int WN, int NREQ = 2>
__device__ __forceinline__ void igemm_epilogue_batched(const IgemmArgs& p, f32x16 (&acc)[TM][TN], float* __restrict__ out, const int bm,
                                                       const int n0, const int wm, const int wn, const int lane, float* stage) {
    const int mrow = lane & 31;
    const int nq = (lane >> 5) * 4;
    const int m_left = p.M - bm * BM;                              // rows of the matrix from the tile's first row on
    const __amdgpu_buffer_rsrc_t ro = epi_rsrc(out + (size_t)bm * BM * p.ldc);   // stores: offsets relative to the tile's first row
    if (p.geglu) {
        if constexpr (TN == 2) {
            const int nb = n0 + wn * WN;                           // value columns nb .. nb+31, gate columns nb+32 .. nb+63
            if (nb + 64 <= p.N) {
                // v * gelu(g) in the accumulator layout, staged per wave as WM x 32 and written row-contiguously (8 lanes = one
                // 128-byte row segment) like the plain epilogue below
                constexpr int SLD = 36;
                float* st = stage + (size_t)(threadIdx.x >> 6) * 32 * SLD;
                const int col = (lane & 7) * 4;
                const bool fast = p.a_bf16 == H16_BF16 || (kF16FastGate && p.a_bf16 == H16_FP16);
                // the wave's eight bias quads, once (they were loaded per 32-row block, inside the element loops)
                const __amdgpu_buffer_rsrc_t rbs = epi_rsrc(p.bias);
                f32x4 bv[4], bg[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bv[g] = epi_load(rbs, p.bias ? (unsigned)(nb + 8 * g + nq) * 4u : kEpiOob);
                    bg[g] = epi_load(rbs, p.bias ? (unsigned)(nb + 32 + 8 * g + nq) * 4u : kEpiOob);
                }
                const f32x2 alpha2 = {p.alpha, p.alpha};
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
                    if (fast) {                                    // the 16-bit arithmetic modes' gate (no fp32 launch selects it)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            f32x4 y;
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                y[e] = (acc[mi][0][4 * g + e] * p.alpha + bv[g][e]) * gelu_gate(acc[mi][1][4 * g + e] * p.alpha + bg[g][e], true);
                            *reinterpret_cast<f32x4*>(st + mrow * SLD + 8 * g + nq) = y;
                        }
                    } else {
                        // erf form on pairs: per element the fma / mul sequence of the scalar code (acc * alpha + bias fused), as
                        // packed instructions -- 16 pairs per 32-row block instead of 32 trips through a 29-instruction loop body
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            f32x4 y;
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                const int r = 4 * g + 2 * h;
                                const f32x2 v = __builtin_elementwise_fma(f32x2{acc[mi][0][r], acc[mi][0][r + 1]}, alpha2, f32x2{bv[g][2 * h], bv[g][2 * h + 1]});
                                const f32x2 x = __builtin_elementwise_fma(f32x2{acc[mi][1][r], acc[mi][1][r + 1]}, alpha2, f32x2{bg[g][2 * h], bg[g][2 * h + 1]});
                                const f32x2 o = v * gelu_erf2(x);
                                y[2 * h] = o[0];
                                y[2 * h + 1] = o[1];
                            }
                            *reinterpret_cast<f32x4*>(st + mrow * SLD + 8 * g + nq) = y;
                        }
                    }
                    f32x4 y[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i] = *reinterpret_cast<const f32x4*>(st + ((lane >> 3) + 8 * i) * SLD + col);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = wm * WM + mi * 32 + (lane >> 3) + 8 * i;
                        epi_store(y[i], ro, row < m_left ? (unsigned)(row * p.ldc + nb / 2 + col) * 4u : kEpiOob);
                    }
                }
            }
        }
        return;
    }
    const bool vec = ((p.N | p.ldc | p.ldr | p.rb_ld) & 3) == 0;   // strides of absent operands are 0
    if (vec) {
        // Row-contiguous epilogue: the wave transposes its accumulators, 32 rows at a time, through LDS (the tile buffers are dead: every
        // real fragment read precedes the last barrier of the k-loop) so that a 16-byte access instruction covers whole rows --
        // 64 / (WN / 4) rows x WN floats -- instead of 32 rows x 32 bytes.  Residual reads and stores then move full 128-byte
        // lines (+5 % on the K = 320 layers, whose output write is a tenth of their time).
        // Memory accesses come in batches: the residual quads of 16 rows and a block's time-embedding quads are requested half a block
        // ahead of their use, as buffer loads whose masked lanes (rows >= M, columns >= N, absent operand) carry an out-of-window
        // offset; adds and stores follow behind counted waits that leave the stores in flight.  (One load, one wait for everything
        // before it, one store per row group -- 16 memory round trips in a row per wave of a 128 x 128 tile -- was a fifth of a
        // K = 320 tile.  Whole 32-row requests do not fit 168 registers: the allocator spilled two quads behind a full wait.)
        constexpr int SLD = WN + 4;                            // padded staging row: conflict-free b128 writes and reads
        constexpr int LPR = WN / 4;                            // lanes per staged row
        constexpr int RPI = 64 / LPR;                          // rows per access instruction
        constexpr int NI = 32 / RPI;                           // access instructions per 32-row block
        float* st = stage + (size_t)(threadIdx.x >> 6) * 32 * SLD;   // one 32-row staging block per wave, reused per mi
        const int col = (lane % LPR) * 4;
        const int rl = lane / LPR;                             // the lane's row within an access instruction
        const int n = n0 + wn * WN + col;
        const bool nok = n < p.N;                              // N % 4 == 0: the lane's four columns are in or out together
        const f32x4 bias4 = epi_load(epi_rsrc(p.bias), ((p.bias != nullptr) & nok) ? (unsigned)n * 4u : kEpiOob);
        const __amdgpu_buffer_rsrc_t rr = epi_rsrc(p.resid ? p.resid + (size_t)bm * BM * p.ldr : nullptr);
        const __amdgpu_buffer_rsrc_t rt = epi_rsrc(p.rowbias);
        const bool rok = (p.resid != nullptr) & nok, tok = (p.rowbias != nullptr) & nok;   // bitwise: selects, not branches
        const int row0 = wm * WM + rl;                         // the lane's first row within the tile
        // Time-embedding rows: a 32-row block touches at most two samples when rows_per_sample >= 32 (every map of the full-size
        // model), so they are two loads per lane and block -- the sample of the block's first row and the next -- requested with the
        // residual, and a select per row group.  Tiny maps (TINY) load one row per row group instead, and their residual with it, NH
        // row groups at a time behind the previous stores: a code path of its own, so that the other one has no load between its
        // stores and no register of its batch is shared with it.
        constexpr int NH = NREQ >= 4 ? 1 : 2;                  // row groups finished together (2: 168 registers; 1 with the short requests: 128, no spill)
        auto run = [&](auto tiny_c) {
            constexpr bool TINY = decltype(tiny_c)::value;
            f32x4 res[TM][NI], tb[TM][2];
            int split[TM];                                     // rows of block mi below split[mi] belong to its first sample
            constexpr int HB = NI / NREQ > NH ? NI / NREQ : NH;   // a request: the residual of HB row groups (NREQ = 2: 16 rows); with a block's first, its time-embedding rows
            constexpr int NR = NI / HB;                        // requests per block
            auto request = [&](const int mi, const int hh) {
                if constexpr (TINY) return;
#pragma unroll
                for (int i = hh * HB; i < hh * HB + HB; ++i) {
                    const int row = row0 + mi * 32 + RPI * i;
                    res[mi][i] = epi_load(rr, (rok & (row < m_left)) ? (unsigned)(row * p.ldr + n) * 4u : kEpiOob);
                }
                if (hh != 0) return;
                const int m0 = __builtin_amdgcn_readfirstlane(bm * BM + wm * WM + mi * 32);   // the block's first row: scalar division
                const int s_lo = m0 / p.rows_per_sample;
                split[mi] = (s_lo + 1) * p.rows_per_sample - m0;
                const int rows = min(p.M - m0, 32);
                tb[mi][0] = epi_load(rt, (tok & (rows > 0)) ? (unsigned)(s_lo * p.rb_ld + n) * 4u : kEpiOob);
                tb[mi][1] = epi_load(rt, (tok & (split[mi] < rows)) ? (unsigned)((s_lo + 1) * p.rb_ld + n) * 4u : kEpiOob);
            };
            request(0, 0);
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e) y[e] = acc[mi][ni][4 * g + e];
                        *reinterpret_cast<f32x4*>(st + mrow * SLD + ni * 32 + 8 * g + nq) = y;
                    }
                // NH row groups at a time: per element, in this order, (* alpha) + bias + time embedding + residual, relu
                // -- under wave-uniform conditions -- then their stores back to back
#pragma unroll
                for (int h = 0; h < NI / NH; ++h) {
                    // (requests stay where they are written, half a block ahead: left alone the scheduler issues them all up front)
                    __builtin_amdgcn_sched_barrier(0);
                    if ((h * NH) % HB == 0) {                  // one request ahead of the one this row group consumes
                        if (h * NH / HB + 1 < NR) request(mi, h * NH / HB + 1);
                        else if (mi + 1 < TM) request(mi + 1, 0);
                    }
                    f32x4 th[NH], rh[NH];
                    if constexpr (TINY) {
                        const int m0 = __builtin_amdgcn_readfirstlane(bm * BM + wm * WM + mi * 32);
                        const int s0 = m0 / p.rows_per_sample, rem = m0 - s0 * p.rows_per_sample;
                        // sample of row m0 + d = s0 + (rem + d) / rows_per_sample with rem + d < 64, the quotient through a
                        // reciprocal: (x + 0.5) / r is at least 1 / 64 away from an integer, the product's error below 2^-16
                        const float inv = __builtin_amdgcn_rcpf((float)p.rows_per_sample);
#pragma unroll
                        for (int j = 0; j < NH; ++j) {
                            const int d = rl + RPI * (h * NH + j);
                            const int smp = s0 + (int)(((float)(rem + d) + 0.5f) * inv);
                            const int row = row0 + mi * 32 + d - rl;
                            th[j] = epi_load(rt, (tok & (row < m_left)) ? (unsigned)(smp * p.rb_ld + n) * 4u : kEpiOob);
                            rh[j] = epi_load(rr, (rok & (row < m_left)) ? (unsigned)(row * p.ldr + n) * 4u : kEpiOob);
                        }
                    }
                    f32x4 y[NH];
#pragma unroll
                    for (int j = 0; j < NH; ++j) y[j] = *reinterpret_cast<const f32x4*>(st + (rl + RPI * (h * NH + j)) * SLD + col);
                    if (p.alpha != 1.0f) {                     // only the VAE attention scales
#pragma unroll
                        for (int j = 0; j < NH; ++j) y[j] *= p.alpha;
                    }
#pragma unroll
                    for (int j = 0; j < NH; ++j) y[j] += bias4;
                    if (p.rowbias) {
#pragma unroll
                        for (int j = 0; j < NH; ++j) {
                            if constexpr (TINY) y[j] += th[j];
                            else y[j] += (rl + RPI * (h * NH + j) >= split[mi]) ? tb[mi][1] : tb[mi][0];
                        }
                    }
                    if (p.resid) {
#pragma unroll
                        for (int j = 0; j < NH; ++j) y[j] += TINY ? rh[j] : res[mi][h * NH + j];
                    }
                    if (p.relu) {
#pragma unroll
                        for (int j = 0; j < NH; ++j)
#pragma unroll
                            for (int e = 0; e < 4; ++e) y[j][e] = fmaxf(y[j][e], 0.f);
                    }
#pragma unroll
                    for (int j = 0; j < NH; ++j) {
                        const int row = row0 + mi * 32 + RPI * (h * NH + j);
                        epi_store(y[j], ro, (nok & (row < m_left)) ? (unsigned)(row * p.ldc + n) * 4u : kEpiOob);
                    }
                }
            }
        };
        if (p.rowbias && p.rows_per_sample < 32) run(std::true_type{});
        else run(std::false_type{});
        return;
    }
    igemm_epilogue_scalar<BM, TM, TN, WM, WN>(p, acc, out, bm, n0, wm, wn, lane);
}



// bf16 OUTPUT (bf16-activation mode): same staging through LDS, but a lane finishes 8 consecutive columns -- two 16-byte
// reads of the fp32 staging row, bias / time-embedding row in fp32, the residual as 8 bf16 (16 bytes), one rounding to bf16 at
// the very end, a 16-byte store.  `out` / `p.resid` are bf16 (p.resid_bf16) or the residual is fp32 (latents never are).
// SWZ (the persistent kernel): the staging area is the stage buffer the tile has just consumed and no byte more -- 32 rows x WN
// floats per wave, UNPADDED, the 16-byte chunk of a row XOR-swizzled with the row (256-byte rows: row & 15; 128-byte rows:
// (row >> 1) & 7) so that the column-major writes and the row-major reads both cover all 64 banks once per 16 lanes.
template <int BM, int TM, int TN, int WM, int WN, bool SWZ = false, typename H = __bf16>      // H: the 16-bit type (deduced from `out`)
__device__ __forceinline__ void bgemm_epilogue_bf16(const IgemmArgs& p, f32x16 (&acc)[TM][TN], H* __restrict__ out, const int bm,
                                                    const int n0, const int wm, const int wn, const int lane, float* stage) {
    const int mrow = lane & 31;
    const int nq = (lane >> 5) * 4;
    if (p.geglu) {
        if constexpr (TN == 2) {
            const int nb = n0 + wn * WN;                           // value columns nb .. nb+31, gate columns nb+32 .. nb+63
            if (nb + 64 <= p.N) {
                constexpr int SLD = 36;
                float* st = stage + (size_t)(threadIdx.x >> 6) * 32 * SLD;
                const int col = (lane & 3) * 8;                    // 4 lanes x 8 bf16 = one 64-byte output row segment
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x4 bv = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + nb + 8 * g + nq) : f32x4{0.f, 0.f, 0.f, 0.f};
                        const f32x4 bg = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + nb + 32 + 8 * g + nq) : f32x4{0.f, 0.f, 0.f, 0.f};
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            y[e] = (acc[mi][0][4 * g + e] * p.alpha + bv[e]) * gelu_gate(acc[mi][1][4 * g + e] * p.alpha + bg[e], p.a_bf16 == H16_BF16 || (kF16FastGate && p.a_bf16 == H16_FP16));
                        *reinterpret_cast<f32x4*>(st + mrow * SLD + 8 * g + nq) = y;
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int row = (lane >> 2) + 16 * i;
                        const int m = bm * BM + wm * WM + mi * 32 + row;
                        if (m < p.M) {
                            const f32x4 y0 = *reinterpret_cast<const f32x4*>(st + row * SLD + col);
                            const f32x4 y1 = *reinterpret_cast<const f32x4*>(st + row * SLD + col + 4);
                            hx8<H> o;
#pragma unroll
                            for (int e = 0; e < 4; ++e) { o[e] = (H)y0[e]; o[4 + e] = (H)y1[e]; }
                            *reinterpret_cast<hx8<H>*>(out + (size_t)m * p.ldc + nb / 2 + col) = o;
                        }
                    }
                }
            }
        }
        return;
    }
    const bool vec = ((p.N | p.ldc | p.ldr) & 7) == 0 && (p.rb_ld & 3) == 0;
    if (vec) {
        constexpr int SLD = SWZ ? WN : WN + 4;
        constexpr int LPR = WN / 8;                            // lanes per staged row (8 columns each)
        constexpr int RPI = 64 / LPR;                          // rows per access instruction
        float* st = stage + (size_t)(threadIdx.x >> 6) * 32 * SLD;
        const int col = (lane % LPR) * 8;
        auto swz = [](const int row) { return !SWZ ? 0 : (WN == 64 ? (row & 15) : ((row >> 1) & 7)); };
        const int wsw = swz(mrow);
        const int n = n0 + wn * WN + col;
        f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
        if (p.bias && n < p.N) {
            b0 = *reinterpret_cast<const f32x4*>(p.bias + n);
            b1 = *reinterpret_cast<const f32x4*>(p.bias + n + 4);
        }
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = acc[mi][ni][4 * g + e];
                    *reinterpret_cast<f32x4*>(st + mrow * SLD + (((ni * 8 + 2 * g + (lane >> 5)) ^ wsw) << 2)) = y;
                }
#pragma unroll
            for (int i = 0; i < 32 / RPI; ++i) {
                const int row = lane / LPR + RPI * i;
                const int m = bm * BM + wm * WM + mi * 32 + row;
                if (m >= p.M || n >= p.N || (p.ablate & 1)) continue;   // N % 8 == 0: the lane's eight columns are in or out together
                const int rsw = swz(row);
                f32x4 y0 = *reinterpret_cast<const f32x4*>(st + row * SLD + ((((col >> 2)) ^ rsw) << 2));
                f32x4 y1 = *reinterpret_cast<const f32x4*>(st + row * SLD + ((((col >> 2) + 1) ^ rsw) << 2));
                if (p.alpha != 1.0f) { y0 *= p.alpha; y1 *= p.alpha; }
                y0 += b0; y1 += b1;
                if (p.rowbias) {
                    const float* rb = p.rowbias + (size_t)(m / p.rows_per_sample) * p.rb_ld + n;
                    y0 += *reinterpret_cast<const f32x4*>(rb);
                    y1 += *reinterpret_cast<const f32x4*>(rb + 4);
                }
                if (p.resid) {
                    if (p.resid_bf16) {
                        const hx8<H> r = *reinterpret_cast<const hx8<H>*>(reinterpret_cast<const H*>(p.resid) + (size_t)m * p.ldr + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) { y0[e] += (float)r[e]; y1[e] += (float)r[4 + e]; }
                    } else {
                        y0 += *reinterpret_cast<const f32x4*>(p.resid + (size_t)m * p.ldr + n);
                        y1 += *reinterpret_cast<const f32x4*>(p.resid + (size_t)m * p.ldr + n + 4);
                    }
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { y0[e] = fmaxf(y0[e], 0.f); y1[e] = fmaxf(y1[e], 0.f); }
                }
                hx8<H> o;
#pragma unroll
                for (int e = 0; e < 4; ++e) { o[e] = (H)y0[e]; o[4 + e] = (H)y1[e]; }
                *reinterpret_cast<hx8<H>*>(out + (size_t)m * p.ldc + n) = o;
            }
        }
        return;
    }
    // scalar fallback (N or a stride not a multiple of 8)
#pragma unroll
    for (int mi = 0; mi < TM; ++mi) {
        const int m = bm * BM + wm * WM + mi * 32 + mrow;
        if (m >= p.M) continue;
        const float* rbp = p.rowbias ? p.rowbias + (size_t)(m / p.rows_per_sample) * p.rb_ld : nullptr;
        H* orow = out + (size_t)m * p.ldc;
#pragma unroll
        for (int ni = 0; ni < TN; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * WN + ni * 32 + 8 * g + nq;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if (n + e >= p.N) break;
                    float v = acc[mi][ni][4 * g + e] * p.alpha + (p.bias ? p.bias[n + e] : 0.f);
                    if (rbp) v += rbp[n + e];
                    if (p.resid) v += p.resid_bf16 ? (float)reinterpret_cast<const H*>(p.resid)[(size_t)m * p.ldr + n + e]
                                                   : p.resid[(size_t)m * p.ldr + n + e];
                    if (p.relu) v = fmaxf(v, 0.f);
                    orow[n + e] = (H)v;
                }
            }
    }
}

// The same epilogue cut in two for the persistent kernel (bgemm.hip).  `prefetch` issues the only global loads the epilogue
// has left -- the bf16 residual -- BEFORE the caller starts the next tile's first stage, so that they are older than that DMA
// in the wave's in-order vmcnt queue and waiting for them never waits for it.  Bias and time-embedding rows do not come from
// global memory here: the caller has put them into LDS for the tile's 128 columns -- `brow[0][128]` = bias, `brow[1 + j][128]` =
// rowbias of sample s_lo + j, j = 0, 1 (a tile's rows belong to at most two samples; sample of row m = m / rows_per_sample).  `finish` stages the
// accumulators through `st` (this wave's 32 x WN floats, unpadded and chunk-swizzled as above), adds, rounds once and stores.
// Residuals are bf16 (the launcher sends an fp32 residual to the non-persistent kernels).
template <typename H, int BM, int TM, int TN, int WM, int WN, bool ROWBIAS = true>      // H: bf16 / fp16; ROWBIAS false: launches that never carry one (linears)
struct BgEpilogue {
    static constexpr int LPR = WN / 8, RPI = 64 / LPR, NI = 32 / RPI;
    hx8<H> res[TM][NI];
    bool vec;

    __device__ __forceinline__ void prefetch(const IgemmArgs& p, const int bm, const int n0, const int wm, const int wn, const int lane) {
        vec = ((p.N | p.ldc | p.ldr) & 7) == 0;
        if (p.geglu || !vec || !p.resid) return;
        // branch-free (a load under a branch cannot be counted by the compiler's vmcnt bookkeeping, which then drains the queue
        // -- the next tile's DMA included -- at the first use): buffer loads against a descriptor based at the tile's first
        // residual row, rows / columns outside the matrix as out-of-window offsets
        const int n = n0 + wn * WN + (lane % LPR) * 8;
        const unsigned long long base = reinterpret_cast<unsigned long long>(reinterpret_cast<const H*>(p.resid) + (size_t)bm * BM * p.ldr);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)base);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo), (short)0,
                                                                            0x7FFFFFF0, 0x00020000);
        // (the empty asm keeps the per-row offsets from being hoisted out of the caller's tile loop as eight loop-invariant
        // registers, which the allocator then spills: a scratch reload in the epilogue is a vmcnt wait behind the DMA)
        unsigned off0 = (unsigned)(((wm * WM + lane / LPR) * p.ldr + n) * 2);
        asm volatile("" : "+v"(off0));
#pragma unroll
        for (int mi = 0; mi < TM; ++mi)
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int row = wm * WM + mi * 32 + lane / LPR + RPI * i;
                const bool ok = bm * BM + row < p.M && n < p.N;
                const unsigned off = ok ? off0 + (unsigned)((mi * 32 + RPI * i) * p.ldr * 2) : 0x80000000u;
                const u32x4 r = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0);
                res[mi][i] = __builtin_bit_cast(hx8<H>, r);
            }
    }

    // WAIT false: no counted vmcnt at the end (the caller runs several finish() calls behind one DMA and waits once, for the sum
    // of their stores: STORES each, when vec / geglu hold)
    static constexpr int STORES = TM * NI, STORES_GEGLU = TM * 2;
    template <bool WAIT = true>
    __device__ __forceinline__ void finish(const IgemmArgs& p, f32x16 (&acc)[TM][TN], H* __restrict__ out, const int bm, const int n0,
                                           const int wm, const int wn, const int lane, float* st, const float* brow, const int s_lo) {
        const int mrow = lane & 31;
        const int nq = (lane >> 5) * 4;
        // stores: buffer stores against a descriptor based at the tile's first output row, masked elements as out-of-window
        // offsets (dropped by the buffer unit) -- issued unconditionally, so that the number of stores behind the next tile's
        // DMA is a compile-time constant and the wait in front of the barrier can be COUNTED (vmcnt(stores)): the DMA has
        // landed, the stores are left in flight
        const unsigned long long obase = reinterpret_cast<unsigned long long>(out + (size_t)bm * BM * p.ldc);
        const unsigned olo = __builtin_amdgcn_readfirstlane((unsigned)obase);
        const unsigned ohi = __builtin_amdgcn_readfirstlane((unsigned)(obase >> 32));
        const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)ohi << 32) | olo), (short)0,
                                                                             0x7FFFFFF0, 0x00020000);
        const bool drop = (p.ablate & 1) != 0;
        if (p.geglu) {
            if constexpr (TN == 2) {
                const int nb = n0 + wn * WN;
                if (nb + 64 > p.N) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    return;
                }
                const int col = (lane & 3) * 8;                    // 4 lanes x 8 bf16 = one 64-byte output row segment
                const int wsw = (mrow >> 1) & 7;                   // 32-float staging rows
                f32x4 gv[4], gg[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    gv[g] = *reinterpret_cast<const f32x4*>(brow + wn * WN + 8 * g + nq);
                    gg[g] = *reinterpret_cast<const f32x4*>(brow + wn * WN + 32 + 8 * g + nq);
                }
#pragma unroll
                for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        f32x4 y;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            y[e] = (acc[mi][0][4 * g + e] * p.alpha + gv[g][e]) * gelu_gate(acc[mi][1][4 * g + e] * p.alpha + gg[g][e], p.a_bf16 == H16_BF16 || (kF16FastGate && p.a_bf16 == H16_FP16));
                        *reinterpret_cast<f32x4*>(st + mrow * 32 + (((2 * g + (lane >> 5)) ^ wsw) << 2)) = y;
                    }
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int row = (lane >> 2) + 16 * i;
                        const int m = bm * BM + wm * WM + mi * 32 + row;
                        const int rsw = (row >> 1) & 7;
                        const f32x4 y0 = *reinterpret_cast<const f32x4*>(st + row * 32 + (((col >> 2) ^ rsw) << 2));
                        const f32x4 y1 = *reinterpret_cast<const f32x4*>(st + row * 32 + ((((col >> 2) + 1) ^ rsw) << 2));
                        hx8<H> o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) { o[e] = (H)y0[e]; o[4 + e] = (H)y1[e]; }
                        const unsigned off = (m < p.M && !drop) ? (unsigned)(((wm * WM + mi * 32 + row) * p.ldc + nb / 2 + col) * 2) : 0x80000000u;
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ors, off, 0, 0);
                    }
                }
                if constexpr (WAIT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TM * 2) : "memory");
                return;
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            return;
        }
        if (!vec) {                                            // N or a stride not a multiple of 8: element-wise, no staging
#pragma unroll
            for (int mi = 0; mi < TM; ++mi) {
                const int m = bm * BM + wm * WM + mi * 32 + mrow;
                if (m >= p.M) continue;
                const float* bb = brow + wn * WN;
                const float* br = brow + 128 + ((ROWBIAS && p.rowbias) ? (m / p.rows_per_sample - s_lo) * 128 : 0) + wn * WN;
                H* orow = out + (size_t)m * p.ldc;
#pragma unroll
                for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = ni * 32 + 8 * g + nq;
                        const int n = n0 + wn * WN + c;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (n + e >= p.N) break;
                            float v = acc[mi][ni][4 * g + e] * p.alpha + bb[c + e];
                            if (ROWBIAS && p.rowbias) v += br[c + e];
                            if (p.resid) v += (float)reinterpret_cast<const H*>(p.resid)[(size_t)m * p.ldr + n + e];
                            if (p.relu) v = fmaxf(v, 0.f);
                            orow[n + e] = (H)v;
                        }
                    }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            return;
        }
        auto swz = [](const int row) { return WN == 64 ? (row & 15) : ((row >> 1) & 7); };
        const int wsw = swz(mrow);
        const int col = (lane % LPR) * 8;
        const int n = n0 + wn * WN + col;
        unsigned ooff0 = (unsigned)(((wm * WM + lane / LPR) * p.ldc + n) * 2);
        asm volatile("" : "+v"(ooff0));                    // as in prefetch(): recomputed per tile, not eight spilled invariants
#pragma unroll
        for (int mi = 0; mi < TM; ++mi) {
#pragma unroll
            for (int ni = 0; ni < TN; ++ni)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 y;
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = acc[mi][ni][4 * g + e];
                    *reinterpret_cast<f32x4*>(st + mrow * WN + (((ni * 8 + 2 * g + (lane >> 5)) ^ wsw) << 2)) = y;
                }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int row = lane / LPR + RPI * i;
                const int m = bm * BM + wm * WM + mi * 32 + row;
                const int rsw = swz(row);
                f32x4 y0 = *reinterpret_cast<const f32x4*>(st + row * WN + (((col >> 2) ^ rsw) << 2));
                f32x4 y1 = *reinterpret_cast<const f32x4*>(st + row * WN + ((((col >> 2) + 1) ^ rsw) << 2));
                const float* bb = brow + wn * WN + col;
                if (p.alpha != 1.0f) { y0 *= p.alpha; y1 *= p.alpha; }
                y0 += *reinterpret_cast<const f32x4*>(bb);
                y1 += *reinterpret_cast<const f32x4*>(bb + 4);
                if (ROWBIAS && p.rowbias) {                        // separately, in the order of the tile kernels: bit-identical results
                    const float* br = bb + 128 + (m < p.M ? (m / p.rows_per_sample - s_lo) * 128 : 0);
                    y0 += *reinterpret_cast<const f32x4*>(br);
                    y1 += *reinterpret_cast<const f32x4*>(br + 4);
                }
                if (p.resid) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { y0[e] += (float)res[mi][i][e]; y1[e] += (float)res[mi][i][4 + e]; }
                }
                if (p.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { y0[e] = fmaxf(y0[e], 0.f); y1[e] = fmaxf(y1[e], 0.f); }
                }
                hx8<H> o;
#pragma unroll
                for (int e = 0; e < 4; ++e) { o[e] = (H)y0[e]; o[4 + e] = (H)y1[e]; }
                const unsigned off = (m < p.M && n < p.N && !drop) ? ooff0 + (unsigned)((mi * 32 + RPI * i) * p.ldc * 2) : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), ors, off, 0, 0);
            }
        }
        if constexpr (WAIT) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(TM * NI) : "memory");
    }
};

}  // namespace e2v
