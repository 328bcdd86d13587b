// Winograd F(2x2, 3x3) form of the stride-1 3x3 convolutions of ResnetBlock3D / Upsample3D (resnet.py:58-66,
// 180, 197) and of the VAE's resnets: 16 multiplies per 2x2 output tile instead of 36, i.e. 2.25x fewer
// matrix-core flops than the direct implicit GEMM, paid for with two HBM-bound transform passes.
//
//   V[k][t][c] = (B^T d B)[k]        d = 4x4 input patch of tile t, channel c            (wino_in_kernel)
//   M[k][t][o] = sum_c V[k][t][c] U[k][o][c]      16 independent GEMMs = igemm(), batch 16
//   y[2x2]     = A^T M A (+ bias, time-embedding row, residual)                          (wino_out_kernel)
//   U[k][o][c] = (G g G^T)[k]        once, at e2v_finalize_weights                       (wino_weight_kernel)
//
// The input transform also absorbs what precedes the conv in the graph: the channel concat of the up blocks
// (two sources), the nearest 2x resize of Upsample3D (torch's fp32-scale index formula) and, for the resnets,
// the GroupNorm affine + SiLU (per-(slab, channel) scale / shift from groupnorm_stats) -- the normalised
// activation is then never written to HBM.  Zero padding is applied after the activation, as F.conv2d does.
//
// fp32 throughout; F(2x2, 3x3) has transform constants 0, +-1, +-1/2 only, its rounding error stays within a small
// multiple of the direct sum's (tests/test_hip_ops.py::test_conv3x3_winograd pins 2e-5 relative to the output scale).
#include "kernels.h"
#include "prof.h"
#include "runtime.h"

#include <algorithm>
#include <string>

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// x * sigmoid(x) on the hardware transcendentals (v_exp_f32, v_rcp_f32: 1 ulp each).  The input transforms evaluate it
// up to 2.25x per element (once per tile that touches the pixel), so the IEEE expf + division of norm.hip's
// gn_apply_kernel would make these HBM-bound kernels ALU-bound; the two forms differ by ~1e-7 relative.
__device__ __forceinline__ float wino_silu(float v) {
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.44269504088896340736f));
}

// a / b in 32 bits whenever both fit (the 64-bit form is a ~100-instruction sequence, paid per thread and tile)
__device__ __forceinline__ size_t wino_div(size_t a, size_t b) {
    return ((a | b) >> 32) == 0 ? (size_t)((unsigned)a / (unsigned)b) : a / b;
}

// The transform planes (V, M) are [tile][channel] matrices one `plane` apart: a wave-uniform plane base plus one 32-bit byte
// offset per thread, the same for every plane, instead of a 64-bit address per access.
// (The empty asm pins the base to scalar registers: left alone, the compiler chains the plane addresses per thread in VGPR pairs.)
#define WINO_GLOBAL __attribute__((address_space(1)))
__device__ __forceinline__ f32x4 wino_plane_load(const float* plane_base, unsigned byte_off) {
    asm("" : "+s"(plane_base));
    return *reinterpret_cast<const WINO_GLOBAL f32x4*>((const WINO_GLOBAL char*)plane_base + byte_off);
}
__device__ __forceinline__ void wino_plane_store(float* plane_base, unsigned byte_off, f32x4 v) {
    asm("" : "+s"(plane_base));
    *reinterpret_cast<WINO_GLOBAL f32x4*>((WINO_GLOBAL char*)plane_base + byte_off) = v;
}

// What precedes the conv, applied to one loaded quad: GN = the GroupNorm affine + SiLU of the resnets.  A padding position
// contributes exactly 0 (F.conv2d pads AFTER the activation): its load went to a clamped in-range address and the masking
// comes last, so the loads of a tile never wait for a branch.
template <bool GN>
__device__ __forceinline__ f32x4 wino_act(f32x4 v, const f32x4& ga, const f32x4& gb, bool ok) {
    if (GN) {
        v[0] = v[0] * ga[0] + ga[1];
        v[1] = v[1] * ga[2] + ga[3];
        v[2] = v[2] * gb[0] + gb[1];
        v[3] = v[3] * gb[2] + gb[3];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = wino_silu(v[e]);
    }
    // Written as an integer AND, not as `ok ? v : 0`: the optimiser folds the transform's constant multiplies into a float select
    // with a zero arm, and bt6 then fuses other products into FMAs than it does for a plain value (12 of the first pass's packed
    // products with hipcc of ROCm 7.2), i.e. V rounds differently.  The back end may still emit v_cndmask for the AND; what matters
    // is which products are fused.  Nothing guarantees it across compilers: after a compiler update compare the operand patterns
    // of v_pk_fma_f32 / v_pk_mul_f32 in wino4_in_kernel with the previous build's, or compare two `bench.py --dump-outputs` runs.
    const u32x4 keep = ok ? ~0u : 0u;
    return __builtin_bit_cast(f32x4, __builtin_bit_cast(u32x4, v) & keep);
}

// Source offsets (in floats, inside one image) of the PATCH rows / columns of a tile that starts at output coordinate o0 - 1:
// clamped to coordinate 0 outside the map, through the nearest resize where there is one, scaled by `step` floats.
template <int PATCH>
__device__ __forceinline__ void wino_patch_offsets(int o0, int n_out, int n_src, bool upsample, float ups, unsigned step,
                                                   unsigned (&off)[PATCH], bool (&ok)[PATCH]) {
#pragma unroll
    for (int r = 0; r < PATCH; ++r) {
        const int i = o0 - 1 + r;
        ok[r] = (unsigned)i < (unsigned)n_out;
        int s = ok[r] ? i : 0;
        if (upsample) s = min((int)floorf((float)s * ups), n_src - 1);
        off[r] = (unsigned)s * step;
    }
}

// one thread = one tile x four channels; consecutive threads = consecutive channel quads (16-byte lanes, coalesced).
// All 16 patch loads of a tile are issued before the first is consumed.
template <bool GN>
__global__ __launch_bounds__(256) void wino_in_kernel(const WinoArgs p, int img_lo, int nimg, float* __restrict__ V) {
    const int Ctot = p.c0 + p.c1;
    const int CQ = Ctot / 4;
    const int th = (p.Ho + 1) / 2, tw = (p.Wo + 1) / 2;
    const size_t T = (size_t)nimg * th * tw;
    const size_t total = T * CQ;
    const size_t plane = T * Ctot;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = wino_div(i, CQ);
        const int c = (int)(i - t * CQ) * 4;
        const int img = (int)wino_div(t, th * tw);
        const int rem = (int)(t - (size_t)img * th * tw);
        const int ty = rem / tw, tx = rem - ty * tw;
        const bool second = c >= p.c0;
        const int ld = second ? p.ld1 : p.ld0;
        const size_t img_row = (size_t)(img_lo + img) * p.Hs * p.Ws;
        const float* __restrict__ src = (second ? p.x1 + (c - p.c0) : p.x0 + c) + img_row * ld;
        f32x4 ga = {1.f, 0.f, 1.f, 0.f}, gb = {1.f, 0.f, 1.f, 0.f};
        if (GN) {                                          // (scale, shift) pairs of the 4 channels
            const size_t slab = wino_div(img_row, (size_t)p.gn_P);
            const float* sc = p.gn_scsh + (slab * Ctot + c) * 2;
            ga = *reinterpret_cast<const f32x4*>(sc);
            gb = *reinterpret_cast<const f32x4*>(sc + 4);
        }
        unsigned yo[4], xo[4];
        bool yok[4], xok[4];
        wino_patch_offsets<4>(2 * ty, p.Ho, p.Hs, p.upsample, p.ups_h, (unsigned)p.Ws * ld, yo, yok);
        wino_patch_offsets<4>(2 * tx, p.Wo, p.Ws, p.upsample, p.ups_w, (unsigned)ld, xo, xok);
        f32x4 d[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) d[r][q] = *reinterpret_cast<const f32x4*>(src + (yo[r] + xo[q]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) d[r][q] = wino_act<GN>(d[r][q], ga, gb, yok[r] && xok[q]);
        // B^T d B,  B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
        f32x4 u[4][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            u[0][q] = d[0][q] - d[2][q];
            u[1][q] = d[1][q] + d[2][q];
            u[2][q] = d[2][q] - d[1][q];
            u[3][q] = d[1][q] - d[3][q];
        }
        const unsigned vo = ((unsigned)t * Ctot + c) * 4u;     // byte offset inside a plane (32 bits: wino_conv3x3 checks)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wino_plane_store(V + (size_t)(4 * r + 0) * plane, vo, u[r][0] - u[r][2]);
            wino_plane_store(V + (size_t)(4 * r + 1) * plane, vo, u[r][1] + u[r][2]);
            wino_plane_store(V + (size_t)(4 * r + 2) * plane, vo, u[r][2] - u[r][1]);
            wino_plane_store(V + (size_t)(4 * r + 3) * plane, vo, u[r][1] - u[r][3]);
        }
    }
}

// What the output transforms share per tile of M x M output pixels.  A tile lies in one image: one 64-bit base per tensor, the
// pixels at 32-bit offsets from it; a ragged tile's missing pixels are not stored, and their residual loads go to the tile's
// first row / column (in range, unused).  RB: 0 no rowbias, 1 one rowbias row per tile (a sample is whole images: the graph),
// 2 one per pixel (any rows_per_sample).
template <int M, int RB, bool RES>
struct WinoTileOut {
    float* out;
    const float* res;
    size_t row0;
    unsigned yc[M], xc[M], yr[M], xr[M];
    bool yok[M], xok[M];
    f32x4 bias, rb;
    f32x4 r[M][M];

    __device__ __forceinline__ WinoTileOut(const WinoArgs& p, int img, int ty, int tx, int n) {
        const int oy0 = M * ty, ox0 = M * tx;
        row0 = ((size_t)img * p.Ho + oy0) * p.Wo + ox0;
        out = p.out + row0 * p.ldc + n;
        res = RES ? p.resid + row0 * p.ldr + n : nullptr;
#pragma unroll
        for (int a = 0; a < M; ++a) {
            yok[a] = oy0 + a < p.Ho;
            xok[a] = ox0 + a < p.Wo;
            yc[a] = (unsigned)(a * p.Wo) * p.ldc;
            xc[a] = (unsigned)a * p.ldc;
            yr[a] = yok[a] ? (unsigned)(a * p.Wo) * p.ldr : 0u;
            xr[a] = xok[a] ? (unsigned)a * p.ldr : 0u;
        }
        bias = f32x4{0.f, 0.f, 0.f, 0.f};
        rb = bias;
        if (p.bias) bias = *reinterpret_cast<const f32x4*>(p.bias + n);
        if (RB == 1) rb = *reinterpret_cast<const f32x4*>(p.rowbias + wino_div(row0, (size_t)p.rows_per_sample) * p.rb_ld + n);
    }
    // all residual loads of the tile, issued with the loads of M and ahead of every use
    __device__ __forceinline__ void load_resid() {
        if (!RES) return;
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
            for (int b = 0; b < M; ++b) r[a][b] = *reinterpret_cast<const f32x4*>(res + (yr[a] + xr[b]));
    }
    // y + bias, + rowbias, + resid (in this order) and the stores.  The stores of a ragged tile sit in branches; every load of the
    // tile is waited for once, explicitly, in front of them: left to the compiler, each branch gets its own vmcnt(0) wait, which on
    // gfx9 also waits for the stores before it.
    // (The empty asm keeps the transform arithmetic in front of that wait, where it overlaps the residual loads: the compiler
    // otherwise sinks it into the branches, each pixel's share behind the wait, and keeps all of M live until the last store.)
    __device__ __forceinline__ void finish(const WinoArgs& p, int n, f32x4 (&y)[M][M]) const {
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
            for (int b = 0; b < M; ++b) asm volatile("" : "+v"(y[a][b]));
        __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0)
#pragma unroll
        for (int a = 0; a < M; ++a)
#pragma unroll
            for (int b = 0; b < M; ++b) {
                if (!(yok[a] && xok[b])) continue;
                f32x4 v = y[a][b] + bias;
                if (RB == 1) v += rb;
                if (RB == 2) {
                    const size_t row = row0 + (size_t)a * p.Wo + b;
                    v += *reinterpret_cast<const f32x4*>(p.rowbias + wino_div(row, (size_t)p.rows_per_sample) * p.rb_ld + n);
                }
                if (RES) v += r[a][b];
                *reinterpret_cast<f32x4*>(out + (yc[a] + xc[b])) = v;
            }
    }
};

// one thread = one tile x four output channels: y = A^T M A,  A^T = [1 1 1 0; 0 1 -1 -1]
template <int RB, bool RES>
__global__ __launch_bounds__(256) void wino_out_kernel(const WinoArgs p, int img_lo, int nimg, const float* __restrict__ Mb) {
    const int NQ = p.N / 4;
    const int th = (p.Ho + 1) / 2, tw = (p.Wo + 1) / 2;
    const size_t T = (size_t)nimg * th * tw;
    const size_t total = T * NQ;
    const size_t plane = T * p.N;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = wino_div(i, NQ);
        const int n = (int)(i - t * NQ) * 4;
        const int img = (int)wino_div(t, th * tw);
        const int rem = (int)(t - (size_t)img * th * tw);
        const int ty = rem / tw, tx = rem - ty * tw;
        const unsigned mo = ((unsigned)t * p.N + n) * 4u;      // byte offset inside a plane (32 bits: wino_conv3x3 checks)
        f32x4 mm[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) mm[k] = wino_plane_load(Mb + (size_t)k * plane, mo);
        WinoTileOut<2, RB, RES> tile(p, img_lo + img, ty, tx, n);
        tile.load_resid();
        __builtin_amdgcn_sched_barrier(0);
        f32x4 w[2][4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            w[0][q] = mm[q] + mm[4 + q] + mm[8 + q];
            w[1][q] = mm[4 + q] - mm[8 + q] - mm[12 + q];
        }
        f32x4 y[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            y[a][0] = w[a][0] + w[a][1] + w[a][2];
            y[a][1] = w[a][1] - w[a][2] - w[a][3];
        }
        tile.finish(p, n, y);
    }
}

// ---------------------------------------------------------------------------------------------------------
// F(4x4, 3x3): 36 multiplies per 4x4 output tile instead of 144 (4x fewer than direct, 1.78x fewer than F(2x2)).
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]
// Transform constants up to 8 make its fp32 rounding error ~17x the direct sum's (5e-6 of the output scale on a
// 640-channel conv): opt-in (E2V_CONV_WINOGRAD4 / E2V_WINO_F4), see DESIGN 3.6.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void bt6(const f32x4 (&d)[6], f32x4 (&o)[6]) {
    o[0] = 4.f * d[0] - 5.f * d[2] + d[4];
    o[1] = -4.f * (d[1] + d[2]) + d[3] + d[4];
    o[2] = 4.f * (d[1] - d[2]) - d[3] + d[4];
    o[3] = 2.f * (d[3] - d[1]) - d[2] + d[4];
    o[4] = 2.f * (d[1] - d[3]) - d[2] + d[4];
    o[5] = 4.f * d[1] - 5.f * d[3] + d[5];
}
__device__ __forceinline__ void at6(const f32x4 (&m)[6], f32x4 (&o)[4]) {
    const f32x4 a = m[1] + m[2], b = m[1] - m[2], c = m[3] + m[4], e = m[3] - m[4];
    o[0] = m[0] + a + c;
    o[1] = b + 2.f * e;
    o[2] = a + 4.f * c;
    o[3] = b + 8.f * e + m[5];
}

// All 36 patch loads of a tile are issued before the first is consumed, with or without the GroupNorm in front (two resident
// waves per SIMD cannot cover 36 chained memory latencies per tile).
template <bool GN>
__global__ __launch_bounds__(256) void wino4_in_kernel(const WinoArgs p, int img_lo, int nimg, float* __restrict__ V) {
    const int Ctot = p.c0 + p.c1;
    const int CQ = Ctot / 4;
    const int th = (p.Ho + 3) / 4, tw = (p.Wo + 3) / 4;
    const size_t T = (size_t)nimg * th * tw;
    const size_t total = T * CQ;
    const size_t plane = T * Ctot;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = wino_div(i, CQ);
        const int c = (int)(i - t * CQ) * 4;
        const int img = (int)wino_div(t, th * tw);
        const int rem = (int)(t - (size_t)img * th * tw);
        const int ty = rem / tw, tx = rem - ty * tw;
        const bool second = c >= p.c0;
        const int ld = second ? p.ld1 : p.ld0;
        const size_t img_row = (size_t)(img_lo + img) * p.Hs * p.Ws;
        const float* __restrict__ src = (second ? p.x1 + (c - p.c0) : p.x0 + c) + img_row * ld;
        f32x4 ga = {1.f, 0.f, 1.f, 0.f}, gb = {1.f, 0.f, 1.f, 0.f};
        if (GN) {
            const size_t slab = wino_div(img_row, (size_t)p.gn_P);
            const float* sc = p.gn_scsh + (slab * Ctot + c) * 2;
            ga = *reinterpret_cast<const f32x4*>(sc);
            gb = *reinterpret_cast<const f32x4*>(sc + 4);
        }
        unsigned yo[6], xo[6];
        bool yok[6], xok[6];
        wino_patch_offsets<6>(4 * ty, p.Ho, p.Hs, p.upsample, p.ups_h, (unsigned)p.Ws * ld, yo, yok);
        wino_patch_offsets<6>(4 * tx, p.Wo, p.Ws, p.upsample, p.ups_w, (unsigned)ld, xo, xok);
        f32x4 d[6][6];                                         // [patch column][patch row]
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int r = 0; r < 6; ++r) d[q][r] = *reinterpret_cast<const f32x4*>(src + (yo[r] + xo[q]));
        __builtin_amdgcn_sched_barrier(0);                     // (the scheduler otherwise trades the batch for registers: load, wait, use)
        // column pass first (B^T d), one patch column at a time so that the 6x6 intermediate replaces the patch in place
        f32x4 u[6][6];
#pragma unroll
        for (int q = 0; q < 6; ++q) {
#pragma unroll
            for (int r = 0; r < 6; ++r) d[q][r] = wino_act<GN>(d[q][r], ga, gb, xok[q] && yok[r]);
            f32x4 o[6];
            bt6(d[q], o);
#pragma unroll
            for (int r = 0; r < 6; ++r) u[r][q] = o[r];
        }
        const unsigned vo = ((unsigned)t * Ctot + c) * 4u;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            f32x4 v[6];
            bt6(u[r], v);
#pragma unroll
            for (int q = 0; q < 6; ++q) wino_plane_store(V + (size_t)(6 * r + q) * plane, vo, v[q]);
        }
    }
}

template <int RB, bool RES>
__global__ __launch_bounds__(256) void wino4_out_kernel(const WinoArgs p, int img_lo, int nimg, const float* __restrict__ Mb) {
    const int NQ = p.N / 4;
    const int th = (p.Ho + 3) / 4, tw = (p.Wo + 3) / 4;
    const size_t T = (size_t)nimg * th * tw;
    const size_t total = T * NQ;
    const size_t plane = T * p.N;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t t = wino_div(i, NQ);
        const int n = (int)(i - t * NQ) * 4;
        const int img = (int)wino_div(t, th * tw);
        const int rem = (int)(t - (size_t)img * th * tw);
        const int ty = rem / tw, tx = rem - ty * tw;
        const unsigned mo = ((unsigned)t * p.N + n) * 4u;
        f32x4 col[6][6];                                       // [column of M][row]
#pragma unroll
        for (int q = 0; q < 6; ++q)
#pragma unroll
            for (int r = 0; r < 6; ++r) col[q][r] = wino_plane_load(Mb + (size_t)(6 * r + q) * plane, mo);
        WinoTileOut<4, RB, RES> tile(p, img_lo + img, ty, tx, n);
        tile.load_resid();
        __builtin_amdgcn_sched_barrier(0);                     // (M and the residual: one batch of loads, nothing moved in between)
        f32x4 w[4][6];                                         // A^T M, one column of M at a time
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            f32x4 o[4];
            at6(col[q], o);
#pragma unroll
            for (int a = 0; a < 4; ++a) w[a][q] = o[a];
        }
        f32x4 y[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a) at6(w[a], y[a]);
        tile.finish(p, n, y);
    }
}

// [O][I][3][3] -> U[36][O][I] = G g G^T
__global__ void wino4_weight_kernel(const float* __restrict__ w, float* __restrict__ U, int cout, int cin) {
    const size_t total = (size_t)cout * cin;
    const float G[6][3] = {{0.25f, 0.f, 0.f}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                           {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float* g = w + i * 9;
        float t[6][3];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int x = 0; x < 3; ++x) t[r][x] = G[r][0] * g[x] + G[r][1] * g[3 + x] + G[r][2] * g[6 + x];
#pragma unroll
        for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int q = 0; q < 6; ++q)
                U[(size_t)(6 * r + q) * total + i] = t[r][0] * G[q][0] + t[r][1] * G[q][1] + t[r][2] * G[q][2];
    }
}

// [O][I][3][3] -> U[16][O][I] = G g G^T,  G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
__global__ void wino_weight_kernel(const float* __restrict__ w, float* __restrict__ U, int cout, int cin) {
    const size_t total = (size_t)cout * cin;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float* g = w + i * 9;
        float t[4][3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            t[0][x] = g[x];
            t[1][x] = 0.5f * (g[x] + g[3 + x] + g[6 + x]);
            t[2][x] = 0.5f * (g[x] - g[3 + x] + g[6 + x]);
            t[3][x] = g[6 + x];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            U[(size_t)(4 * r + 0) * total + i] = t[r][0];
            U[(size_t)(4 * r + 1) * total + i] = 0.5f * (t[r][0] + t[r][1] + t[r][2]);
            U[(size_t)(4 * r + 2) * total + i] = 0.5f * (t[r][0] - t[r][1] + t[r][2]);
            U[(size_t)(4 * r + 3) * total + i] = t[r][2];
        }
    }
}

void wino_pack_weights(const float* w_oihw, float* U, int cout, int cin, int m, hipStream_t s) {
    const size_t total = (size_t)cout * cin;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    if (m == 4) E2V_KLAUNCH(wino4_weight_kernel, dim3(blocks), dim3(256), 0, s, w_oihw, U, cout, cin);
    else E2V_KLAUNCH(wino_weight_kernel, dim3(blocks), dim3(256), 0, s, w_oihw, U, cout, cin);
}

static inline size_t wino_tiles(const WinoArgs& a, int nimg) {
    return (size_t)nimg * ((a.Ho + a.m - 1) / a.m) * ((a.Wo + a.m - 1) / a.m);
}

size_t wino_workspace_floats(const WinoArgs& a, int nimg) {
    return (size_t)(a.m + 2) * (a.m + 2) * wino_tiles(a, nimg) * (size_t)(a.c0 + a.c1 + a.N);
}

int wino_chunk_images(const WinoArgs& a, size_t max_floats) {
    const size_t per_img = wino_workspace_floats(a, 1);
    size_t n = max_floats / (per_img ? per_img : 1);
    if (n < 1) n = 1;
    return (int)(n < (size_t)a.nimg ? n : (size_t)a.nimg);
}

using WinoInKernel = void (*)(const WinoArgs, int, int, float*);
using WinoOutKernel = void (*)(const WinoArgs, int, int, const float*);

void wino_conv3x3(const WinoArgs& a, float* ws, int chunk_images, hipStream_t s) {
    const int Ctot = a.c0 + a.c1;
    const int P = (a.m + 2) * (a.m + 2);                          // 16 or 36 GEMMs
    // the transforms address the pixels of one image / one tile by 32-bit offsets from a 64-bit base
    const int ldmax = std::max(std::max(a.ld0, a.ld1), std::max(a.ldc, a.ldr));
    E2V_REQUIRE((uint64_t)a.Hs * a.Ws * ldmax < ((uint64_t)1 << 32) && (uint64_t)(a.m + 1) * a.Wo * ldmax < ((uint64_t)1 << 32) &&
                    (uint64_t)wino_tiles(a, std::min(chunk_images, a.nimg)) * std::max(Ctot, a.N) < ((uint64_t)1 << 30),
                E2V_ESHAPE, "winograd conv: an image or a transform plane exceeds 32-bit offsets");
    // what is fixed per launch selects the kernel: the activation in front, the rowbias form (a sample made of whole images -- every
    // graph launch -- has one rowbias row per tile), the residual
    E2V_REQUIRE(!a.gn_scsh || a.gn_silu, E2V_EINVAL, "winograd conv: the fused GroupNorm comes with its SiLU");
    static const WinoInKernel in_kernels[2][2] = {{wino_in_kernel<false>, wino_in_kernel<true>}, {wino4_in_kernel<false>, wino4_in_kernel<true>}};
    static const WinoOutKernel out_kernels[2][3][2] = {
        {{wino_out_kernel<0, false>, wino_out_kernel<0, true>}, {wino_out_kernel<1, false>, wino_out_kernel<1, true>},
         {wino_out_kernel<2, false>, wino_out_kernel<2, true>}},
        {{wino4_out_kernel<0, false>, wino4_out_kernel<0, true>}, {wino4_out_kernel<1, false>, wino4_out_kernel<1, true>},
         {wino4_out_kernel<2, false>, wino4_out_kernel<2, true>}}};
    const int rb_form = !a.rowbias ? 0 : a.rows_per_sample % (a.Ho * a.Wo) == 0 ? 1 : 2;
    const WinoInKernel in_kernel = in_kernels[a.m == 4][a.gn_scsh != nullptr];
    const WinoOutKernel out_kernel = out_kernels[a.m == 4][rb_form][a.resid != nullptr];
    for (int lo = 0; lo < a.nimg; lo += chunk_images) {
        const int n = a.nimg - lo < chunk_images ? a.nimg - lo : chunk_images;
        const size_t T = wino_tiles(a, n);
        float* V = ws;
        float* Mb = ws + (size_t)P * T * Ctot;
        {
            const size_t total = T * (Ctot / 4);
            const double px = (double)a.m * a.m;                  // output pixels per tile
            std::string nm = a.gn_scsh ? "wino_in_gn_silu" : "wino_in";
            if (prof_detail())
                nm += " T" + std::to_string(T) + " C" + std::to_string(Ctot) + " m" + std::to_string(a.m) + (a.c1 ? " cat" : "") + (a.upsample ? " up" : "");
            ProfScope ps(nm.c_str(), 2.0 * P * T * Ctot, 4.0 * ((px + P) * T * Ctot), s);
            const int blocks = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
            E2V_KLAUNCH(in_kernel, dim3(blocks), dim3(256), 0, s, a, lo, n, V);
        }
        IgemmArgs g;
        g.a0 = V; g.c0 = Ctot; g.lda0 = Ctot; g.w = a.U; g.ldw = Ctot; g.ldw16 = Ctot;
        g.out = Mb; g.ldc = a.N; g.M = (int)T; g.N = a.N; g.taps = 1;
        g.batch = P; g.sa0 = (long long)T * Ctot; g.sw = (long long)a.N * Ctot; g.sout = (long long)T * a.N;
        if (a.U3) { g.x3 = 1; g.w3 = a.U3; g.w3_plane = (long long)P * a.N * Ctot; }
        igemm(g, s);
        {
            const size_t total = T * (a.N / 4);
            const double px = (double)a.m * a.m;
            std::string nm = "wino_out";
            if (prof_detail())
                nm += " T" + std::to_string(T) + " N" + std::to_string(a.N) + " m" + std::to_string(a.m) + (a.resid ? " res" : "") + (a.rowbias ? " temb" : "");
            ProfScope ps(nm.c_str(), 1.5 * P * T * a.N, 4.0 * (P * T * a.N + px * T * a.N * (a.resid ? 2 : 1)), s);
            const int blocks = (int)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
            E2V_KLAUNCH(out_kernel, dim3(blocks), dim3(256), 0, s, a, lo, n, Mb);
        }
    }
}

}  // namespace e2v
