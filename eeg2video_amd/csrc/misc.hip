// Element-wise and layout kernels of the path (all HBM-bound, grid-stride, 16-byte lanes where the
// layout allows): boundary layout conversion NCFHW <-> channel-last, the fused classifier-free
// guidance + DDIM update, the timestep sinusoid, SiLU, and a tiled transpose for the VAE attention.
#include <type_traits>

#include "h16.h"
#include "kernels.h"
#include "prof.h"
#include "act_io.h"
#include "runtime.h"

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline int grid_for(size_t total, int cap = 8192) {
    size_t b = (total + 255) / 256;
    return (int)(b < (size_t)cap ? (b ? b : 1) : cap);
}

// in [n][C][FHW] -> out [n][FHW][Cpad] (extra channels zero), times `scale`
template <typename T>
__global__ void ncfhw_to_cl_kernel(const float* __restrict__ in, T* __restrict__ out, int n, int C, int Cpad, int FHW,
                                   float scale) {
    const size_t total = (size_t)n * FHW * Cpad;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = i % Cpad;
        const size_t r = i / Cpad;
        const int p = r % FHW;
        const int b = r / FHW;
        out[i] = (T)(c < C ? in[((size_t)b * C + c) * FHW + p] * scale : 0.f);
    }
}
void ncfhw_to_cl(const float* in, float* out, int n, int C, int Cpad, int FHW, float scale, hipStream_t s, int out_bf16) {
    const size_t total = (size_t)n * FHW * Cpad;
    if (out_bf16)
        h16_dispatch(out_bf16, [&](auto h16_tag) {
            using H = decltype(h16_tag);
            E2V_KLAUNCH(ncfhw_to_cl_kernel<H>, dim3(grid_for(total)), dim3(256), 0, s, in, reinterpret_cast<H*>(out), n, C, Cpad, FHW, scale);
        });
    else
        E2V_KLAUNCH(ncfhw_to_cl_kernel<float>, dim3(grid_for(total)), dim3(256), 0, s, in, out, n, C, Cpad, FHW, scale);
}

// in [n][FHW][ld] (first C channels) -> out [n][C][FHW]; y = x*mul + add, optional clamp to [0,1]
__global__ void cl_to_ncfhw_kernel(const float* __restrict__ in, int ld, float* __restrict__ out, int n, int C, int FHW,
                                   float mul, float add, int clamp, float lo, float hi) {
    const size_t total = (size_t)n * C * FHW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = i % FHW;
        const size_t r = i / FHW;
        const int c = r % C;
        const int b = r / C;
        float v = in[((size_t)b * FHW + p) * ld + c] * mul + add;
        if (clamp) v = fminf(fmaxf(v, lo), hi);
        out[i] = v;
    }
}
void cl_to_ncfhw(const float* in, int ld, float* out, int n, int C, int FHW, float mul, float add, int clamp, float lo,
                 float hi, hipStream_t s) {
    const size_t total = (size_t)n * C * FHW;
    E2V_KLAUNCH(cl_to_ncfhw_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, ld, out, n, C, FHW, mul, add, clamp, lo,
                       hi);
}

// frames decoded as (b f) images, channel-last [n*F][HW][ld] -> video [n][C][F][HW]
// ('(b f) c h w -> b c f h w' of pipeline_tuneeeg2video.py:180, then (v/2+0.5).clamp(0,1) of :181)
__global__ void frames_to_ncfhw_kernel(const float* __restrict__ in, int ld, float* __restrict__ out, int n, int F, int C,
                                       int HW, float mul, float add, int clamp01) {
    const size_t total = (size_t)n * C * F * HW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = i % HW;
        size_t r = i / HW;
        const int f = r % F; r /= F;
        const int c = r % C;
        const int b = r / C;
        float v = in[(((size_t)b * F + f) * HW + p) * ld + c] * mul + add;
        if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
        out[i] = v;
    }
}
void nchw_frames_to_ncfhw(const float* in, int ld, float* out, int n, int F, int C, int HW, float mul, float add, int clamp01,
                          hipStream_t s) {
    const size_t total = (size_t)n * C * F * HW;
    E2V_KLAUNCH(frames_to_ncfhw_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, ld, out, n, F, C, HW, mul, add,
                       clamp01);
}

// diffusers get_timestep_embedding: w_i = exp(-ln(10000) i / (half - shift)),
// emb = [sin(t w), cos(t w)], swapped to [cos, sin] when flip_sin_to_cos.  t has nt entries (1 = broadcast).
template <typename TT>
__global__ void timestep_sinusoid_kernel(const TT* __restrict__ t, int nt, float* __restrict__ out, int n, int dim,
                                         int flip, float shift) {
    const int half = dim / 2;
    const int total = n * half;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int b = i / half, k = i - b * half;
        const float tv = (float)t[nt == 1 ? 0 : b];
        const float expo = (-9.210340371976184f * (float)k) / ((float)half - shift);
        const float arg = tv * expf(expo);
        const float sv = sinf(arg), cv = cosf(arg);
        float* o = out + (size_t)b * dim;
        if (flip) { o[k] = cv; o[half + k] = sv; } else { o[k] = sv; o[half + k] = cv; }
    }
}
void timestep_sinusoid(const long long* t, int nt, float* out, int n, int dim, int flip, float shift, hipStream_t s, int t_is_f32) {
    if (t_is_f32)       // fractional timesteps of the sigma-space schedulers (Euler, LMS): the fp32 value the reference's .float() makes
        E2V_KLAUNCH(timestep_sinusoid_kernel<float>, dim3(grid_for((size_t)n * dim / 2)), dim3(256), 0, s,
                           reinterpret_cast<const float*>(t), nt, out, n, dim, flip, shift);
    else
        E2V_KLAUNCH(timestep_sinusoid_kernel<long long>, dim3(grid_for((size_t)n * dim / 2)), dim3(256), 0, s, t, nt, out, n, dim,
                           flip, shift);
}

__global__ void silu_kernel(const float* __restrict__ in, float* __restrict__ out, size_t count) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const float v = in[i];
        out[i] = v / (1.0f + expf(-v));
    }
}
void silu(const float* in, float* out, long long count, hipStream_t s) {
    if (count <= 0) return;
    E2V_KLAUNCH(silu_kernel, dim3(grid_for((size_t)count)), dim3(256), 0, s, in, out, (size_t)count);
}

// out[b][c][r] = in[b][r][c], 32x32 LDS tiles
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* __restrict__ in, int ld_in, T* __restrict__ out,
                                                        int ld_out, int rows, int cols, long long sb_in, long long sb_out) {
    __shared__ T tile[32][33];
    const T* src = in + (size_t)blockIdx.z * sb_in;
    T* dst = out + (size_t)blockIdx.z * sb_out;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        tile[k][tx] = (r < rows && c < cols) ? src[(size_t)r * ld_in + c] : (T)0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (c < cols && r < rows) dst[(size_t)c * ld_out + r] = tile[tx][k];
    }
}
void transpose2d(const float* in, int ld_in, float* out, int ld_out, int rows, int cols, int batch, long long sb_in,
                 long long sb_out, hipStream_t s, int bf16) {
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch);
    if (bf16)            // (a 2-byte payload: one instance serves bf16 and fp16)
        E2V_KLAUNCH(transpose_kernel<unsigned short>, grid, dim3(256), 0, s, reinterpret_cast<const unsigned short*>(in), ld_in,
                           reinterpret_cast<unsigned short*>(out), ld_out, rows, cols, sb_in, sb_out);
    else
        E2V_KLAUNCH(transpose_kernel<float>, grid, dim3(256), 0, s, in, ld_in, out, ld_out, rows, cols, sb_in, sb_out);
}

// pipeline_tuneeeg2video.py:320-325 fused: guidance, then DDIM (eta = 0):
//   x0 = (x - sqrt(1-a_t) eps) / sqrt(a_t);  x' = sqrt(a_p) x0 + sqrt(1-a_p) eps
// eps_c == nullptr: no guidance (guidance_scale <= 1), eps = eps_u.
__global__ void ddim_cfg_step_kernel(const float* __restrict__ eu, const float* __restrict__ ec, const float* __restrict__ x,
                                     float* __restrict__ xo, size_t count, float g, float sa, float sb, float sap, float sbp) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        float e = eu[i];
        if (ec) e = e + g * (ec[i] - e);
        const float x0 = (x[i] - sb * e) / sa;
        xo[i] = sap * x0 + sbp * e;
    }
}
void ddim_cfg_step(const float* eps_u, const float* eps_c, const float* x, float* x_out, long long count, float guidance,
                   float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_p, float sqrt_1m_a_p, hipStream_t s) {
    if (count <= 0) return;
    ProfScope ps("ddim_cfg_step", 8.0 * count, 4.0 * count * (eps_c ? 4.0 : 3.0), s);
    E2V_KLAUNCH(ddim_cfg_step_kernel, dim3(grid_for((size_t)count)), dim3(256), 0, s, eps_u, eps_c, x, x_out,
                       (size_t)count, guidance, sqrt_a_t, sqrt_1m_a_t, sqrt_a_p, sqrt_1m_a_p);
}

// out = sum_i c_i x_i over up to five tensors (the linear multistep combinations of PNDM/PLMS and its sample update);
// cfg (ec != nullptr): out = eu + g (ec - eu), the guidance line of the pipeline (pipeline_tuneeeg2video.py:320-322)
struct LinComb { const float* x[5]; float c[5]; int n; };
__global__ void lincomb_kernel(const LinComb a, float* __restrict__ out, size_t count) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        float v = a.c[0] * a.x[0][i];
#pragma unroll
        for (int k = 1; k < 5; ++k)
            if (k < a.n) v += a.c[k] * a.x[k][i];
        out[i] = v;
    }
}
void lincomb(int n, const float* const* xs, const float* coefs, float* out, long long count, hipStream_t s) {
    if (count <= 0) return;
    LinComb a{};
    a.n = n;
    for (int k = 0; k < n; ++k) { a.x[k] = xs[k]; a.c[k] = coefs[k]; }
    ProfScope ps("lincomb", 2.0 * n * count, 4.0 * count * (n + 1), s);
    E2V_KLAUNCH(lincomb_kernel, dim3(grid_for((size_t)count)), dim3(256), 0, s, a, out, (size_t)count);
}
__global__ void cfg_combine_kernel(const float* __restrict__ eu, const float* __restrict__ ec, float g, float* __restrict__ out,
                                   size_t count) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x) {
        const float e = eu[i];
        out[i] = e + g * (ec[i] - e);
    }
}
void cfg_combine(const float* eu, const float* ec, float g, float* out, long long count, hipStream_t s) {
    if (count <= 0) return;
    ProfScope ps("cfg_combine", 3.0 * count, 12.0 * count, s);
    E2V_KLAUNCH(cfg_combine_kernel, dim3(grid_for((size_t)count)), dim3(256), 0, s, eu, ec, g, out, (size_t)count);
}

// ---- SURVEY 8(f) rows ---------------------------------------------------------------------------------------
__global__ void dana_kernel(const float* __restrict__ x0, const float* __restrict__ ed, const float* __restrict__ es,
                            const float* __restrict__ coef, float s1b, float sb, float* __restrict__ out, int B, int F, int C,
                            int HW) {
    const size_t total = (size_t)B * C * F * HW;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = i % HW;
        size_t r = i / HW;
        const int f = r % F; r /= F;
        const int c = r % C;
        const int b = r / C;
        const size_t src = (((size_t)b * F + f) * C + c) * HW + p;          // [B,F,C,HW]
        const size_t same = ((size_t)b * C + c) * HW + p;                   // [B,1,C,HW]
        const float noise = ed[src] * s1b + es[same] * sb;                  // DANA_module.py:60-61
        out[i] = coef[2 * b] * x0[src] + coef[2 * b + 1] * noise;           // :71-72
    }
}
void dana_noise(const float* x0, const float* eps_div, const float* eps_same, const float* coef, float sqrt_1m_beta,
                float sqrt_beta, float* out, int B, int F, int C, int HW, hipStream_t s) {
    const size_t total = (size_t)B * C * F * HW;
    if (!total) return;
    ProfScope ps("dana_noise", 6.0 * total, 4.0 * total * 3.2, s);
    E2V_KLAUNCH(dana_kernel, dim3(grid_for(total)), dim3(256), 0, s, x0, eps_div, eps_same, coef, sqrt_1m_beta, sqrt_beta,
                       out, B, F, C, HW);
}

__global__ void frames_to_u8_kernel(const float* __restrict__ in, unsigned char* __restrict__ out, size_t count) {
    const size_t n4 = count / 4;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(in + 4 * i);
        uchar4 o;
        o.x = (unsigned char)(v[0] * 255.f); o.y = (unsigned char)(v[1] * 255.f);
        o.z = (unsigned char)(v[2] * 255.f); o.w = (unsigned char)(v[3] * 255.f);
        *reinterpret_cast<uchar4*>(out + 4 * i) = o;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (size_t i = n4 * 4; i < count; ++i) out[i] = (unsigned char)(in[i] * 255.f);
}
void frames_to_u8(const float* in, unsigned char* out, long long count, hipStream_t s) {
    if (count <= 0) return;
    ProfScope ps("frames_to_u8", 1.0 * count, 5.0 * count, s);
    E2V_KLAUNCH(frames_to_u8_kernel, dim3(grid_for((size_t)count / 4 + 1)), dim3(256), 0, s, in, out, (size_t)count);
}

template <typename T>
__global__ void pad_cols_kernel(const float* __restrict__ in, int cols, T* __restrict__ out, int cp, size_t rows) {
    const size_t total = rows * cp;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = i % cp;
        const size_t r = i / cp;
        out[i] = (T)(c < cols ? in[r * cols + c] : 0.f);
    }
}
void pad_cols(const float* in, int cols, float* out, int cols_pad, long long rows, hipStream_t s, int out_bf16) {
    if (rows <= 0) return;
    if (out_bf16)
        h16_dispatch(out_bf16, [&](auto h16_tag) {
            using H = decltype(h16_tag);
            E2V_KLAUNCH(pad_cols_kernel<H>, dim3(grid_for((size_t)rows * cols_pad)), dim3(256), 0, s, in, cols, reinterpret_cast<H*>(out), cols_pad, (size_t)rows);
        });
    else
        E2V_KLAUNCH(pad_cols_kernel<float>, dim3(grid_for((size_t)rows * cols_pad)), dim3(256), 0, s, in, cols, out, cols_pad, (size_t)rows);
}

// ---- in-place weight update (e2v_update_tensor; kernels.h: WeightScatterArgs) --------------------------------------------------
// One lane per 8-column piece of a source row: the piece is read ONCE (16-byte loads) and written to every live form of the linear --
// fp32 (two 16-byte stores), bf16 / fp16 (one each) and the three truncation planes of the f32x3 mode (one each).  The conversions are
// the ones finalize() uses: the compiler's round-to-nearest-even casts of to_h16_kernel and the subtraction chain of
// split_bf16x3_kernel, so an updated matrix has the bits a fresh finalize would give it.  VEC = false serves what 16-byte accesses
// cannot: a row length that is no multiple of 8 (22, 310: the Semantic Predictor's first layer, 4: the VAE's latent convs) or a source
// that is not 16-byte aligned -- element loads guarded by the row length (nothing is read past the source), element stores for the
// fp32 and plane rows; the 16-bit rows are padded to a multiple of 8 and always take whole pieces.
template <typename Src, bool VEC>
__global__ __launch_bounds__(256) void weight_scatter_kernel(const WeightScatterArgs a, int pieces) {
    const Src* __restrict__ src = static_cast<const Src*>(a.src);
    const size_t total = (size_t)a.rows * pieces;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % pieces);
        const int r = (int)(i / pieces);
        const int c0 = p * 8;
        float v[8];
        if constexpr (VEC) {
            const Src* sp = src + (size_t)r * a.in + c0;
            if constexpr (sizeof(Src) == 4) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(sp), hi = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) { v[k] = lo[k]; v[4 + k] = hi[k]; }
            } else {
                const hx8<Src> q = *reinterpret_cast<const hx8<Src>*>(sp);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (float)q[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = c0 + k < a.in ? (float)src[(size_t)r * a.in + c0 + k] : 0.f;
        }
        int dr = r;
        if (a.half > 0) {
            const int jj = r % a.half;
            dr = 2 * a.blk * (jj / a.blk) + jj % a.blk + (r >= a.half ? a.blk : 0);
        }
        dr += a.row_off;
        if (a.d32) {
            float* d = a.d32 + (size_t)dr * a.ld32 + c0;
            if constexpr (VEC) {
                *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) if (c0 + k < a.ld32) d[k] = v[k];
            }
        }
        if (c0 < a.ld16) {              // (ld16 is a multiple of 8: a piece is inside the row or past it)
            if (a.d16b) {
                hx8<__bf16> o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = (__bf16)v[k];
                *reinterpret_cast<hx8<__bf16>*>(static_cast<__bf16*>(a.d16b) + (size_t)dr * a.ld16 + c0) = o;
            }
            if (a.d16h) {
                hx8<_Float16> o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = (_Float16)v[k];
                *reinterpret_cast<hx8<_Float16>*>(static_cast<_Float16*>(a.d16h) + (size_t)dr * a.ld16 + c0) = o;
            }
        }
        if (a.d3) {                     // x = p0 + p1 + p2 exactly (split_bf16x3_kernel)
            hx8<unsigned short> p0, p1, p2;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float x = v[k];
                const unsigned b1 = __builtin_bit_cast(unsigned, x) & 0xFFFF0000u;
                const float r1 = x - __builtin_bit_cast(float, b1);
                const unsigned b2 = __builtin_bit_cast(unsigned, r1) & 0xFFFF0000u;
                const float r2 = r1 - __builtin_bit_cast(float, b2);
                p0[k] = (unsigned short)(b1 >> 16);
                p1[k] = (unsigned short)(b2 >> 16);
                p2[k] = (unsigned short)(__builtin_bit_cast(unsigned, r2) >> 16);
            }
            unsigned short* d = static_cast<unsigned short*>(a.d3) + (size_t)dr * a.ld3 + c0;
            if constexpr (VEC) {
                *reinterpret_cast<hx8<unsigned short>*>(d) = p0;
                *reinterpret_cast<hx8<unsigned short>*>(d + a.plane) = p1;
                *reinterpret_cast<hx8<unsigned short>*>(d + 2 * a.plane) = p2;
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (c0 + k < a.ld3) { d[k] = p0[k]; d[a.plane + k] = p1[k]; d[2 * a.plane + k] = p2[k]; }
            }
        }
    }
}
void weight_scatter(const WeightScatterArgs& a, hipStream_t s) {
    if (a.rows <= 0 || a.in <= 0) return;
    const bool any16 = a.d16b || a.d16h;
    E2V_REQUIRE(a.src && (!a.d32 || a.ld32 >= a.in) && (!any16 || (a.ld16 >= a.in && a.ld16 % 8 == 0)) && (!a.d3 || a.ld3 >= a.in) &&
                    a.blk > 0 && (a.half == 0 || (a.rows == 2 * a.half && a.half % a.blk == 0)),
                E2V_EINVAL, "weight_scatter: bad destination geometry");
    int cols = a.in;
    if (a.d32) cols = cols > a.ld32 ? cols : a.ld32;
    if (any16) cols = cols > a.ld16 ? cols : a.ld16;
    if (a.d3) cols = cols > a.ld3 ? cols : a.ld3;
    const int pieces = (cols + 7) / 8;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    // 16-byte accesses everywhere: whole pieces in the source and in every destination row, every row start aligned
    const bool vec = a.in % 8 == 0 && al16(a.src) &&
                     (!a.d32 || (a.ld32 == a.in && al16(a.d32 + (size_t)a.row_off * a.ld32))) &&
                     (!a.d3 || (a.ld3 == a.in && a.plane % 8 == 0 && al16(a.d3))) && (!any16 || (al16(a.d16b) && al16(a.d16h)));
    const size_t total = (size_t)a.rows * pieces;
    const dim3 g(grid_for(total)), b(256);
    auto launch = [&](auto src_tag) {
        using Src = decltype(src_tag);
        if (vec) E2V_KLAUNCH((weight_scatter_kernel<Src, true>), g, b, 0, s, a, pieces);
        else E2V_KLAUNCH((weight_scatter_kernel<Src, false>), g, b, 0, s, a, pieces);
    };
    if (a.src_mode == H16_NONE) launch(float{});
    else h16_dispatch(a.src_mode, launch);
}

// ---- weight read-back (e2v_read_tensor; kernels.h: WeightGatherArgs) -----------------------------------------------------------------
// The inverse of weight_scatter_kernel over the same row map: one lane per 8-column piece of a DESTINATION row, read from the one
// stored form the caller chose (Src = float, __bf16, _Float16; X3: unsigned short planes, summed (p0 + p1) + p2 -- the partial sums
// fit fp32's 24 bits, so the value is the fp32 weight the planes were split from) and written dense in the requested type (the compiler's
// round-to-nearest-even casts, as to_h16_kernel).  VEC: 16-byte loads and stores.  VEC = false serves a row length that is no multiple
// of 8 (22, 310, 4) and a source row or a destination that is not 16-byte aligned: element loads guarded by `in` (the padding columns
// of a source row are never read), element stores guarded by `in` (rows * in elements are written, no more).
template <typename Src, typename Dst, bool X3, bool VEC>
__global__ __launch_bounds__(256) void weight_gather_kernel(const WeightGatherArgs a, int pieces) {
    const Src* __restrict__ src = static_cast<const Src*>(a.src);
    Dst* __restrict__ dst = static_cast<Dst*>(a.dst);
    const size_t total = (size_t)a.rows * pieces;
    auto plane_val = [](unsigned short p0, unsigned short p1, unsigned short p2) {
        const float f0 = __builtin_bit_cast(float, (unsigned)p0 << 16), f1 = __builtin_bit_cast(float, (unsigned)p1 << 16),
                    f2 = __builtin_bit_cast(float, (unsigned)p2 << 16);
        return (f0 + f1) + f2;
    };
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % pieces);
        const int r = (int)(i / pieces);
        const int c0 = p * 8;
        int sr = r;
        if (a.half > 0) {
            const int jj = r % a.half;
            sr = 2 * a.blk * (jj / a.blk) + jj % a.blk + (r >= a.half ? a.blk : 0);
        }
        sr += a.row_off;
        const Src* sp = src + (size_t)sr * a.ld + c0;
        float v[8];
        if constexpr (VEC) {
            if constexpr (X3) {
                const hx8<unsigned short> p0 = *reinterpret_cast<const hx8<unsigned short>*>(sp),
                                          p1 = *reinterpret_cast<const hx8<unsigned short>*>(sp + a.plane),
                                          p2 = *reinterpret_cast<const hx8<unsigned short>*>(sp + 2 * a.plane);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = plane_val(p0[k], p1[k], p2[k]);
            } else if constexpr (sizeof(Src) == 4) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(sp), hi = *reinterpret_cast<const f32x4*>(sp + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) { v[k] = lo[k]; v[4 + k] = hi[k]; }
            } else {
                const hx8<Src> q = *reinterpret_cast<const hx8<Src>*>(sp);
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = (float)q[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                v[k] = 0.f;
                if (c0 + k < a.in) {
                    if constexpr (X3) v[k] = plane_val(sp[k], sp[a.plane + k], sp[2 * a.plane + k]);
                    else v[k] = (float)sp[k];
                }
            }
        }
        Dst* d = dst + (size_t)r * a.in + c0;
        if constexpr (VEC) {
            if constexpr (sizeof(Dst) == 4) {
                *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<f32x4*>(d + 4) = f32x4{v[4], v[5], v[6], v[7]};
            } else {
                hx8<Dst> o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = (Dst)v[k];
                *reinterpret_cast<hx8<Dst>*>(d) = o;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) if (c0 + k < a.in) d[k] = (Dst)v[k];
        }
    }
}
void weight_gather(const WeightGatherArgs& a, hipStream_t s) {
    if (a.rows <= 0 || a.in <= 0) return;
    E2V_REQUIRE(a.src && a.dst && a.ld >= a.in && a.row_off >= 0 && a.blk > 0 && (a.half == 0 || (a.rows == 2 * a.half && a.half % a.blk == 0)) &&
                    (!a.x3 || a.plane >= (long long)(a.row_off + a.rows) * a.ld),
                E2V_EINVAL, "weight_gather: bad source geometry");
    const int pieces = (a.in + 7) / 8;
    const size_t esz = a.x3 || a.src_mode != H16_NONE ? 2 : 4;
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    // 16-byte accesses: whole pieces, every source row start (of every plane) and the destination aligned
    const bool vec = a.in % 8 == 0 && ((size_t)a.ld * esz) % 16 == 0 && al16(static_cast<const char*>(a.src) + (size_t)a.row_off * a.ld * esz) &&
                     (!a.x3 || a.plane % 8 == 0) && al16(a.dst);
    const size_t total = (size_t)a.rows * pieces;
    const dim3 g(grid_for(total)), b(256);
    auto launch = [&](auto src_tag, auto dst_tag, auto x3_tag) {
        using Src = decltype(src_tag);
        using Dst = decltype(dst_tag);
        constexpr bool X3 = decltype(x3_tag)::value;
        if (vec) E2V_KLAUNCH((weight_gather_kernel<Src, Dst, X3, true>), g, b, 0, s, a, pieces);
        else E2V_KLAUNCH((weight_gather_kernel<Src, Dst, X3, false>), g, b, 0, s, a, pieces);
    };
    auto with_dst = [&](auto src_tag, auto x3_tag) {
        if (a.dst_mode == H16_NONE) launch(src_tag, float{}, x3_tag);
        else h16_dispatch(a.dst_mode, [&](auto dst_tag) { launch(src_tag, dst_tag, x3_tag); });
    };
    if (a.x3) with_dst((unsigned short)0, std::true_type{});
    else if (a.src_mode == H16_NONE) with_dst(float{}, std::false_type{});
    else h16_dispatch(a.src_mode, [&](auto src_tag) { with_dst(src_tag, std::false_type{}); });
}

// strided row copy with a storage-type change: out[r][c] = in[r][c] for c < cols, 0 for cols <= c < cols_out
template <typename TI, typename TO>
__global__ void cvt_rows_kernel(const TI* __restrict__ in, int ld_in, TO* __restrict__ out, int ld_out, size_t rows, int cols, int cols_out) {
    const size_t total = rows * cols_out;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = i % cols_out;
        const size_t r = i / cols_out;
        out[r * ld_out + c] = c < cols ? (TO)(float)in[r * ld_in + c] : (TO)0.f;
    }
}
void cvt_rows(const void* in, int ld_in, int in_bf16, void* out, int ld_out, int out_bf16, long long rows, int cols, int cols_out,
              hipStream_t s) {
    if (rows <= 0 || cols_out <= 0) return;
    const dim3 g(grid_for((size_t)rows * cols_out)), b(256);
    if (in_bf16 || out_bf16) {           // (both 16-bit: the same type -- a run has one 16-bit mode)
        h16_dispatch(in_bf16 ? in_bf16 : out_bf16, [&](auto h16_tag) {
            using H = decltype(h16_tag);
            if (in_bf16 && out_bf16)
                E2V_KLAUNCH((cvt_rows_kernel<H, H>), g, b, 0, s, static_cast<const H*>(in), ld_in, static_cast<H*>(out), ld_out, (size_t)rows, cols, cols_out);
            else if (in_bf16)
                E2V_KLAUNCH((cvt_rows_kernel<H, float>), g, b, 0, s, static_cast<const H*>(in), ld_in, static_cast<float*>(out), ld_out, (size_t)rows, cols, cols_out);
            else
                E2V_KLAUNCH((cvt_rows_kernel<float, H>), g, b, 0, s, static_cast<const float*>(in), ld_in, static_cast<H*>(out), ld_out, (size_t)rows, cols, cols_out);
        });
    }
    else
        E2V_KLAUNCH((cvt_rows_kernel<float, float>), g, b, 0, s, static_cast<const float*>(in), ld_in, static_cast<float*>(out), ld_out, (size_t)rows, cols, cols_out);
}

// E2V_POOL_GUARD (runtime.h): compare the two guard zones of one block with the pattern, in 16-bit units (a 16-bit tensor may end on
// a 2-byte boundary).  One workgroup; each thread keeps the first altered unit of its stride, thread 0 folds the 256 candidates and
// writes the slot -- plain loads and stores, nothing shared between launches.
__global__ __launch_bounds__(256) void pool_guard_check_kernel(const unsigned short* __restrict__ lead, const unsigned short* __restrict__ trail,
                                                               unsigned units, unsigned* __restrict__ slot) {
    __shared__ unsigned first[2][256];
    for (int z = 0; z < 2; ++z) {
        const unsigned short* p = z ? trail : lead;
        unsigned f = 0xFFFFFFFFu;
        for (unsigned i = threadIdx.x; i < units; i += 256)
            if (p[i] != (unsigned short)(kGuardPattern & 0xFFFFu) && f == 0xFFFFFFFFu) f = i;
        first[z][threadIdx.x] = f;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int z = 0; z < 2; ++z) {
            unsigned f = 0xFFFFFFFFu;
            for (int t = 0; t < 256; ++t) f = first[z][t] < f ? first[z][t] : f;
            slot[z] = f;
        }
}
void pool_guard_check(const void* lead, const void* trail, size_t guard_bytes, uint32_t* slot, hipStream_t s) {
    E2V_KLAUNCH(pool_guard_check_kernel, dim3(1), dim3(256), 0, s, static_cast<const unsigned short*>(lead),
                static_cast<const unsigned short*>(trail), (unsigned)(guard_bytes / 2), slot);
    const hipError_t e = hipGetLastError();                  // (e.g. a stream the caller has destroyed since)
    if (e != hipSuccess) throw Error(E2V_EHIP, std::string("pool_guard_check: ") + hipGetErrorString(e));
}

}  // namespace e2v
