// Kernels of the ViT image classifier (transformers ViTForImageClassification behind e2v_image_classify: the classifier half of
// img_classify_metric, EEG2Video/40_class_run_metrics.py:86-98) that the rest of the library has no counterpart for: the tables
// of Pillow's antialiased resize, non-causal self-attention over the tokens of one image, and the softmax / top-3 head.  LayerNorm,
// the linears and the erf GELU are norm.hip's, igemm.hip's and text.hip's; the preprocess and the token rows are video.hip's.  fp32
// whatever the context's compute mode.
#include <algorithm>
#include <cmath>

#include "act_io.h"
#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// Pillow's Image.resize(BILINEAR / BICUBIC) (src/libImaging/Resample.c, ImagingResampleInner for 8-bit images): per axis a table of
// normalised filter weights in double (precompute_coeffs), rounded to 22-bit fixed point (normalize_coeffs_8bpc); the
// horizontal pass runs first and its result is rounded to bytes before the vertical pass reads it -- except for an image more than
// 100 times as tall as it is wide that is being shrunk vertically, which Image.resize (PIL/Image.py) resizes vertically first.
// The filters are Resample.c's bilinear_filter (support 1) and bicubic_filter (a = -0.5, support 2); the bicubic one has negative
// lobes, so coefficients may be negative and a sum may leave [0, 255]: the kernels' arithmetic >> 22 and clip8 are Pillow's.
// The 22 bits leave the 32-bit accumulator room: it starts at 2^21 and the positive (negative) coefficients of an output add at most
// 255 times their sum; both bounds are checked here for every output, so no table that would overflow reaches a kernel.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

double bicubic_filter(double x) {                                               // Resample.c: `#define a -0.5`
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

}  // namespace

ResizeAxis resize_axis(int in_size, int out_size, int filter) {
    E2V_REQUIRE(filter == kResizeBilinear || filter == kResizeBicubic, E2V_EINVAL, "resize filter: 2 (bilinear) or 3 (bicubic), Pillow's codes");
    const bool cubic = filter == kResizeBicubic;
    ResizeAxis t;
    t.in = in_size; t.out = out_size;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = (cubic ? 2.0 : 1.0) * filterscale;
    t.ksize = (int)std::ceil(support) * 2 + 1;
    t.first.assign(out_size, 0);
    t.count.assign(out_size, 0);
    t.coeff.assign((size_t)out_size * t.ksize, 0);
    std::vector<double> k(t.ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            const double arg = (x + xmin - center + 0.5) * ss;
            const double w = cubic ? bicubic_filter(arg) : bilinear_filter(arg);
            k[x] = w;
            ww += w;
        }
        long long pos = 0, neg = 0;
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const int q = k[x] < 0 ? (int)(-0.5 + k[x] * (1 << 22)) : (int)(0.5 + k[x] * (1 << 22));
            t.coeff[(size_t)xx * t.ksize + x] = q;
            (q < 0 ? neg : pos) += q;
        }
        E2V_REQUIRE((1LL << 21) + 255 * pos <= 2147483647LL && (1LL << 21) + 255 * neg >= -2147483648LL, E2V_ESHAPE,
                    "resize table: an output's coefficients could overflow the 32-bit accumulator");
        t.first[xx] = xmin;
        t.count[xx] = xmax;
    }
    return t;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Non-causal self-attention over the tokens of one image (ViTSelfAttention, head dim 64): the text encoder's kernel (text.hip)
// without the triangle and with up to NR = ceil(T / 64) keys per lane.  One workgroup per (image, head); K and V of the head are
// staged in LDS once ([T][68] fp32 each; the stride, the workgroup's 8 waves and the wave ops are act_io.h's, shared with that
// kernel).  A wave takes the queries i = w, w + 8, ...; for query i
//   scores   lane j holds s_{j + 64 r} = q_i . k_{j + 64 r}, r < NR: the query's 64 values are read lane by lane into scalar
//            registers, d ascending, one fma chain per key; a lane without a key in block r reads row T - 1 and drops the score;
//   softmax  fp32, the maximum over the wave subtracted, the lane's exponentials added r ascending, then butterfly reductions;
//   output   lane d accumulates sum_j p_j v_j[d] over j = 0 .. T - 1 in order (p_j read from its lane), divided by the sum at the end.
// The summation order of a row depends on T alone -- not on the batch, the head count or the position of the image in the call.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

template <int NR>
__global__ __launch_bounds__(64 * kKeyWaves) void image_attn_kernel(const float* __restrict__ qkv, int ldqkv, float* __restrict__ out, int ldo,
                                                                    int T, int heads) {
    extern __shared__ __attribute__((aligned(16))) char img_smem[];
    float* Ks = reinterpret_cast<float*>(img_smem);
    float* Vs = Ks + (size_t)T * kKeyLd;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int C = heads * 64;
    const float* base = qkv + (size_t)b * T * ldqkv + h * 64;
    for (int i = threadIdx.x; i < T * 16; i += 64 * kKeyWaves) {
        const int r = i >> 4, c = (i & 15) * 4;
        const float* src = base + (size_t)r * ldqkv + c;
        *reinterpret_cast<f32x4*>(Ks + r * kKeyLd + c) = *reinterpret_cast<const f32x4*>(src + C);
        *reinterpret_cast<f32x4*>(Vs + r * kKeyLd + c) = *reinterpret_cast<const f32x4*>(src + 2 * C);
    }
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    bool on[NR];
    const float* krow[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        on[r] = lane + 64 * r < T;
        krow[r] = Ks + (on[r] ? lane + 64 * r : T - 1) * kKeyLd;
    }
    for (int i = w; i < T; i += kKeyWaves) {
        const float qv = base[(size_t)i * ldqkv + lane];
        float sc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) sc[r] = 0.f;
#pragma unroll 4
        for (int d = 0; d < 64; d += 4) {
            const float q0 = lane_value(qv, d), q1 = lane_value(qv, d + 1), q2 = lane_value(qv, d + 2), q3 = lane_value(qv, d + 3);
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const f32x4 k = *reinterpret_cast<const f32x4*>(krow[r] + d);
                sc[r] = fmaf(q0, k.x, sc[r]);
                sc[r] = fmaf(q1, k.y, sc[r]);
                sc[r] = fmaf(q2, k.z, sc[r]);
                sc[r] = fmaf(q3, k.w, sc[r]);
            }
        }
        float m = -INFINITY;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            sc[r] *= 0.125f;                                                       // 64^-0.5
            m = fmaxf(m, on[r] ? sc[r] : -INFINITY);
        }
        m = wave_max(m);
        float l = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            sc[r] = on[r] ? expf(sc[r] - m) : 0.f;
            l += sc[r];
        }
        l = wave_sum(l);
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int nj = min(64, T - 64 * r);                                    // (>= 1: NR = ceil(T / 64))
            const float* vcol = Vs + (size_t)64 * r * kKeyLd + lane;
            for (int j = 0; j < nj; ++j) acc = fmaf(lane_value(sc[r], j), vcol[j * kKeyLd], acc);
        }
        out[((size_t)b * T + i) * ldo + h * 64 + lane] = acc / l;
    }
}

template <int NR>
void image_attn_launch(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, size_t smem, hipStream_t s) {
    E2V_KATTR(image_attn_kernel<NR>, (size_t)2 * kImageAttnMaxT * kKeyLd * sizeof(float));
    E2V_KLAUNCH(image_attn_kernel<NR>, dim3(B * heads), dim3(64 * kKeyWaves), smem, s, qkv, ldqkv, out, ldo, T, heads);
}

}  // namespace

void image_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s) {
    E2V_REQUIRE(T >= 1 && T <= kImageAttnMaxT, E2V_ESHAPE, "image attention: 1 <= T <= " + std::to_string(kImageAttnMaxT));
    E2V_REQUIRE(B >= 1 && heads >= 1, E2V_ESHAPE, "image attention: B, heads >= 1");
    const size_t smem = (size_t)2 * T * kKeyLd * sizeof(float);
    const double pairs = (double)B * heads * T * T;
    std::string pname = "image_attn";
    if (prof_detail()) pname += " B" + std::to_string(B) + " T" + std::to_string(T) + " h" + std::to_string(heads);
    ProfScope ps(pname.c_str(), 4.0 * 64 * pairs, 4.0 * 4.0 * 64 * B * heads * T, s);
    switch ((T + 63) / 64) {
        case 1: image_attn_launch<1>(qkv, ldqkv, out, ldo, B, T, heads, smem, s); break;
        case 2: image_attn_launch<2>(qkv, ldqkv, out, ldo, B, T, heads, smem, s); break;
        case 3: image_attn_launch<3>(qkv, ldqkv, out, ldo, B, T, heads, smem, s); break;
        case 4: image_attn_launch<4>(qkv, ldqkv, out, ldo, B, T, heads, smem, s); break;
        default: image_attn_launch<5>(qkv, ldqkv, out, ldo, B, T, heads, smem, s); break;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The head after the classifier linear: one wave per image.  softmax in fp32 (the lane's strided terms added in index order, then
// a butterfly); top 3 by the key (value, index) -- equal logits rank as a stable ascending argsort ranks them, the larger index
// last -- written in ascending order: logits.argsort(-1)[-3:] (40_class_run_metrics.py:97).
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ unsigned long long head_key(float v, int j) {
    unsigned u = __builtin_bit_cast(unsigned, v + 0.f);                            // (-0 -> +0: they compare equal in a sort)
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);                                // order of the floats as unsigned integers
    return ((unsigned long long)u << 32) | (unsigned)(j + 1);                      // 0 is "none"
}

__device__ __forceinline__ unsigned long long head_wave_max(unsigned long long k) {
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)k, m, 64), hi = (unsigned)__shfl_xor((int)(unsigned)(k >> 32), m, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

__global__ __launch_bounds__(64) void image_head_kernel(const float* __restrict__ logits, int ld, int L, float* __restrict__ logits_out,
                                                        float* __restrict__ probs, int* __restrict__ top3) {
    const int lane = threadIdx.x;
    const float* x = logits + (size_t)blockIdx.x * ld;
    if (logits_out)
        for (int j = lane; j < L; j += 64) logits_out[(size_t)blockIdx.x * L + j] = x[j];
    if (probs) {
        float m = -INFINITY;
        for (int j = lane; j < L; j += 64) m = fmaxf(m, x[j]);
        m = wave_max(m);
        float l = 0.f;
        for (int j = lane; j < L; j += 64) l += expf(x[j] - m);
        l = wave_sum(l);
        for (int j = lane; j < L; j += 64) probs[(size_t)blockIdx.x * L + j] = expf(x[j] - m) / l;
    }
    if (top3) {
        unsigned long long k0 = 0, k1 = 0, k2 = 0;                                 // the lane's three largest keys, k0 >= k1 >= k2
        for (int j = lane; j < L; j += 64) {
            const unsigned long long k = head_key(x[j], j);
            if (k > k0) { k2 = k1; k1 = k0; k0 = k; }
            else if (k > k1) { k2 = k1; k1 = k; }
            else if (k > k2) k2 = k;
        }
        for (int r = 0; r < 3; ++r) {                                              // L >= 3: every round finds a key (keys are distinct)
            const unsigned long long best = head_wave_max(k0);
            if (k0 == best) { k0 = k1; k1 = k2; k2 = 0; }
            if (lane == 0) top3[(size_t)blockIdx.x * 3 + (2 - r)] = (int)(unsigned)(best & 0xFFFFFFFFu) - 1;
        }
    }
}

}  // namespace

void image_head(const float* logits, int ld, int L, int nimg, float* logits_out, float* probs, int* top3, hipStream_t s) {
    ProfScope ps("image_head", 8.0 * nimg * L, 12.0 * nimg * L, s);
    E2V_KLAUNCH(image_head_kernel, dim3(nimg), dim3(64), 0, s, logits, ld, L, logits_out, probs, top3);
}

}  // namespace e2v
