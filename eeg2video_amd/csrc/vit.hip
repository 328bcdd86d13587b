// Kernels of the ViT image classifier (transformers ViTForImageClassification behind e2v_image_classify: the classifier half of
// img_classify_metric, EEG2Video/40_class_run_metrics.py:86-98) that the rest of the library has no counterpart for: the image
// processor (Pillow's antialiased resize fused with the pixel table and the patch layout), the assembly of the token rows,
// non-causal self-attention over the tokens of one image, and the softmax / top-3 head.  LayerNorm, the linears and the erf GELU
// are norm.hip's, igemm.hip's and text.hip's.  fp32 by default whatever the context's compute mode; the preprocess and the
// token rows also come over 16-bit rows for a tower in 16-bit mode (e2v_set_tower_dtype).
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "act_io.h"
#include "h16.h"
#include "image_prep.h"
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

// The band of output rows a workgroup of the preprocess kernel takes: the horizontally resized source rows the band reads stay in
// LDS as bytes ([rows][S]).  One patch row (P output rows) where that fits, else the largest band that does; 0: not even one row.
ImagePrepPlan image_prep_plan(int H, int W, int S, int P, const float* lut768) {
    ImagePrepPlan p;
    p.H = H; p.W = W; p.S = S;
    const ResizeAxis h = resize_axis(W, S), v = resize_axis(H, S);
    p.kh = h.ksize; p.kv = v.ksize;
    p.vfirst = (long long)H > 100LL * W && S < H;                                // Image.resize: `self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`
    auto rows_of = [&](int band) {
        int most = 0;
        for (int y0 = 0; y0 < S; y0 += band) {
            const int y1 = std::min(y0 + band, S) - 1;
            int lo = v.first[y0], hi = v.first[y0] + v.count[y0];
            for (int y = y0; y <= y1; ++y) { lo = std::min(lo, v.first[y]); hi = std::max(hi, v.first[y] + v.count[y]); }
            // (the kernel takes the band's source rows as [first of its first row, end of its last row): both ends are monotonic)
            if (lo != v.first[y0] || hi != v.first[y1] + v.count[y1]) return 1 << 30;
            most = std::max(most, hi - lo);
        }
        return most;
    };
    for (int band = std::min(P, S); band >= 1; --band) {                         // (vertical first: the band's rows at the source width)
        const int rows = p.vfirst ? band : rows_of(band);
        if ((long long)rows * (p.vfirst ? W : S) <= kImagePrepLdsBytes) { p.band = band; p.band_rows = rows; break; }
    }
    p.words.reserve((size_t)4 * S + (size_t)S * (p.kh + p.kv) + 768);
    p.words.insert(p.words.end(), h.first.begin(), h.first.end());
    p.words.insert(p.words.end(), h.count.begin(), h.count.end());
    p.words.insert(p.words.end(), v.first.begin(), v.first.end());
    p.words.insert(p.words.end(), v.count.begin(), v.count.end());
    p.words.insert(p.words.end(), h.coeff.begin(), h.coeff.end());
    p.words.insert(p.words.end(), v.coeff.begin(), v.coeff.end());
    for (int i = 0; i < 768; ++i) p.words.push_back(__builtin_bit_cast(int, lut768[i]));
    return p;
}

namespace {

// One workgroup: `band` output rows of one channel of one image.
//   1. horizontal pass over the source rows the band reads -> bytes in LDS ([rows][S]; staging in LDS instead of a byte buffer in
//      the pool: the intermediate of a band is consumed by the workgroup that made it, 5 KB at 288 x 512 -> 224, and never visits HBM);
//   2. vertical pass over those bytes -> byte -> pixel table -> the patch-row matrix.
// Integer arithmetic as Pillow's: 32-bit accumulators starting at 2^21, >> 22, clipped to a byte.
// VFIRST (Pillow's order for very tall images): 1. vertical pass of the band's rows at the source width W -> bytes in LDS ([band][W]);
// 2. horizontal pass over them.
// O: the patch rows' storage type -- fp32, or bf16 / fp16 (a tower in 16-bit mode): the table's fp32 value rounded once, at the store.
template <bool F32, bool VFIRST, typename O>
__global__ __launch_bounds__(256) void image_prep_kernel(PrepView v, int F, long long img0, int W, int S, int P, int kh, int kv, int band,
                                                         const int* __restrict__ plan, O* __restrict__ rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char prep_tmp[];
    const int* hfirst = plan;
    const int* hcount = plan + S;
    const int* vfirst = plan + 2 * S;
    const int* vcount = plan + 3 * S;
    const int* hco = plan + 4 * S;
    const int* vco = hco + (size_t)S * kh;
    const float* lut = reinterpret_cast<const float*>(vco + (size_t)S * kv);
    const int y0 = blockIdx.x * band, y1 = min(y0 + band, S);
    const int c = blockIdx.y;
    const long long gimg = img0 + blockIdx.z;
    const long long clip = gimg / F, f = gimg - clip * F;
    const long long base = clip * v.s_n + f * v.s_img + c * v.s_c;
    const int np = S / P, K = 3 * P * P;
    if (VFIRST) {
        for (int i = threadIdx.x; i < (y1 - y0) * W; i += 256) {
            const int ry = i / W, x = i - ry * W, yy = y0 + ry;
            const long long coloff = base + (long long)x * v.s_x;
            const int first = vfirst[yy], cnt = vcount[yy];
            int acc = 1 << 21;
            for (int k = 0; k < cnt; ++k) acc += vco[yy * kv + k] * prep_load<F32>(v, coloff + (long long)(first + k) * v.s_y);
            prep_tmp[i] = (unsigned char)clip8(acc >> 22);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < (y1 - y0) * S; i += 256) {
            const int ry = i / S, xx = i - ry * S, yy = y0 + ry;
            const int x0 = hfirst[xx], cnt = hcount[xx];
            int acc = 1 << 21;
            for (int k = 0; k < cnt; ++k) acc += hco[xx * kh + k] * (int)prep_tmp[ry * W + x0 + k];
            const int byte = clip8(acc >> 22);
            const int py = yy / P, px = xx / P;
            const size_t row = ((size_t)blockIdx.z * np + py) * np + px;
            rows[row * K + (size_t)c * P * P + (yy - py * P) * P + (xx - px * P)] = (O)lut[c * 256 + byte];
        }
        return;
    }
    const int r0 = vfirst[y0], nr = vfirst[y1 - 1] + vcount[y1 - 1] - r0;
    for (int i = threadIdx.x; i < nr * S; i += 256) {
        const int r = i / S, xx = i - r * S;
        const long long rowoff = base + (long long)(r0 + r) * v.s_y;
        const int x0 = hfirst[xx], cnt = hcount[xx];
        int acc = 1 << 21;
        for (int k = 0; k < cnt; ++k) acc += hco[xx * kh + k] * prep_load<F32>(v, rowoff + (long long)(x0 + k) * v.s_x);
        prep_tmp[i] = (unsigned char)clip8(acc >> 22);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (y1 - y0) * S; i += 256) {
        const int ry = i / S, xx = i - ry * S, yy = y0 + ry;
        const int first = vfirst[yy] - r0, cnt = vcount[yy];
        int acc = 1 << 21;
        for (int k = 0; k < cnt; ++k) acc += vco[yy * kv + k] * (int)prep_tmp[(first + k) * S + xx];
        const int byte = clip8(acc >> 22);
        const int py = yy / P, px = xx / P;
        const size_t row = ((size_t)blockIdx.z * np + py) * np + px;
        rows[row * K + (size_t)c * P * P + (yy - py * P) * P + (xx - px * P)] = (O)lut[c * 256 + byte];
    }
}

}  // namespace

void image_preprocess(const FrameSrc& src, int n, int F, long long img0, int nimg, const ImagePrepPlan& plan, const int* plan_dev, int P,
                      float* rows, hipStream_t s, int h16) {
    const int S = plan.S;
    E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, "image preprocess: the source rows of one output row do not fit the kernel's LDS band");
    E2V_REQUIRE(nimg >= 1 && nimg <= 65535 && img0 >= 0 && img0 + nimg <= (long long)n * F, E2V_EINVAL, "image preprocess: bad image range");
    const long long HW = (long long)plan.H * plan.W;
    PrepView v;
    v.p = src.p;
    if (src.channels_last) { v.s_n = (long long)F * HW * 3; v.s_img = HW * 3; v.s_c = 1; v.s_y = (long long)plan.W * 3; v.s_x = 3; }
    else { v.s_n = 3LL * F * HW; v.s_img = HW; v.s_c = (long long)F * HW; v.s_y = plan.W; v.s_x = 1; }
    const size_t smem = (size_t)plan.band_rows * (plan.vfirst ? plan.W : S);
    const dim3 grid((S + plan.band - 1) / plan.band, 3, nimg);
    ProfScope ps("image_preprocess", 2.0 * nimg * 3 * S * ((double)plan.H * plan.kh + (double)S * plan.kv),
                 (double)nimg * 3 * (HW * (src.f32 ? 4.0 : 1.0) + (h16 ? 2.0 : 4.0) * S * S), s);
    auto launch_as = [&](auto* out) {
        using O = std::remove_pointer_t<decltype(out)>;
        auto launch = [&](auto kernel) {
            E2V_KLAUNCH(kernel, grid, dim3(256), smem, s, v, F, img0, plan.W, S, P, plan.kh, plan.kv, plan.band, plan_dev, out);
        };
        if (plan.vfirst) { if (src.f32) launch(image_prep_kernel<true, true, O>); else launch(image_prep_kernel<false, true, O>); }
        else { if (src.f32) launch(image_prep_kernel<true, false, O>); else launch(image_prep_kernel<false, false, O>); }
    };
    if (!h16) return launch_as(rows);
    h16_dispatch(h16, [&](auto tag) { launch_as(reinterpret_cast<decltype(tag)*>(rows)); });
}

// ---------------------------------------------------------------------------------------------------------------------------
// token rows: x[i][0] = cls + pos[0], x[i][1 + p] = patch row p of image i + pos[1 + p]; one wave per row, 16 bytes per lane and step
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void image_embed_kernel(const float* __restrict__ patches, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, float* __restrict__ out, int rows, int T, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int img = row / T, t = row - img * T;
    const f32x4* a = reinterpret_cast<const f32x4*>(t == 0 ? cls : patches + ((size_t)img * (T - 1) + (t - 1)) * C);
    const f32x4* p = reinterpret_cast<const f32x4*>(pos + (size_t)t * C);
    f32x4* o = reinterpret_cast<f32x4*>(out + (size_t)row * C);
    for (int c = lane; c < C / 4; c += 64) o[c] = a[c] + p[c];
}

// the same over 16-bit patch and token rows (a tower in 16-bit mode): the class row and the positions stay fp32, the sum is fp32 and
// is rounded once at the store
template <typename H>
__global__ __launch_bounds__(256) void image_embed_h16_kernel(const H* __restrict__ patches, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, H* __restrict__ out, int rows, int T, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int img = row / T, t = row - img * T;
    const H* a = patches + ((size_t)img * (T - 1) + (t - 1)) * C;          // (t == 0: not read)
    const float* p = pos + (size_t)t * C;
    H* o = out + (size_t)row * C;
    for (int c = 4 * lane; c < C; c += 256) st4(o + c, (t == 0 ? ld4(cls + c) : ld4(a + c)) + ld4(p + c));
}

void image_embed(const float* patches, const float* cls, const float* pos, float* x, int nimg, int T, int C, hipStream_t s, int h16) {
    const int rows = nimg * T;
    ProfScope ps("image_embed", (double)rows * C, (h16 ? 8.0 : 12.0) * rows * C, s);
    if (!h16) { E2V_KLAUNCH(image_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, patches, cls, pos, x, rows, T, C); return; }
    h16_dispatch(h16, [&](auto tag) {
        using H = decltype(tag);
        E2V_KLAUNCH(image_embed_h16_kernel<H>, dim3((rows + 3) / 4), dim3(256), 0, s, reinterpret_cast<const H*>(patches), cls, pos,
                    reinterpret_cast<H*>(x), rows, T, C);
    });
}

// ---------------------------------------------------------------------------------------------------------------------------
// Non-causal self-attention over the tokens of one image (ViTSelfAttention, head dim 64): the text encoder's kernel (text.hip)
// without the triangle and with up to NR = ceil(T / 64) keys per lane.  One workgroup per (image, head); K and V of the head are
// staged in LDS once ([T][68] fp32 each: the stride that keeps the 16 lanes of a ds_read_b128 group 4 banks apart).  A wave takes
// the queries i = w, w + 8, ...; for query i
//   scores   lane j holds s_{j + 64 r} = q_i . k_{j + 64 r}, r < NR: the query's 64 values are read lane by lane into scalar
//            registers, d ascending, one fma chain per key; a lane without a key in block r reads row T - 1 and drops the score;
//   softmax  fp32, the maximum over the wave subtracted, the lane's exponentials added r ascending, then butterfly reductions;
//   output   lane d accumulates sum_j p_j v_j[d] over j = 0 .. T - 1 in order (p_j read from its lane), divided by the sum at the end.
// The summation order of a row depends on T alone -- not on the batch, the head count or the position of the image in the call.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

constexpr int kImgLd = 68;          // LDS row stride in floats
constexpr int kImgWaves = 8;

__device__ __forceinline__ float img_wave_max(float v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float img_wave_sum(float v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ float img_lane_value(float v, int lane) {      // v of `lane` (wave-uniform) as a scalar
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

template <int NR>
__global__ __launch_bounds__(64 * kImgWaves) void image_attn_kernel(const float* __restrict__ qkv, int ldqkv, float* __restrict__ out, int ldo,
                                                                    int T, int heads) {
    extern __shared__ __attribute__((aligned(16))) char img_smem[];
    float* Ks = reinterpret_cast<float*>(img_smem);
    float* Vs = Ks + (size_t)T * kImgLd;
    const int b = blockIdx.x / heads, h = blockIdx.x - b * heads;
    const int C = heads * 64;
    const float* base = qkv + (size_t)b * T * ldqkv + h * 64;
    for (int i = threadIdx.x; i < T * 16; i += 64 * kImgWaves) {
        const int r = i >> 4, c = (i & 15) * 4;
        const float* src = base + (size_t)r * ldqkv + c;
        *reinterpret_cast<f32x4*>(Ks + r * kImgLd + c) = *reinterpret_cast<const f32x4*>(src + C);
        *reinterpret_cast<f32x4*>(Vs + r * kImgLd + c) = *reinterpret_cast<const f32x4*>(src + 2 * C);
    }
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    bool on[NR];
    const float* krow[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        on[r] = lane + 64 * r < T;
        krow[r] = Ks + (on[r] ? lane + 64 * r : T - 1) * kImgLd;
    }
    for (int i = w; i < T; i += kImgWaves) {
        const float qv = base[(size_t)i * ldqkv + lane];
        float sc[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) sc[r] = 0.f;
#pragma unroll 4
        for (int d = 0; d < 64; d += 4) {
            const float q0 = img_lane_value(qv, d), q1 = img_lane_value(qv, d + 1), q2 = img_lane_value(qv, d + 2), q3 = img_lane_value(qv, d + 3);
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
        m = img_wave_max(m);
        float l = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            sc[r] = on[r] ? expf(sc[r] - m) : 0.f;
            l += sc[r];
        }
        l = img_wave_sum(l);
        float acc = 0.f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int nj = min(64, T - 64 * r);                                    // (>= 1: NR = ceil(T / 64))
            const float* vcol = Vs + (size_t)64 * r * kImgLd + lane;
            for (int j = 0; j < nj; ++j) acc = fmaf(img_lane_value(sc[r], j), vcol[j * kImgLd], acc);
        }
        out[((size_t)b * T + i) * ldo + h * 64 + lane] = acc / l;
    }
}

template <int NR>
void image_attn_launch(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, size_t smem, hipStream_t s) {
    E2V_KATTR(image_attn_kernel<NR>, (size_t)2 * kImageAttnMaxT * kImgLd * sizeof(float));
    E2V_KLAUNCH(image_attn_kernel<NR>, dim3(B * heads), dim3(64 * kImgWaves), smem, s, qkv, ldqkv, out, ldo, T, heads);
}

}  // namespace

void image_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s) {
    E2V_REQUIRE(T >= 1 && T <= kImageAttnMaxT, E2V_ESHAPE, "image attention: 1 <= T <= " + std::to_string(kImageAttnMaxT));
    E2V_REQUIRE(B >= 1 && heads >= 1, E2V_ESHAPE, "image attention: B, heads >= 1");
    const size_t smem = (size_t)2 * T * kImgLd * sizeof(float);
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
        m = img_wave_max(m);
        float l = 0.f;
        for (int j = lane; j < L; j += 64) l += expf(x[j] - m);
        l = img_wave_sum(l);
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
