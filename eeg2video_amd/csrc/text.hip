// Kernels of the CLIP text encoder (transformers CLIPTextModel: the pre-LN text transformer behind e2v_text_encode) that the
// rest of the library has no counterpart for: the embedding gather, causal self-attention over one prompt and the MLP's
// activation.  LayerNorm and the linears are norm.hip's and igemm.hip's.  fp32 in every compute mode; the activation pass also comes
// on 16-bit storage, for the metric towers in 16-bit mode (e2v_set_tower_dtype).
#include <cmath>

#include "act_io.h"
#include "h16.h"
#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// x[b, t, :] = token_table[id[b, t]] + position_table[t]: one wave per row, 16 bytes per lane and step
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void text_embed_kernel(const int* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, float* __restrict__ out, int rows, int T, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const f32x4* a = reinterpret_cast<const f32x4*>(tok + (size_t)ids[row] * C);
    const f32x4* p = reinterpret_cast<const f32x4*>(pos + (size_t)(row % T) * C);
    f32x4* o = reinterpret_cast<f32x4*>(out + (size_t)row * C);
    for (int c = lane; c < C / 4; c += 64) o[c] = a[c] + p[c];
}

void text_embed(const int* ids, const float* tok, const float* pos, float* out, int rows, int T, int C, hipStream_t s) {
    ProfScope ps("text_embed", (double)rows * C, 12.0 * rows * C, s);
    E2V_KLAUNCH(text_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, ids, tok, pos, out, rows, T, C);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Causal self-attention over one prompt (CLIPAttention with the triu mask, head dim 64): one workgroup per (prompt, head).
// K and V of the head are staged in LDS once ([T][68] fp32 each: act_io.h, with the wave ops, shared with the image classifier's
// kernel in vit.hip, which is this one without the triangle).  A wave takes the queries i = w, w + 8, ...; for query i
//   scores   lane j (and j + 64) holds s_j = q_i . k_j for j <= i -- the query's 64 values are read lane by lane into scalar
//            registers, the key row comes from LDS 16 bytes at a time; keys past i are never read (no -inf is added);
//   softmax  fp32, the maximum over the wave subtracted, butterfly reductions over the 64 lanes;
//   output   lane d accumulates sum_j p_j v_j[d] over j = 0 .. i in order (p_j read from its lane), divided by the sum at the end.
// Nothing of a query depends on a later row of the prompt, and the summation order of a row does not depend on T or B.
// ---------------------------------------------------------------------------------------------------------------------------
// s = q . K[j] for this lane's key row (qv: the query, one value per lane).  Called by all 64 lanes: a lane without a key of
// its own is given row i again (a row the query may read) and its score is dropped by the caller.
__device__ __forceinline__ float text_score(const float* __restrict__ krow, float qv) {
    float acc = 0.f;
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
        const f32x4 k = *reinterpret_cast<const f32x4*>(krow + d);
        acc = fmaf(lane_value(qv, d), k.x, acc);
        acc = fmaf(lane_value(qv, d + 1), k.y, acc);
        acc = fmaf(lane_value(qv, d + 2), k.z, acc);
        acc = fmaf(lane_value(qv, d + 3), k.w, acc);
    }
    return acc * 0.125f;                                                           // 64^-0.5
}

__global__ __launch_bounds__(64 * kKeyWaves) void text_causal_attn_kernel(const float* __restrict__ qkv, int ldqkv, float* __restrict__ out,
                                                                           int ldo, int T, int heads) {
    extern __shared__ __attribute__((aligned(16))) char text_smem[];
    float* Ks = reinterpret_cast<float*>(text_smem);
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
    for (int i = w; i < T; i += kKeyWaves) {
        const float qv = base[(size_t)i * ldqkv + lane];
        const bool on0 = lane <= i, on1 = lane + 64 <= i;
        float s0 = text_score(Ks + (on0 ? lane : i) * kKeyLd, qv), s1 = 0.f;
        if (i >= 64) s1 = text_score(Ks + (on1 ? lane + 64 : i) * kKeyLd, qv);     // (wave-uniform: every lane is in)
        const float m = wave_max(fmaxf(on0 ? s0 : -INFINITY, on1 ? s1 : -INFINITY));
        const float p0 = on0 ? expf(s0 - m) : 0.f, p1 = on1 ? expf(s1 - m) : 0.f;
        const float l = wave_sum(p0 + p1);
        float acc = 0.f;
        const int n0 = i < 63 ? i + 1 : 64;
        for (int j = 0; j < n0; ++j) acc = fmaf(lane_value(p0, j), Vs[j * kKeyLd + lane], acc);
        for (int j = 64; j <= i; ++j) acc = fmaf(lane_value(p1, j - 64), Vs[j * kKeyLd + lane], acc);
        out[((size_t)b * T + i) * ldo + h * 64 + lane] = acc / l;
    }
}

void text_causal_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s) {
    E2V_REQUIRE(T >= 1 && T <= kTextAttnMaxT, E2V_ESHAPE, "causal attention: 1 <= T <= " + std::to_string(kTextAttnMaxT));
    const size_t smem = (size_t)2 * T * kKeyLd * sizeof(float);
    const double pairs = (double)B * heads * T * (T + 1) / 2;                  // (query, key) pairs of the causal triangle
    std::string pname = "text_causal_attn";
    if (prof_detail()) pname += " B" + std::to_string(B) + " T" + std::to_string(T) + " h" + std::to_string(heads);
    ProfScope ps(pname.c_str(), 4.0 * 64 * pairs, 4.0 * 4.0 * 64 * B * heads * T, s);
    E2V_KATTR(text_causal_attn_kernel, (size_t)2 * kTextAttnMaxT * kKeyLd * sizeof(float));
    E2V_KLAUNCH(text_causal_attn_kernel, dim3(B * heads), dim3(64 * kKeyWaves), smem, s, qkv, ldqkv, out, ldo, T, heads);
}

// ---------------------------------------------------------------------------------------------------------------------------
// the MLP's activation, in place on the fc1 output: quick-GELU h sigmoid(1.702 h) (SD-v1-4's text tower) or the erf GELU
// ---------------------------------------------------------------------------------------------------------------------------
template <int ACT>
__device__ __forceinline__ float text_act(float h) {
    if (ACT == 0) return h / (1.0f + expf(-1.702f * h));
    return 0.5f * h * (1.0f + erff(h * 0.70710678118654752f));
}

template <int ACT>
__global__ __launch_bounds__(256) void text_activation_kernel(float* __restrict__ x, size_t quads) {
    f32x4* p = reinterpret_cast<f32x4*>(x);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < quads; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 v = p[i];
        v.x = text_act<ACT>(v.x); v.y = text_act<ACT>(v.y); v.z = text_act<ACT>(v.z); v.w = text_act<ACT>(v.w);
        p[i] = v;
    }
}

// the same on 16-bit storage (a tower in 16-bit mode): eight elements per 16-byte access, widened exactly, the activation in fp32,
// rounded once at the store
template <int ACT, typename H>
__global__ __launch_bounds__(256) void text_activation_h16_kernel(H* __restrict__ x, size_t octets) {
    using V = RowVec<H, 8>;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < octets; i += (size_t)gridDim.x * blockDim.x) {
        V v = V::load(x + 8 * i);
        v.apply([](float h) { return text_act<ACT>(h); });
        v.store(x + 8 * i);
    }
}

void text_activation(float* x, long long count, int act, hipStream_t s, int h16) {
    const int per = h16 ? 8 : 4;                // elements per 16-byte access
    E2V_REQUIRE(count % per == 0 && (act == 0 || act == 1), E2V_EINVAL, "text activation: whole 16-byte pieces, quick_gelu (0) or gelu (1)");
    if (count <= 0) return;
    const size_t pieces = (size_t)count / per;
    const size_t blocks = (pieces + 255) / 256;
    const int grid = (int)(blocks < 8192 ? blocks : 8192);
    ProfScope ps(act == 0 ? "text_quick_gelu" : "text_gelu", 8.0 * count, (h16 ? 4.0 : 8.0) * count, s);
    if (!h16) {
        if (act == 0) E2V_KLAUNCH(text_activation_kernel<0>, dim3(grid), dim3(256), 0, s, x, pieces);
        else E2V_KLAUNCH(text_activation_kernel<1>, dim3(grid), dim3(256), 0, s, x, pieces);
        return;
    }
    h16_dispatch(h16, [&](auto tag) {
        using H = decltype(tag);
        H* xh = reinterpret_cast<H*>(x);
        if (act == 0) E2V_KLAUNCH((text_activation_h16_kernel<0, H>), dim3(grid), dim3(256), 0, s, xh, pieces);
        else E2V_KLAUNCH((text_activation_h16_kernel<1, H>), dim3(grid), dim3(256), 0, s, xh, pieces);
    });
}

}  // namespace e2v
