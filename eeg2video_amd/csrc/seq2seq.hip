// Kernels of the Seq2Seq latent model (the reference's myTransformer, EEG2Video_New/Seq2Seq/my_autoregressive_transformer.py:16-192,
// behind e2v_seq2seq_latents) that the rest of the library has no counterpart for: the EEGNet embedding of one EEG window, attention
// over the handful of tokens the model ever holds, and the latent layout.  LayerNorm and the linears are norm.hip's and igemm.hip's;
// positions, the mean over the window rows and the appended rows are token_embed, token_mean and copy_rows.  fp32 in every compute mode.
#include <cmath>

#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------------
// MyEEGNet_embedding up to the flatten (:16-84), eval mode, of one window per workgroup:
//   block 1  ZeroPad2d(31, 32), conv 1 -> F1 (1 x 64), BN1
//   block 2  grouped conv F1 -> F1 D (C x 1, groups F1), BN2, ELU, AvgPool(1, 4)
//   block 3  ZeroPad2d(7, 8), depthwise F1 D (1 x 16), pointwise F1 D -> F2, BN3, ELU, AvgPool(1, 8)
// The temporal conv, BN1 and the spatial conv are linear, so the FD = F1 D spatial mixes z[o][t] = sum_c w2[o][c] x[c][t] are taken
// FIRST (FD C T multiplies instead of F1 C T 64) and the 64 taps run over z; BN1's shift then is b1[f] sum_c w2[o][c] at every t.
// The three BNs arrive folded (eegnet_pack): block 2 is  a2[o] (taps over z) + c2[o],  block 3  a3[g] (pointwise) + c3[g].
//
// Phases, a barrier between each; every value is the work of ONE thread that sums in index order (c, tap, channel ascending), so a
// window's features do not depend on the grid:
//   0  the pack -> LDS; the window -> xs[C][T], through the optional scaler (x - mean) / scale, 4-byte loads (a window of a raw
//      segment starts 200 bytes into a row); the zero borders of zp and pp
//   1  zp[o][31 + t] = sum_c w2[o][c] xs[c][t]
//   2  pp[o][7 + u]  = mean over t = 4u .. 4u + 3 of ELU(a2[o] sum_k w1[o / D][k] zp[o][t + k] + c2[o])        (u < T / 4)
//   3  dw[o][u]      = sum_k w3[o][k] pp[o][u + k]
//   4  qe[g][u]      = ELU(a3[g] sum_o w4[g][o] dw[o][u] + c3[g])
//   5  out[g (T/32) + v] = mean over u = 8v .. 8v + 7 of qe[g][u]                                               (v < (T / 4) / 8)
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }

__global__ __launch_bounds__(256) void eegnet_embed_kernel(EegnetArgs p) {
    extern __shared__ __attribute__((aligned(16))) char eegnet_smem[];
    const EegnetLayout L = eegnet_layout(p.C, p.T, p.F1, p.D, p.F2);
    float* const sm = reinterpret_cast<float*>(eegnet_smem);
    float* const pk = sm + L.pack;
    float* const xs = sm + L.xs;
    float* const zp = sm + L.zp;
    float* const pp = sm + L.pp;
    float* const dw = sm + L.dw;
    float* const qe = sm + L.qe;
    const int C = p.C, T = p.T, D = p.D, F2 = p.F2, FD = p.F1 * p.D;
    const int T4 = T / 4, T32 = T4 / 8, ldz = T + 63, ldp = T4 + 15;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.W, w = blockIdx.x - b * p.W;

    // ---- phase 0 ----
    for (int i = tid; i < L.pack_floats; i += 256) pk[i] = p.pack[i];
    {
        const float* src = p.eeg + (long long)b * p.clip_stride + (long long)w * p.window_stride;
        const float* mean = p.mean ? p.mean + (size_t)w * C * T : nullptr;
        const float* scale = p.scale ? p.scale + (size_t)w * C * T : nullptr;
        for (int i = tid; i < C * T; i += 256) {
            const int c = i / T, t = i - c * T;
            float v = src[(long long)c * p.channel_stride + t];
            if (mean) v = (v - mean[i]) / scale[i];
            xs[i] = v;
        }
    }
    for (int i = tid; i < FD * 63; i += 256) {
        const int o = i / 63, j = i - o * 63;
        zp[o * ldz + (j < 31 ? j : T + j)] = 0.f;
    }
    for (int i = tid; i < FD * 15; i += 256) {
        const int o = i / 15, j = i - o * 15;
        pp[o * ldp + (j < 7 ? j : T4 + j)] = 0.f;
    }
    __syncthreads();
    const float* const w1 = pk + L.w1;
    const float* const w2 = pk + L.w2;
    const float* const a2 = pk + L.a2;
    const float* const c2 = pk + L.c2;
    const float* const w3 = pk + L.w3;
    const float* const w4 = pk + L.w4;
    const float* const a3 = pk + L.a3;
    const float* const c3 = pk + L.c3;

    // ---- phase 1 ----
    for (int i = tid; i < FD * T; i += 256) {
        const int o = i / T, t = i - o * T;
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(w2[o * C + c], xs[c * T + t], acc);
        zp[o * ldz + 31 + t] = acc;
    }
    __syncthreads();

    // ---- phase 2 ----
    for (int i = tid; i < FD * T4; i += 256) {
        const int o = i / T4, u = i - o * T4;
        const float* wt = w1 + (o / D) * 64;
        const float* z = zp + o * ldz + 4 * u;
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
        for (int k = 0; k < 64; ++k) {
            const float wk = wt[k];
            acc0 = fmaf(wk, z[k], acc0);
            acc1 = fmaf(wk, z[k + 1], acc1);
            acc2 = fmaf(wk, z[k + 2], acc2);
            acc3 = fmaf(wk, z[k + 3], acc3);
        }
        const float sa = a2[o], sc = c2[o];
        const float e = ((elu1(fmaf(acc0, sa, sc)) + elu1(fmaf(acc1, sa, sc))) + elu1(fmaf(acc2, sa, sc))) + elu1(fmaf(acc3, sa, sc));
        pp[o * ldp + 7 + u] = e * 0.25f;
    }
    __syncthreads();

    // ---- phase 3 ----
    for (int i = tid; i < FD * T4; i += 256) {
        const int o = i / T4, u = i - o * T4;
        float acc = 0.f;
        for (int k = 0; k < 16; ++k) acc = fmaf(w3[o * 16 + k], pp[o * ldp + u + k], acc);
        dw[i] = acc;
    }
    __syncthreads();

    // ---- phase 4 ----
    for (int i = tid; i < F2 * T4; i += 256) {
        const int g = i / T4, u = i - g * T4;
        float acc = 0.f;
        for (int o = 0; o < FD; ++o) acc = fmaf(w4[g * FD + o], dw[o * T4 + u], acc);
        qe[i] = elu1(fmaf(acc, a3[g], c3[g]));
    }
    __syncthreads();

    // ---- phase 5 ----
    float* const out = p.out + (size_t)blockIdx.x * F2 * T32;
    for (int i = tid; i < F2 * T32; i += 256) {
        const int g = i / T32, v = i - g * T32;
        const float* q = qe + g * T4 + 8 * v;
        float acc = 0.f;
        for (int k = 0; k < 8; ++k) acc += q[k];
        out[i] = acc * 0.125f;
    }
}

// the pack as the kernel reads it, from the torch-layout tensors of the state dict (host arithmetic, folded in double, one rounding)
std::vector<float> eegnet_pack(const EegnetHostW& h, int C, int F1, int D, int F2, float bn_eps) {
    const EegnetLayout L = eegnet_layout(C, 4, F1, D, F2);      // (the pack's offsets do not depend on T)
    const int FD = F1 * D;
    std::vector<float> pk((size_t)L.pack_floats, 0.f);
    auto fold = [&](const float* bn, int n, int i, double& scale, double& shift) {      // bn: weight | bias | running_mean | running_var
        scale = (double)bn[i] / std::sqrt((double)bn[3 * n + i] + (double)bn_eps);
        shift = (double)bn[n + i] - (double)bn[2 * n + i] * scale;
    };
    for (int i = 0; i < F1 * 64; ++i) pk[L.w1 + i] = h.w1[i];
    for (int i = 0; i < FD * C; ++i) pk[L.w2 + i] = h.w2[i];
    for (int i = 0; i < FD * 16; ++i) pk[L.w3 + i] = h.w3[i];
    for (int i = 0; i < F2 * FD; ++i) pk[L.w4 + i] = h.w4[i];
    for (int o = 0; o < FD; ++o) {
        double s1, b1, s2, b2, wsum = 0.0;
        fold(h.bn1, F1, o / D, s1, b1);
        fold(h.bn2, FD, o, s2, b2);
        for (int c = 0; c < C; ++c) wsum += (double)h.w2[o * C + c];
        pk[L.a2 + o] = (float)(s2 * s1);
        pk[L.c2 + o] = (float)(s2 * b1 * wsum + b2);
    }
    for (int g = 0; g < F2; ++g) {
        double s3, b3;
        fold(h.bn3, F2, g, s3, b3);
        pk[L.a3 + g] = (float)s3;
        pk[L.c3 + g] = (float)b3;
    }
    return pk;
}

void eegnet_embed(const EegnetArgs& a, hipStream_t s) {
    E2V_REQUIRE(a.B >= 1 && a.W >= 1 && a.C >= 1 && a.F1 >= 1 && a.D >= 1 && a.F2 >= 1 && a.T >= 32, E2V_ESHAPE,
                "EEGNet embedding: positive sizes, at least 32 samples a window (the two pools leave T / 32 columns)");
    E2V_REQUIRE((long long)a.B * a.W <= 0x7FFFFFFFLL, E2V_ESHAPE, "EEGNet embedding: B * windows must stay below 2^31");
    const EegnetLayout L = eegnet_layout(a.C, a.T, a.F1, a.D, a.F2);
    E2V_REQUIRE(L.total_floats * sizeof(float) <= (size_t)kEegnetMaxLdsBytes, E2V_ESHAPE,
                "EEGNet embedding: one window with its intermediates needs " + std::to_string(L.total_floats * sizeof(float)) +
                    " bytes of LDS, the kernel has " + std::to_string(kEegnetMaxLdsBytes));
    E2V_REQUIRE((a.mean == nullptr) == (a.scale == nullptr), E2V_EINVAL, "EEGNet embedding: the scaler is a mean AND a scale, or neither");
    const size_t smem = L.total_floats * sizeof(float);
    const double win = (double)a.B * a.W;
    std::string pname = "eegnet_embed";
    if (prof_detail()) pname += " B" + std::to_string(a.B) + " W" + std::to_string(a.W) + " C" + std::to_string(a.C) + " T" + std::to_string(a.T);
    ProfScope ps(pname.c_str(), 2.0 * win * a.F1 * a.D * ((double)a.C * a.T + 64.0 * a.T), 4.0 * win * a.C * a.T, s);
    E2V_KATTR(eegnet_embed_kernel, kEegnetMaxLdsBytes);
    E2V_KLAUNCH(eegnet_embed_kernel, dim3((unsigned)(a.B * a.W)), dim3(256), smem, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// softmax(q k^T scale) v over at most 32 keys: one wave per (clip, head, query).  Lane j holds the score of key j -- q . k_j over d
// ascending, 16 bytes of the key row at a time; the query comes from the same address in every lane --, a key past the query's
// absolute position (causal) takes no part.  The maximum is a butterfly over the wave; the sum of the exponentials and the output
// (lane d, and d + 64 for head dims past 64: sum_j p_j v_j[d]) run over the keys in order, so a query's result depends on its own
// keys alone.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void seq_attn_kernel(SeqAttnArgs p) {
    const int lane = threadIdx.x;
    const int qi = blockIdx.x % p.Nq;
    const int bh = blockIdx.x / p.Nq;
    const int b = bh / p.heads, h = bh - b * p.heads;
    const int D = p.D;
    int nk = p.Nk;
    if (p.causal) { const int vis = p.q_pos0 + qi + 1; nk = vis < nk ? vis : nk; }
    const float* q = p.q + (long long)b * p.sq + (long long)qi * p.ldq + h * D;
    const float* kb = p.k + (long long)b * p.skv + h * D;
    const float* vb = p.v + (long long)b * p.skv + h * D;
    float sc = -INFINITY;
    if (lane < nk) {
        const float* kr = kb + (long long)lane * p.ldkv;
        float acc = 0.f;
        for (int d = 0; d < D; d += 4) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + d);
            const f32x4 qv = *reinterpret_cast<const f32x4*>(q + d);
            acc = fmaf(qv.x, kv.x, acc);
            acc = fmaf(qv.y, kv.y, acc);
            acc = fmaf(qv.z, kv.z, acc);
            acc = fmaf(qv.w, kv.w, acc);
        }
        sc = acc * p.scale;
    }
    float m = sc;
    for (int x = 32; x >= 1; x >>= 1) m = fmaxf(m, __shfl_xor(m, x, 64));
    const float pj = lane < nk ? expf(sc - m) : 0.f;
    float l = 0.f, o0 = 0.f, o1 = 0.f;
    const bool on0 = lane < D, on1 = lane + 64 < D;
    for (int j = 0; j < nk; ++j) {
        const float pv = __shfl(pj, j, 64);
        l += pv;
        const float* vr = vb + (long long)j * p.ldkv;
        if (on0) o0 = fmaf(pv, vr[lane], o0);
        if (on1) o1 = fmaf(pv, vr[lane + 64], o1);
    }
    float* o = p.o + (long long)b * p.so + (long long)qi * p.ldo + h * D;
    if (on0) o[lane] = o0 / l;
    if (on1) o[lane + 64] = o1 / l;
}

void seq_attention(const SeqAttnArgs& a, hipStream_t s) {
    E2V_REQUIRE(a.B >= 1 && a.heads >= 1 && a.Nq >= 1 && a.Nk >= 1 && a.Nk <= kSeqAttnMaxKeys && a.q_pos0 >= 0, E2V_ESHAPE,
                "sequence attention: positive sizes and at most " + std::to_string(kSeqAttnMaxKeys) + " keys (one per lane of half a wave)");
    E2V_REQUIRE(a.D >= 4 && a.D % 4 == 0 && a.D <= 128, E2V_ESHAPE, "sequence attention: the head dim is a multiple of 4 up to 128");
    E2V_REQUIRE(a.ldq % 4 == 0 && a.ldkv % 4 == 0 && a.sq % 4 == 0 && a.skv % 4 == 0 && ((reinterpret_cast<uintptr_t>(a.q) | reinterpret_cast<uintptr_t>(a.k)) & 15) == 0,
                E2V_ESHAPE, "sequence attention: q and k rows are read 16 bytes at a time (strides multiples of 4, 16-byte aligned)");
    E2V_REQUIRE((long long)a.B * a.heads * a.Nq <= 0x7FFFFFFFLL, E2V_ESHAPE, "sequence attention: B * heads * Nq must stay below 2^31");
    const double pairs = (double)a.B * a.heads * a.Nq * a.Nk;
    std::string pname = "seq_attn";
    if (prof_detail()) pname += " B" + std::to_string(a.B) + " h" + std::to_string(a.heads) + " D" + std::to_string(a.D) + " Nq" + std::to_string(a.Nq) + " Nk" + std::to_string(a.Nk);
    ProfScope ps(pname.c_str(), 4.0 * a.D * pairs, 4.0 * a.D * (double)a.B * a.heads * (2.0 * a.Nq + 2.0 * a.Nk), s);
    E2V_KLAUNCH(seq_attn_kernel, dim3((unsigned)(a.B * a.heads * a.Nq)), dim3(64), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// latents [B][F][C][HW] (the predictor's rows) -> [B][C][F][HW] (what the pipeline and e2v_generate take); HW a multiple of 4
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seq_latents_bcfhw_kernel(const float* __restrict__ in, float* __restrict__ out, int F, int C, int HW4,
                                                                size_t quads) {
    const f32x4* src = reinterpret_cast<const f32x4*>(in);
    f32x4* dst = reinterpret_cast<f32x4*>(out);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < quads; i += (size_t)gridDim.x * blockDim.x) {
        const size_t x = i % HW4, r = i / HW4;
        const size_t f = r % F, r2 = r / F;
        const size_t c = r2 % C, b = r2 / C;
        dst[i] = src[((b * F + f) * C + c) * HW4 + x];
    }
}

void seq_latents_bcfhw(const float* in, float* out, int B, int F, int C, int HW, hipStream_t s) {
    E2V_REQUIRE(HW % 4 == 0 && B >= 1 && F >= 1 && C >= 1, E2V_ESHAPE, "latent layout: h * w is a multiple of 4");
    const size_t quads = (size_t)B * F * C * (HW / 4);
    const size_t blocks = (quads + 255) / 256;
    ProfScope ps("seq_latents_bcfhw", 0.0, 32.0 * quads, s);
    E2V_KLAUNCH(seq_latents_bcfhw_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, s, in, out, F, C, HW / 4, quads);
}

}  // namespace e2v
