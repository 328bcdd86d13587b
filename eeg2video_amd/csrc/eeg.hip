// The EEG front end's feature extractor (e2v_eeg_de_psd): the reference's DE_PSD (EEG_preprocessing/DE_PSD.py:8-71) of every
// (clip, window, electrode) row, read where it lies in the raw segment.  fp32 in every compute mode, no atomics; every value is the
// work of one thread that sums in index order, so a row's features depend on the row (and the sampling rate) alone.
#include <cmath>

#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));
static_assert(kShallowGroup == 4, "the ShallowNet kernel reads a group's weights as one 16-byte vector");

// ---------------------------------------------------------------------------------------------------------------------------
// What DE_PSD computes of one row x[0 .. m) (the reference in float64; here fp32 from tables made in double):
//   h[k]   = 0.5 - 0.5 cos(2 pi (k + 1) / (m + 1))            the reference's Hann row of length L = m (every caller passes L = m)
//   X[j]   = sum_{n < min(m, 200)} h[n] x[n] e^{-2 pi i j n / 200}    scipy.fftpack.fft(h x, 200): a row longer than the transform is
//                                                             TRUNCATED to its first 200 windowed samples, a shorter one zero-padded
//   E[p]   = (sum_{j = first[p]}^{last[p]} |X[j]|^2) / (last[p] - first[p] + 1)      first = int(fStart / fs 200) - 1, last =
//                                                             int(fEnd / fs 200) - 1 (range(fStartNum - 1, fEndNum)); the bands overlap
//   psd[p] = E[p],  de[p] = log2(100 E[p])
// One workgroup per row.  Phases, a barrier between each:
//   0  the plan (Hann row, twiddles) and the windowed row -> LDS; the row through 4-byte loads (a window starts anywhere in a segment)
//   1  thread j < bins: X[j] by the direct sum over n ascending, one accumulator each for the real and the imaginary part, the
//      twiddle of (j, n) from the table at (j n) mod 200 (the index is stepped, never multiplied out); |X[j]|^2 -> LDS
//   2  thread p < 5: the band sum over j ascending, the division, log2f, the optional scaler (de - mean) / scale
// A row of zeros gives E = 0: psd 0 and de -inf (the reference raises ValueError in math.log there).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kDePsdThreads) void eeg_de_psd_kernel(DePsdArgs p) {
    __shared__ float xs[kDePsdN];
    __shared__ float2 tw[kDePsdN];
    __shared__ float pw[kDePsdN / 2];
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const int c = row % p.C, bw = row / p.C;
    const int w = bw % p.W, b = bw / p.W;
    const float* src = p.eeg + (long long)b * p.clip_stride + (long long)w * p.window_stride + (long long)c * p.channel_stride;

    // ---- phase 0 ----
    for (int i = tid; i < kDePsdN; i += kDePsdThreads) {
        xs[i] = i < p.n ? src[i] * p.plan[i] : 0.f;
        tw[i] = make_float2(p.plan[kDePsdN + 2 * i], p.plan[kDePsdN + 2 * i + 1]);
    }
    __syncthreads();

    // ---- phase 1 ----
    if (tid < p.bins) {
        float re = 0.f, im = 0.f;
        int idx = 0;
        for (int n = 0; n < p.n; ++n) {
            const float x = xs[n];
            const float2 t = tw[idx];
            re = fmaf(x, t.x, re);
            im = fmaf(x, t.y, im);
            idx += tid;
            if (idx >= kDePsdN) idx -= kDePsdN;
        }
        pw[tid] = fmaf(re, re, im * im);
    }
    __syncthreads();

    // ---- phase 2 ----
    if (tid < kDePsdBands) {
        float e = 0.f;
        for (int j = p.first[tid]; j <= p.last[tid]; ++j) e += pw[j];
        e = e / (float)(p.last[tid] - p.first[tid] + 1);
        const size_t o = (size_t)row * kDePsdBands + tid;
        if (p.psd) p.psd[o] = e;
        if (p.de) {
            float d = log2f(100.f * e);
            if (p.de_mean) d = (d - p.de_mean[c * kDePsdBands + tid]) / p.de_scale[c * kDePsdBands + tid];
            p.de[o] = d;
        }
    }
}

// host arithmetic in double, rounded once: the first min(m, 200) values of the Hann row of length m (zeros behind them), then
// cos | sin (2 pi j / 200) interleaved
std::vector<float> de_psd_plan(int m) {
    std::vector<float> plan((size_t)kDePsdPlanFloats, 0.f);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < std::min(m, kDePsdN); ++k) plan[k] = (float)(0.5 - 0.5 * std::cos(2.0 * pi * (double)(k + 1) / (double)(m + 1)));
    for (int j = 0; j < kDePsdN; ++j) {
        plan[kDePsdN + 2 * j] = (float)std::cos(2.0 * pi * (double)j / (double)kDePsdN);
        plan[kDePsdN + 2 * j + 1] = (float)std::sin(2.0 * pi * (double)j / (double)kDePsdN);
    }
    return plan;
}

// the reference's bin ranges at sampling rate fs, with its own double arithmetic: int(f / fs * 200).  false where the reference would
// index from the end of the spectrum (a first bin below 0) or past its half (a last bin above 99)
bool de_psd_bands(int fs, int* first, int* last) {
    static const int f_start[kDePsdBands] = {1, 4, 8, 14, 31}, f_end[kDePsdBands] = {4, 8, 14, 31, 99};
    if (fs < 1) return false;
    for (int p = 0; p < kDePsdBands; ++p) {
        const int s = (int)((double)f_start[p] / (double)fs * (double)kDePsdN), e = (int)((double)f_end[p] / (double)fs * (double)kDePsdN);
        first[p] = s - 1;
        last[p] = e - 1;
        if (s < 1 || e > kDePsdN / 2 || e < s) return false;
    }
    return true;
}

void eeg_de_psd(const DePsdArgs& a, hipStream_t s) {
    E2V_REQUIRE(a.B >= 1 && a.W >= 1 && a.C >= 1 && a.n >= 1 && a.n <= kDePsdN, E2V_ESHAPE,
                "DE / PSD: positive sizes, at most " + std::to_string(kDePsdN) + " samples enter the transform");
    E2V_REQUIRE((long long)a.B * a.W * a.C <= 0x7FFFFFFFLL, E2V_ESHAPE, "DE / PSD: B * windows * electrodes must stay below 2^31");
    E2V_REQUIRE(a.bins >= 1 && a.bins <= kDePsdN / 2 && a.bins <= kDePsdThreads, E2V_ESHAPE, "DE / PSD: at most 100 bins, the half spectrum");
    for (int p = 0; p < kDePsdBands; ++p)
        E2V_REQUIRE(a.first[p] >= 0 && a.first[p] <= a.last[p] && a.last[p] < a.bins, E2V_ESHAPE, "DE / PSD: a band lies outside the computed bins");
    E2V_REQUIRE((a.de_mean == nullptr) == (a.de_scale == nullptr), E2V_EINVAL, "DE / PSD: the scaler is a mean AND a scale, or neither");
    E2V_REQUIRE(a.eeg && a.plan && (a.de || a.psd), E2V_EINVAL, "DE / PSD: null argument");
    const double rows = (double)a.B * a.W * a.C;
    std::string pname = "eeg_de_psd";
    if (prof_detail()) pname += " B" + std::to_string(a.B) + " W" + std::to_string(a.W) + " C" + std::to_string(a.C) + " n" + std::to_string(a.n);
    ProfScope ps(pname.c_str(), 4.0 * rows * a.bins * a.n, 4.0 * rows * (a.n + 2.0 * kDePsdBands), s);
    E2V_KLAUNCH(eeg_de_psd_kernel, dim3((unsigned)((long long)a.B * a.W * a.C)), dim3(kDePsdThreads), 0, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// shallownet up to the flatten (EEG2Video/models/models.py:105-123), eval mode:
//   Conv2d(1, F, (1, K)) -> Conv2d(F, F, (C, 1)) -> BatchNorm2d (running statistics) -> ELU -> AvgPool2d((1, P), (1, S)) -> flatten
// The two convolutions and the BatchNorm are linear with nothing between them: shallownet_fold makes them ONE filter w [F][C][K] and a
// constant c [F] (F C K multiply-adds per column instead of F K + F F C),
//   y[f][t] = sum_{c, k} w[f][c][k] x[c][t + k] + c[f],   t < Tc = T - K + 1
//   out[f cols + j] = (sum_{i < P} ELU(y[f][S j + i])) / P,   j < cols = (Tc - P) / S + 1          (filter-major: the reference's flatten)
// The folded filter of the global net (40 x 62 x 25: 248 KB) does not fit the LDS beside a clip, and nothing in it is shared between
// output filters: the grid is split BY OUTPUT FILTERS, one workgroup per (clip, group of kShallowGroup filters).  The workgroup stages
// its clip (through the optional scaler) in LDS; the filter is never staged -- every thread of the workgroup needs the same weight at
// the same time, so it is read through the constant cache with workgroup-uniform addresses and costs no LDS traffic and no vector
// load.  Thread t owns column t of its group's filters: one LDS read of x[c][t + k] (consecutive lanes, consecutive words) feeds
// kShallowGroup multiply-adds, summed over (c, k) in index order in one accumulator per filter.  The pool sums its P columns in
// index order.  A value depends on its clip and the weights alone.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }

__global__ __launch_bounds__(kShallowThreads) void shallownet_kernel(ShallowArgs p) {
    extern __shared__ __attribute__((aligned(16))) char shallow_smem[];
    const int C = p.C, T = p.T, K = p.K, Tc = T - K + 1;
    float* const xs = reinterpret_cast<float*>(shallow_smem);                  // [C][T]
    float* const ys = xs + (((size_t)C * T + 3) / 4) * 4;                      // [kShallowGroup][Tc]
    const int tid = threadIdx.x;
    const int groups = (p.F + kShallowGroup - 1) / kShallowGroup;
    const int b = blockIdx.x / groups, f0 = (blockIdx.x - b * groups) * kShallowGroup;

    {
        const float* src = p.eeg + (long long)b * p.clip_stride;
        for (int i = tid; i < C * T; i += kShallowThreads) {
            const int c = i / T, t = i - c * T;
            float v = src[(long long)c * p.channel_stride + t];
            if (p.mean) v = (v - p.mean[i]) / p.scale[i];
            xs[i] = v;
        }
    }
    __syncthreads();

    // the group's filters, interleaved [c K + k][kShallowGroup]: one 16-byte scalar load per (c, k), the same for every thread
    const f32x4* __restrict__ w = reinterpret_cast<const f32x4*>(p.w) + (size_t)(f0 / kShallowGroup) * C * K;
    for (int t = tid; t < Tc; t += kShallowThreads) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int c = 0; c < C; ++c) {
            const float* x = xs + c * T + t;
            const f32x4* wc = w + c * K;
#pragma unroll 5
            for (int k = 0; k < K; ++k) {
                const float xv = x[k];
                const f32x4 wv = wc[k];
                a0 = fmaf(wv.x, xv, a0);
                a1 = fmaf(wv.y, xv, a1);
                a2 = fmaf(wv.z, xv, a2);
                a3 = fmaf(wv.w, xv, a3);
            }
        }
        const float acc[kShallowGroup] = {a0, a1, a2, a3};
#pragma unroll
        for (int g = 0; g < kShallowGroup; ++g)
            if (f0 + g < p.F) ys[g * Tc + t] = elu1(acc[g] + p.c[f0 + g]);
    }
    __syncthreads();

    const int cols = (Tc - p.P) / p.S + 1;
    float* const out = p.out + (size_t)b * p.ldo;
    for (int i = tid; i < kShallowGroup * cols; i += kShallowThreads) {
        const int g = i / cols, j = i - g * cols;
        if (f0 + g >= p.F) continue;
        const float* y = ys + g * Tc + p.S * j;
        float acc = 0.f;
        for (int q = 0; q < p.P; ++q) acc += y[q];
        out[(size_t)(f0 + g) * cols + j] = acc / (float)p.P;
    }
}

// the folded filter as the kernel reads it, from the torch-layout tensors of the state dict (host arithmetic, folded in double, one
// rounding): w [groups][C K][kShallowGroup] -- filter f is lane f % kShallowGroup of group f / kShallowGroup, zeros past F -- then
// c [groups kShallowGroup]
std::vector<float> shallownet_fold(const ShallowHostW& h, int C, int F, int K, float bn_eps) {
    const int groups = (F + kShallowGroup - 1) / kShallowGroup;
    const size_t CK = (size_t)C * K;
    std::vector<float> pk((size_t)groups * kShallowGroup * (CK + 1), 0.f);
    std::vector<double> row(CK);
    for (int f = 0; f < F; ++f) {
        const double scale = (double)h.bn[f] / std::sqrt((double)h.bn[3 * F + f] + (double)bn_eps);
        const double shift = (double)h.bn[F + f] - (double)h.bn[2 * F + f] * scale;
        std::fill(row.begin(), row.end(), 0.0);
        double cst = (double)h.b2[f];
        for (int g = 0; g < F; ++g)
            for (int c = 0; c < C; ++c) {
                const double m = (double)h.w2[((size_t)f * F + g) * C + c];
                cst += m * (double)h.b1[g];
                for (int k = 0; k < K; ++k) row[(size_t)c * K + k] += m * (double)h.w1[(size_t)g * K + k];
            }
        float* dst = pk.data() + (size_t)(f / kShallowGroup) * CK * kShallowGroup + f % kShallowGroup;
        for (size_t i = 0; i < CK; ++i) dst[i * kShallowGroup] = (float)(row[i] * scale);
        pk[(size_t)groups * kShallowGroup * CK + f] = (float)(cst * scale + shift);
    }
    return pk;
}

void shallownet(const ShallowArgs& a, hipStream_t s) {
    E2V_REQUIRE(a.B >= 1 && a.C >= 1 && a.F >= 1 && a.K >= 1 && a.P >= 1 && a.S >= 1 && a.T >= a.K + a.P - 1, E2V_ESHAPE,
                "ShallowNet: positive sizes, at least taps + pool - 1 samples (one pooled column)");
    const int groups = (a.F + kShallowGroup - 1) / kShallowGroup;
    E2V_REQUIRE((long long)a.B * groups <= 0x7FFFFFFFLL, E2V_ESHAPE, "ShallowNet: B * filter groups must stay below 2^31");
    const size_t smem = shallownet_lds_bytes(a.C, a.T, a.K);
    E2V_REQUIRE(smem <= (size_t)kShallowMaxLdsBytes, E2V_ESHAPE,
                "ShallowNet: one clip with a group's columns needs " + std::to_string(smem) + " bytes of LDS, the kernel has " + std::to_string(kShallowMaxLdsBytes));
    E2V_REQUIRE((a.mean == nullptr) == (a.scale == nullptr), E2V_EINVAL, "ShallowNet: the scaler is a mean AND a scale, or neither");
    E2V_REQUIRE(a.eeg && a.w && a.c && a.out && a.ldo >= a.F * shallownet_columns(a.T, a.K, a.P, a.S), E2V_EINVAL, "ShallowNet: null argument or a short output row");
    const double cols = (double)a.B * a.F * (a.T - a.K + 1);
    std::string pname = "shallownet";
    if (prof_detail()) pname += " B" + std::to_string(a.B) + " C" + std::to_string(a.C) + " T" + std::to_string(a.T) + " F" + std::to_string(a.F);
    ProfScope ps(pname.c_str(), 2.0 * cols * a.C * a.K, 4.0 * a.B * ((double)groups * a.C * a.T + (double)a.F * a.C * a.K), s);
    E2V_KATTR(shallownet_kernel, kShallowMaxLdsBytes);
    E2V_KLAUNCH(shallownet_kernel, dim3((unsigned)(a.B * groups)), dim3(kShallowThreads), smem, s, a);
}

// ---------------------------------------------------------------------------------------------------------------------------
// What e2v_glmnet_raw / e2v_glmnet_mlp hand back, one workgroup per clip: the logits without the head's padding columns, the
// concatenated features, the label = argmax of the logits (the LOWEST index among equal maxima; a NaN is never a maximum)
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void glm_outputs_kernel(const float* __restrict__ head, int ldh, const float* __restrict__ feat, int E2, int L,
                                                         float* __restrict__ logits, float* __restrict__ features, int* __restrict__ labels) {
    const int b = blockIdx.x;
    const float* h = head + (size_t)b * ldh;
    if (logits)
        for (int i = threadIdx.x; i < L; i += 64) logits[(size_t)b * L + i] = h[i];
    if (features)
        for (int i = threadIdx.x; i < E2; i += 64) features[(size_t)b * E2 + i] = feat[(size_t)b * E2 + i];
    if (labels && threadIdx.x == 0) {
        int best = 0;
        float m = h[0];
        for (int i = 1; i < L; ++i)
            if (h[i] > m || (m != m && h[i] == h[i])) { m = h[i]; best = i; }
        labels[b] = best;
    }
}

void glm_outputs(const float* head, int ldh, const float* feat, int E2, int L, int B, float* logits, float* features, int* labels, hipStream_t s) {
    E2V_REQUIRE(B >= 1 && L >= 1 && ldh >= L && E2 >= 1 && head && feat, E2V_ESHAPE, "GLMNet outputs: positive sizes");
    ProfScope ps("glm_outputs", 0.0, 4.0 * B * (2.0 * L + 2.0 * E2), s);
    E2V_KLAUNCH(glm_outputs_kernel, dim3((unsigned)B), dim3(64), 0, s, head, ldh, feat, E2, L, logits, features, labels);
}

}  // namespace e2v
