// The 8 leftover value columns of flash_attn_kernel<40> (csrc/attn.hip), three ways, in a loop shaped like one 32-key tile of that
// kernel: 20 + 16 v_mfma_f32_32x32x2_f32 fed from LDS, 16 v_exp_f32, then  rem[c] += V[key][32 + c] * P[query][key]  over the lane's
// 16 keys as
//   form 0: 32 broadcast ds_read_b128 + 128 lane-FMAs as v_pk_fma_f32 / v_fma_f32 (each lane all 8 columns of its query),
//   form 1: 32 ds_read_b32 + 32 v_mfma_f32_4x4x1_16b_f32 (lane 4b+i supplies A = V[key][32 + 4g + i], B = P; D[i] lands in lane 4b+j
//           as column 32 + 4g + i of query j's lane: the same registers as form 0),
//   form 2: the same MFMAs fed by 16 ds_read_b64 from an image whose columns 32..39 are stored interleaved (32, 36, 33, 37, ...).
// One wave per SIMD (256 blocks of 4 waves).  Prints the time per tile of every form over alternating rounds and checks every form's
// rem registers for exact equality with a host fmaf loop in the same key order; that check is also the check of the operand layout.
//   hipcc -O3 --offload-arch=gfx950 -mllvm -amdgpu-mfma-vgpr-form=1 tools/micro/attn_leftover.hip -o tools/micro/attn_leftover
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int D = 40, LD = D + 4, G = D / 8, KT = 32;
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// kimg / vimg: [32][LD] LDS images; p: [64][16] per-lane probabilities; q: [64][G][4]; rem_out: [blocks][256][8]; sink keeps the rest live
template <int FORM>
__global__ __launch_bounds__(256) void tile_loop(const float* __restrict__ kimg, const float* __restrict__ vimg, const float* __restrict__ pin,
                                                 const float* __restrict__ qin, float* __restrict__ rem_out, float* __restrict__ sink, const int iters) {
    __shared__ __attribute__((aligned(16))) float smem[2 * KT * LD];
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    for (int i = tid; i < 2 * KT * LD; i += 256) smem[i] = i < KT * LD ? kimg[i] : vimg[i - KT * LD];
    __syncthreads();
    const float* Ks = smem;
    const float* Vs = smem + KT * LD;
    f32x4 qf[G];
    f32x16 pfix, p;
    for (int g = 0; g < G; ++g)
        for (int e = 0; e < 4; ++e) qf[g][e] = qin[(lane * G + g) * 4 + e];
    for (int r = 0; r < 16; ++r) pfix[r] = pin[lane * 16 + r];
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 rem0 = {0.f, 0.f, 0.f, 0.f}, rem1 = {0.f, 0.f, 0.f, 0.f};
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int it = 0; it < iters; ++it) {
        asm volatile("" ::: "memory");                       // the LDS reads stay in the loop
        f32x16 st;
        const float* kp = Ks + j * LD + h * 4;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const f32x4 kf = *reinterpret_cast<const f32x4*>(kp + g * 8);
#pragma unroll
            for (int s = 0; s < 4; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[s], qf[g][s], (g == 0 && s == 0) ? zero16 : st, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r)          // the tile's own exp feeds P as in the kernel; its value is pfix (>= 0.01) whatever exp returns (< 2^40)
            p[r] = __builtin_fmaxf(pfix[r], __builtin_amdgcn_exp2f(st[r]) * 0x1p-100f);
        const float* vp = Vs + (4 * h) * LD + j;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[((r & 3) + 8 * (r >> 2)) * LD], p[r], acc, 0, 0, 0);
        if constexpr (FORM == 0) {
            const float* vr = Vs + (4 * h) * LD + 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* row = vr + ((r & 3) + 8 * (r >> 2)) * LD;
                rem0 += *reinterpret_cast<const f32x4*>(row) * p[r];
                rem1 += *reinterpret_cast<const f32x4*>(row + 4) * p[r];
            }
        } else if constexpr (FORM == 1) {
            const float* vr = Vs + (4 * h) * LD + 32 + (lane & 3);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float* row = vr + ((r & 3) + 8 * (r >> 2)) * LD;
                rem0 = __builtin_amdgcn_mfma_f32_4x4x1f32(row[0], p[r], rem0, 0, 0, 0);
                rem1 = __builtin_amdgcn_mfma_f32_4x4x1f32(row[4], p[r], rem1, 0, 0, 0);
            }
        } else {
            const float* vr = Vs + (4 * h) * LD + 32 + 2 * (lane & 3);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f32x2 a = *reinterpret_cast<const f32x2*>(vr + ((r & 3) + 8 * (r >> 2)) * LD);
                rem0 = __builtin_amdgcn_mfma_f32_4x4x1f32(a[0], p[r], rem0, 0, 0, 0);
                rem1 = __builtin_amdgcn_mfma_f32_4x4x1f32(a[1], p[r], rem1, 0, 0, 0);
            }
        }
    }
    float* ro = rem_out + ((size_t)blockIdx.x * 256 + tid) * 8;
    for (int e = 0; e < 4; ++e) { ro[e] = rem0[e]; ro[4 + e] = rem1[e]; }
    float s = 0.f;
    for (int r = 0; r < 16; ++r) s += acc[r];
    sink[(size_t)blockIdx.x * 256 + tid] = s;
}

static float urand(unsigned& s) { s = s * 1664525u + 1013904223u; return (float)(s >> 8) * (1.0f / 16777216.0f); }

int main() {
    constexpr int BLOCKS = 256, NFORM = 3;
    unsigned seed = 12345u;
    std::vector<float> V(KT * D), kimg(KT * LD, 0.f), vimg[2], p(64 * 16), q(64 * G * 4);
    for (auto& x : V) x = 2.f * urand(seed) - 1.f;
    for (int k = 0; k < KT; ++k) for (int c = 0; c < D; ++c) kimg[k * LD + c] = 0.25f * (2.f * urand(seed) - 1.f);
    for (auto& x : p) x = 0.01f + 0.99f * urand(seed);
    for (auto& x : q) x = 2.f * urand(seed) - 1.f;
    for (int f = 0; f < 2; ++f) {
        vimg[f].assign(KT * LD, 0.f);
        for (int k = 0; k < KT; ++k)
            for (int c = 0; c < D; ++c) {
                int pos = c;
                if (f == 1 && c >= 32) pos = 32 + 2 * ((c - 32) & 3) + ((c - 32) >> 2);      // 32, 36, 33, 37, ...
                vimg[f][k * LD + pos] = V[k * D + c];
            }
    }
    float *dk, *dv[2], *dp, *dq, *drem, *dsink;
    CHECK(hipMalloc(&dk, kimg.size() * 4)); CHECK(hipMalloc(&dp, p.size() * 4)); CHECK(hipMalloc(&dq, q.size() * 4));
    CHECK(hipMalloc(&drem, (size_t)BLOCKS * 256 * 8 * 4)); CHECK(hipMalloc(&dsink, (size_t)BLOCKS * 256 * 4));
    CHECK(hipMemcpy(dk, kimg.data(), kimg.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dp, p.data(), p.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dq, q.data(), q.size() * 4, hipMemcpyHostToDevice));
    for (int f = 0; f < 2; ++f) {
        CHECK(hipMalloc(&dv[f], vimg[f].size() * 4));
        CHECK(hipMemcpy(dv[f], vimg[f].data(), vimg[f].size() * 4, hipMemcpyHostToDevice));
    }
    auto launch = [&](int form, int iters) {
        if (form == 0) hipLaunchKernelGGL(tile_loop<0>, dim3(BLOCKS), dim3(256), 0, 0, dk, dv[0], dp, dq, drem, dsink, iters);
        else if (form == 1) hipLaunchKernelGGL(tile_loop<1>, dim3(BLOCKS), dim3(256), 0, 0, dk, dv[0], dp, dq, drem, dsink, iters);
        else hipLaunchKernelGGL(tile_loop<2>, dim3(BLOCKS), dim3(256), 0, 0, dk, dv[1], dp, dq, drem, dsink, iters);
    };
    // exactness: rem of lane (query j, half h) after `iters` tiles, against fmaf in the kernel's key order
    const int citers = 37;
    std::vector<float> want(64 * 8);
    for (int lane = 0; lane < 64; ++lane) {
        const int h = lane >> 5;
        for (int c = 0; c < 8; ++c) {
            float r = 0.f;
            for (int it = 0; it < citers; ++it)
                for (int rr = 0; rr < 16; ++rr) r = fmaf(V[((rr & 3) + 8 * (rr >> 2) + 4 * h) * D + 32 + c], p[lane * 16 + rr], r);
            want[lane * 8 + c] = r;
        }
    }
    bool exact[NFORM];
    std::vector<float> got((size_t)BLOCKS * 256 * 8);
    for (int form = 0; form < NFORM; ++form) {
        CHECK(hipMemset(drem, 0xff, got.size() * 4));
        launch(form, citers);
        CHECK(hipDeviceSynchronize());
        CHECK(hipMemcpy(got.data(), drem, got.size() * 4, hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (size_t t = 0; t < (size_t)BLOCKS * 256; ++t)
            if (memcmp(&got[t * 8], &want[(t & 63) * 8], 32) != 0) ++bad;
        exact[form] = bad == 0;
        printf("form %d: rem registers %s the host fmaf chain (%zu of %d lanes differ)\n", form, bad ? "DIFFER from" : "equal", bad, BLOCKS * 256);
    }
    // time: alternating rounds, the clock warmed by a first untimed round
    const int iters = 20000, rounds = 5;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    float ns[NFORM][rounds];
    for (int r = -1; r < rounds; ++r)
        for (int form = 0; form < NFORM; ++form) {
            CHECK(hipEventRecord(e0));
            launch(form, iters);
            CHECK(hipEventRecord(e1));
            CHECK(hipEventSynchronize(e1));
            float ms;
            CHECK(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) ns[form][r] = ms * 1e6f / iters;
        }
    for (int form = 0; form < NFORM; ++form) {
        float lo = ns[form][0], hi = lo;
        printf("form %d: ns per tile", form);
        for (int r = 0; r < rounds; ++r) { printf(" %.1f", ns[form][r]); lo = fminf(lo, ns[form][r]); hi = fmaxf(hi, ns[form][r]); }
        printf("   min %.1f max %.1f spread %.1f\n", lo, hi, hi - lo);
    }
    return (exact[0] && exact[1] && exact[2]) ? 0 : 1;
}
