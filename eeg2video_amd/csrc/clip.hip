// What the CLIP score (clip_score / clip_score_only / n_way_scores, EEG2Video/40_class_run_metrics.py:20-55,145-188) needs beyond
// the image classifier's kernels: the cosine similarity of embedding rows, pairwise or as a matrix.  The vision tower itself is made
// of kernels that exist: its processor (CLIPImageProcessor: bicubic resize of the shortest edge, centre crop, pixel table) is
// video.hip's crop-window preprocess at one frame per image over bicubic tables, its token rows and attention are vit.hip's, its
// LayerNorms, linears and quick-GELU norm.hip's, igemm.hip's and text.hip's.  fp32 in every compute mode.
#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kSimTile = 16;        // a workgroup of the matrix form: 16 x 16 outputs, one per thread
constexpr int kSimChunk = 64;       // dims staged per step
constexpr int kSimLd = 68;          // LDS row stride in floats: the 16 rows a ds_read_b128 group reads sit 4 banks apart

// The sums of one output: dot(a, b), |a|^2 and |b|^2, each as four partial sums (element d goes to partial d mod 4, d ascending).
struct SimAcc {
    f32x4 ab = {0.f, 0.f, 0.f, 0.f}, aa = {0.f, 0.f, 0.f, 0.f}, bb = {0.f, 0.f, 0.f, 0.f};
    __device__ __forceinline__ void step(const f32x4 a, const f32x4 b) {
        ab.x = fmaf(a.x, b.x, ab.x); ab.y = fmaf(a.y, b.y, ab.y); ab.z = fmaf(a.z, b.z, ab.z); ab.w = fmaf(a.w, b.w, ab.w);
        aa.x = fmaf(a.x, a.x, aa.x); aa.y = fmaf(a.y, a.y, aa.y); aa.z = fmaf(a.z, a.z, aa.z); aa.w = fmaf(a.w, a.w, aa.w);
        bb.x = fmaf(b.x, b.x, bb.x); bb.y = fmaf(b.y, b.y, bb.y); bb.z = fmaf(b.z, b.z, bb.z); bb.w = fmaf(b.w, b.w, bb.w);
    }
    // torch.nn.functional.cosine_similarity: x1 . x2 / (max(||x1||, eps) * max(||x2||, eps)); a zero row: 0 / (eps * ...) = 0
    __device__ __forceinline__ float result(float eps) const {
        const float dot = (ab.x + ab.y) + (ab.z + ab.w);
        const float na = fmaxf(sqrtf((aa.x + aa.y) + (aa.z + aa.w)), eps), nb = fmaxf(sqrtf((bb.x + bb.y) + (bb.z + bb.w)), eps);
        return dot / na / nb;
    }
};

// pairs: one thread per output, both rows read where they are (16 bytes per load)
__global__ __launch_bounds__(256) void clip_similarity_pairs_kernel(const float* __restrict__ a, const float* __restrict__ b, int n, int D,
                                                                    float eps, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const f32x4* pa = reinterpret_cast<const f32x4*>(a + (size_t)i * D);
    const f32x4* pb = reinterpret_cast<const f32x4*>(b + (size_t)i * D);
    SimAcc acc;
    for (int d = 0; d < D / 4; ++d) acc.step(pa[d], pb[d]);
    out[i] = acc.result(eps);
}

// matrix: a workgroup takes rows i0 .. i0 + 15 of a and j0 .. j0 + 15 of b; 64 dims of both tiles are staged in LDS per step (one
// 16-byte load per thread and tile; rows past the end are zeros and their outputs are not stored); thread (ti, tj) runs the sums of
// the pair form over (a[i0 + ti], b[j0 + tj]).
__global__ __launch_bounds__(256) void clip_similarity_matrix_kernel(const float* __restrict__ a, int na, const float* __restrict__ b, int nb,
                                                                     int D, float eps, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float As[kSimTile * kSimLd];
    __shared__ __attribute__((aligned(16))) float Bs[kSimTile * kSimLd];
    const int tj = threadIdx.x & 15, ti = threadIdx.x >> 4;
    const int i0 = blockIdx.y * kSimTile, j0 = blockIdx.x * kSimTile;
    const int lr = threadIdx.x >> 4, lc = (threadIdx.x & 15) * 4;              // the staging load of this thread: row lr, dims lc .. lc + 3
    SimAcc acc;
    for (int d0 = 0; d0 < D; d0 += kSimChunk) {
        const int nd = min(kSimChunk, D - d0);                                 // (a multiple of 4)
        f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
        if (lc < nd) {
            if (i0 + lr < na) va = *reinterpret_cast<const f32x4*>(a + (size_t)(i0 + lr) * D + d0 + lc);
            if (j0 + lr < nb) vb = *reinterpret_cast<const f32x4*>(b + (size_t)(j0 + lr) * D + d0 + lc);
        }
        __syncthreads();                                                       // (the previous step's reads are done)
        *reinterpret_cast<f32x4*>(As + lr * kSimLd + lc) = va;
        *reinterpret_cast<f32x4*>(Bs + lr * kSimLd + lc) = vb;
        __syncthreads();
        for (int d = 0; d < nd; d += 4)
            acc.step(*reinterpret_cast<const f32x4*>(As + ti * kSimLd + d), *reinterpret_cast<const f32x4*>(Bs + tj * kSimLd + d));
    }
    if (i0 + ti < na && j0 + tj < nb) out[(size_t)(i0 + ti) * nb + j0 + tj] = acc.result(eps);
}

}  // namespace

void clip_similarity(const float* a, int na, const float* b, int nb, int D, bool matrix, float eps, float* out, hipStream_t s) {
    E2V_REQUIRE(na >= 1 && nb >= 1 && D >= 4 && D % 4 == 0, E2V_ESHAPE, "clip similarity: na, nb >= 1 and D a positive multiple of 4");
    E2V_REQUIRE(matrix || na == nb, E2V_ESHAPE, "clip similarity: the pair form takes as many rows of a as of b");
    const double outs = matrix ? (double)na * nb : (double)na;
    ProfScope ps(matrix ? "clip_similarity_matrix" : "clip_similarity_pairs", 6.0 * outs * D, 4.0 * ((double)(na + nb) * D + outs), s);
    if (matrix) {
        const int gy = (na + kSimTile - 1) / kSimTile;
        E2V_REQUIRE(gy <= 65535, E2V_ESHAPE, "clip similarity: at most 65535 * 16 rows of a in the matrix form");
        E2V_KLAUNCH(clip_similarity_matrix_kernel, dim3((nb + kSimTile - 1) / kSimTile, gy), dim3(256), 0, s, a, na, b, nb, D, eps, out);
    } else {
        E2V_KLAUNCH(clip_similarity_pairs_kernel, dim3((na + 255) / 256), dim3(256), 0, s, a, b, na, D, eps, out);
    }
}

}  // namespace e2v
