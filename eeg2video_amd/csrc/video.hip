// Kernels of the VideoMAE video classifier (transformers VideoMAEForVideoClassification behind e2v_video_classify: the classifier
// half of video_classify_metric, EEG2Video/40_class_run_metrics.py:108-142), and what the three frame-input towers share: the frame
// processor (Pillow's antialiased resize to a target of which only a window is computed -- the whole S x S image for ViT, the centre
// crop of the shortest-edge resize for VideoMAE and CLIP --, fused with the pixel table and the tubelet patch layout) and the token
// rows (with or without a class token); then attention over any number of tokens and the mean over a clip's tokens.  fp32 by default
// whatever the context's compute mode; the preprocess, the token rows and the mean also come over 16-bit rows for a tower in 16-bit
// mode (e2v_set_tower_dtype).
#include <algorithm>
#include <type_traits>

#include "act_io.h"
#include "h16.h"
#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

// ---------------------------------------------------------------------------------------------------------------------------
// VideoMAEImageProcessor: resize(size = {"shortest_edge": E}) -> get_resize_output_image_size(default_to_square = False): the
// short side becomes E, the long side int(E * long / short); center_crop(S, S): top = (nh - S) // 2, left = (nw - S) // 2.
// ---------------------------------------------------------------------------------------------------------------------------
PrepWindow video_crop(int H, int W, int edge, int S) {
    PrepWindow c;
    if (H <= W) { c.nh = edge; c.nw = (int)((long long)edge * W / H); }
    else { c.nh = (int)((long long)edge * H / W); c.nw = edge; }
    c.top = (c.nh - S) / 2;
    c.left = (c.nw - S) / 2;
    return c;
}

// The tables of the two axes ((W -> nw), (H -> nh): the targets may differ), sliced to the window: output row yy of the window is
// row top + yy of the (H -> nh) table, output column xx is column left + xx of the (W -> nw) table.  Pillow computes the whole
// resized image and a crop discards the rest; a sample inside the window depends on its own taps only, so the window's bytes are
// Pillow's.  The vertical-first exception (PIL/Image.py: `self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`) is decided
// by the source and the resize target, as there.
// The band of output rows a workgroup of the preprocess kernel takes: the resized source rows the band reads stay in LDS as bytes.
// One patch row (P output rows) where that fits, else the largest band that does; 0: not even one row.
PrepPlan prep_plan(int H, int W, const PrepWindow& win, int S, int P, const float* lut768, int filter) {
    PrepPlan p;
    p.H = H; p.W = W; p.S = S;
    const ResizeAxis hf = resize_axis(W, win.nw, filter), vf = resize_axis(H, win.nh, filter);
    p.kh = hf.ksize; p.kv = vf.ksize;
    p.vfirst = (long long)H > 100LL * W && win.nh < H;
    const int top = win.top, left = win.left;
    auto vfirst_of = [&](int yy) { return vf.first[top + yy]; };
    auto vcount_of = [&](int yy) { return vf.count[top + yy]; };
    p.c0 = hf.first[left];
    int c1 = p.c0;
    for (int xx = 0; xx < S; ++xx) {
        p.c0 = std::min(p.c0, hf.first[left + xx]);
        c1 = std::max(c1, hf.first[left + xx] + hf.count[left + xx]);
    }
    p.cw = c1 - p.c0;
    auto rows_of = [&](int band) {
        int most = 0;
        for (int y0 = 0; y0 < S; y0 += band) {
            const int y1 = std::min(y0 + band, S) - 1;
            int lo = vfirst_of(y0), hi = vfirst_of(y0) + vcount_of(y0);
            for (int y = y0; y <= y1; ++y) { lo = std::min(lo, vfirst_of(y)); hi = std::max(hi, vfirst_of(y) + vcount_of(y)); }
            // (the kernel takes the band's source rows as [first of its first row, end of its last row): both ends are monotonic)
            if (lo != vfirst_of(y0) || hi != vfirst_of(y1) + vcount_of(y1)) return 1 << 30;
            most = std::max(most, hi - lo);
        }
        return most;
    };
    for (int band = std::min(P, S); band >= 1; --band) {                         // (vertical first: the band's rows over the columns read)
        const int rows = p.vfirst ? band : rows_of(band);
        if ((long long)rows * (p.vfirst ? p.cw : S) <= kImagePrepLdsBytes) { p.band = band; p.band_rows = rows; break; }
    }
    p.words.reserve((size_t)4 * S + (size_t)S * (p.kh + p.kv) + 768);
    for (int xx = 0; xx < S; ++xx) p.words.push_back(hf.first[left + xx]);
    for (int xx = 0; xx < S; ++xx) p.words.push_back(hf.count[left + xx]);
    for (int yy = 0; yy < S; ++yy) p.words.push_back(vf.first[top + yy]);
    for (int yy = 0; yy < S; ++yy) p.words.push_back(vf.count[top + yy]);
    p.words.insert(p.words.end(), hf.coeff.begin() + (size_t)left * p.kh, hf.coeff.begin() + (size_t)(left + S) * p.kh);
    p.words.insert(p.words.end(), vf.coeff.begin() + (size_t)top * p.kv, vf.coeff.begin() + (size_t)(top + S) * p.kv);
    for (int i = 0; i < 768; ++i) p.words.push_back(__builtin_bit_cast(int, lut768[i]));
    return p;
}

namespace {

struct PrepView {
    const void* p;
    long long s_n, s_img, s_c, s_y, s_x;         // clip, frame, channel, row, column -- in elements
};

__device__ __forceinline__ int prep_quantise(float x) {      // the bytes of frames_to_u8 on [0, 1]; NaN -> 0 (metrics.hip: quantise)
    x = x > 0.f ? x : 0.f;
    x = x < 1.f ? x : 1.f;
    return (int)(x * 255.f);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

template <bool F32>
__device__ __forceinline__ int prep_load(const PrepView& v, long long off) {
    return F32 ? prep_quantise(static_cast<const float*>(v.p)[off]) : (int)static_cast<const unsigned char*>(v.p)[off];
}

// One workgroup: `band` output rows of one channel of one frame.
//   1. horizontal pass over the source rows the band reads -> bytes in LDS ([rows][S]; staging in LDS instead of a byte buffer in
//      the pool: the intermediate of a band is consumed by the workgroup that made it, 5 KB at 288 x 512 -> 224, and never visits HBM);
//   2. vertical pass over those bytes -> byte -> pixel table -> the patch-row matrix.
// Integer arithmetic as Pillow's: 32-bit accumulators starting at 2^21, >> 22, clipped to a byte.
// VFIRST (Pillow's order for very tall images): 1. vertical pass of the band's rows over the source columns [c0, c0 + cw) the window
// reads -> bytes in LDS ([band][cw]); 2. horizontal pass over them.
// Frame f = ts t + dt of a clip writes column ((c ts + dt) P + y) P + x of token row (t, py, px).  The launch covers frames img0 .. of
// the [n][F] source, from a multiple of ts on (t counts the launch's tubelets); at ts = 1 every frame is an image of its own.
// O: the patch rows' storage type -- fp32, or bf16 / fp16 (a tower in 16-bit mode): the table's fp32 value rounded once, at the store.
template <bool F32, bool VFIRST, typename O>
__global__ __launch_bounds__(256) void frame_prep_kernel(PrepView v, int F, int ts, long long img0, int S, int P, int kh, int kv, int band,
                                                         int c0, int cw, const int* __restrict__ plan, O* __restrict__ rows) {
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
    const int t = blockIdx.z / ts, dt = blockIdx.z - t * ts;                 // (F and img0 are multiples of ts)
    const long long base = clip * v.s_n + f * v.s_img + c * v.s_c;
    const int np = S / P;
    const size_t K = (size_t)3 * ts * P * P;
    const size_t row0 = (size_t)t * np * np;
    const size_t col0 = (size_t)(c * ts + dt) * P * P;
    auto put = [&](int yy, int xx, int byte) {
        const int py = yy / P, px = xx / P;
        rows[(row0 + (size_t)py * np + px) * K + col0 + (yy - py * P) * P + (xx - px * P)] = (O)lut[c * 256 + byte];
    };
    if (VFIRST) {
        for (int i = threadIdx.x; i < (y1 - y0) * cw; i += 256) {
            const int ry = i / cw, x = i - ry * cw, yy = y0 + ry;
            const long long coloff = base + (long long)(c0 + x) * v.s_x;
            const int first = vfirst[yy], cnt = vcount[yy];
            int acc = 1 << 21;
            for (int k = 0; k < cnt; ++k) acc += vco[yy * kv + k] * prep_load<F32>(v, coloff + (long long)(first + k) * v.s_y);
            prep_tmp[i] = (unsigned char)clip8(acc >> 22);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < (y1 - y0) * S; i += 256) {
            const int ry = i / S, xx = i - ry * S;
            const int x0 = hfirst[xx] - c0, cnt = hcount[xx];
            int acc = 1 << 21;
            for (int k = 0; k < cnt; ++k) acc += hco[xx * kh + k] * (int)prep_tmp[ry * cw + x0 + k];
            put(y0 + ry, xx, clip8(acc >> 22));
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
        put(yy, xx, clip8(acc >> 22));
    }
}

}  // namespace

void frame_preprocess(const FrameSrc& src, int n, int F, int ts, long long img0, int nimg, const PrepPlan& plan, const int* plan_dev, int P,
                      float* rows, const char* name, hipStream_t s, int h16) {
    E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, "frame preprocess: the source rows of one output row do not fit the kernel's LDS band");
    E2V_REQUIRE(ts >= 1 && F % ts == 0 && img0 % ts == 0 && nimg % ts == 0 && nimg >= 1 && nimg <= 65535 && img0 >= 0 &&
                    img0 + nimg <= (long long)n * F,
                E2V_EINVAL, "frame preprocess: bad frame range");
    const int S = plan.S;
    const long long HW = (long long)plan.H * plan.W;
    PrepView v;
    v.p = src.p;
    if (src.channels_last) { v.s_n = (long long)F * HW * 3; v.s_img = HW * 3; v.s_c = 1; v.s_y = (long long)plan.W * 3; v.s_x = 3; }
    else { v.s_n = 3LL * F * HW; v.s_img = HW; v.s_c = (long long)F * HW; v.s_y = plan.W; v.s_x = 1; }
    const size_t smem = (size_t)plan.band_rows * (plan.vfirst ? plan.cw : S);
    const dim3 grid((S + plan.band - 1) / plan.band, 3, nimg);
    ProfScope ps(name, 2.0 * nimg * 3 * S * ((double)plan.band_rows * (S / plan.band + 1) * plan.kh + (double)S * plan.kv),
                 (double)nimg * 3 * ((double)S * plan.W * (src.f32 ? 4.0 : 1.0) + (h16 ? 2.0 : 4.0) * S * S), s);
    auto launch_as = [&](auto* out) {
        using O = std::remove_pointer_t<decltype(out)>;
        auto launch = [&](auto kernel) {
            E2V_KLAUNCH(kernel, grid, dim3(256), smem, s, v, F, ts, img0, S, P, plan.kh, plan.kv, plan.band, plan.c0, plan.cw, plan_dev, out);
        };
        if (plan.vfirst) { if (src.f32) launch(frame_prep_kernel<true, true, O>); else launch(frame_prep_kernel<false, true, O>); }
        else { if (src.f32) launch(frame_prep_kernel<true, false, O>); else launch(frame_prep_kernel<false, false, O>); }
    };
    if (!h16) return launch_as(rows);
    h16_dispatch(h16, [&](auto tag) { launch_as(reinterpret_cast<decltype(tag)*>(rows)); });
}

// ---------------------------------------------------------------------------------------------------------------------------
// token rows: x[b T + t] = patch row (b, t) + pos[t], or, with a class token, x[b T] = cls + pos[0] and x[b T + 1 + p] = patch row
// (b, p) + pos[1 + p]; one wave per row, 16 bytes of fp32 per lane and step.  X: the storage type of the patch and token rows (fp32,
// or the 16-bit rows of a tower in 16-bit mode); the class row and the positions are fp32, the sum is fp32 and is rounded once, at
// the store.
// ---------------------------------------------------------------------------------------------------------------------------
template <typename X>
__global__ __launch_bounds__(256) void token_embed_kernel(const X* __restrict__ patches, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, X* __restrict__ out, long long rows, int T, int C) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const long long b = row / T;
    const int t = (int)(row - b * T);
    const X* a = patches + (size_t)(cls ? row - b - 1 : row) * C;          // (the class row, t == 0: not read)
    const float* p = pos + (size_t)t * C;
    X* o = out + (size_t)row * C;
    const bool is_cls = cls && t == 0;
    for (int c = 4 * lane; c < C; c += 256) st4(o + c, (is_cls ? ld4(cls + c) : ld4(a + c)) + ld4(p + c));
}

void token_embed(const float* patches, const float* cls, const float* pos, float* x, int B, int T, int C, hipStream_t s, int h16) {
    const long long rows = (long long)B * T;
    ProfScope ps(cls ? "image_embed" : "video_embed", (double)rows * C, (h16 ? 8.0 : 12.0) * rows * C, s);
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (!h16) { E2V_KLAUNCH(token_embed_kernel<float>, grid, dim3(256), 0, s, patches, cls, pos, x, rows, T, C); return; }
    h16_dispatch(h16, [&](auto tag) {
        using H = decltype(tag);
        E2V_KLAUNCH(token_embed_kernel<H>, grid, dim3(256), 0, s, reinterpret_cast<const H*>(patches), cls, pos, reinterpret_cast<H*>(x), rows, T, C);
    });
}

// ---------------------------------------------------------------------------------------------------------------------------
// Attention over the T tokens of a clip.  At 588 (6 frames) to 1568 (16 frames) keys of 64 dims a head's K and V are 301 to 803 KB:
// they cannot stay in LDS as image_attn_kernel (vit.hip) keeps them, so this is the fp32 matrix-instruction kernel of the UNet's attention
// (attn.hip: flash_attn_kernel<64>, S^T = K Q^T with the query on the lane, online softmax in the exp2 domain, K and V staged per
// key tile) called as a cross-attention of every sequence to itself: mode 1, one "frame" per sample, Nq = Nk = T.  The order of a
// row's sums is the key-tile order: it depends on T alone.  A kernel of its own for this shape -- 8 waves / 256 queries per
// workgroup over 64-key stages, workgroups dealt to the XCDs by (sequence, head) -- gave the same bits and was 1.27x SLOWER at
// 16 x 12 x 588 (0.221 against 0.174 ms) and 1.33x at 1568: 162 VGPRs leave one such workgroup per CU.  It is not here.
// ---------------------------------------------------------------------------------------------------------------------------
void token_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s) {
    E2V_REQUIRE(B >= 1 && heads >= 1 && T >= 1, E2V_ESHAPE, "token attention: B, heads, T >= 1");
    const int C = heads * 64;
    AttnArgs a;
    a.q = qkv; a.ldq = ldqkv; a.k = qkv + C; a.v = qkv + 2 * C; a.ldkv = ldqkv; a.o = out; a.ldo = ldo;
    a.n = B; a.F = 1; a.heads = heads; a.D = 64; a.Nq = T; a.Nk = T; a.mode = 1; a.scale = 0.125f;
    flash_attention(a, s);
}

// ---------------------------------------------------------------------------------------------------------------------------
// mean over the T token rows of a clip: one thread per (clip, column), the rows added in index order (a fixed order, no atomics),
// eight loads in flight per thread; then one division by T (torch's mean: sum / count)
// ---------------------------------------------------------------------------------------------------------------------------
// X: fp32 rows, or the 16-bit rows of a tower in 16-bit mode (widened exactly; the sum and the output stay fp32).
template <typename X>
__global__ __launch_bounds__(256) void token_mean_kernel(const X* __restrict__ x, float* __restrict__ out, int T, int C) {
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= C) return;
    const X* p = x + (size_t)blockIdx.y * T * C + col;
    float acc = 0.f;
    int t = 0;
    for (; t + 8 <= T; t += 8) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (float)p[(size_t)(t + e) * C];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc += v[e];
    }
    for (; t < T; ++t) acc += (float)p[(size_t)t * C];
    out[(size_t)blockIdx.y * C + col] = acc / (float)T;
}

void token_mean(const float* x, float* out, int B, int T, int C, hipStream_t s, int h16) {
    E2V_REQUIRE(B >= 1 && B <= 65535, E2V_ESHAPE, "token mean: 1 <= B <= 65535");
    ProfScope ps("token_mean", (double)B * T * C, (h16 ? 2.0 : 4.0) * B * T * C + 4.0 * B * C, s);
    const dim3 grid((C + 255) / 256, B);
    if (!h16) { E2V_KLAUNCH(token_mean_kernel<float>, grid, dim3(256), 0, s, x, out, T, C); return; }
    h16_dispatch(h16, [&](auto tag) {
        using H = decltype(tag);
        E2V_KLAUNCH(token_mean_kernel<H>, grid, dim3(256), 0, s, reinterpret_cast<const H*>(x), out, T, C);
    });
}

}  // namespace e2v
