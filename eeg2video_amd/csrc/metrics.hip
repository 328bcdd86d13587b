// Frame metrics (e2v_frame_metrics): per-frame SSIM and MSE of two clips, as the reference scores a sweep
// (EEG2Video/40_class_run_metrics.py:201-233: skimage.metrics.structural_similarity(data_range=255, channel_axis=-1) and
// mse_loss(img1 / 255, img2 / 255)).  A stream over two tensors: every input byte is fetched from HBM about once.
//
// One workgroup (256 threads) scores a tile of kTW x kR window positions of one image, channel after channel:
//   1. its (rows + 6) x (cols + 6) patch of both inputs is read (any type / layout: FrameSrc strides), quantised to bytes ONCE and
//      kept as two byte tiles in LDS; the squared byte difference of the pixels the tile OWNS is taken on the way (every pixel
//      belongs to exactly one tile: the last tile of each direction also owns the 6 rows / columns that start no window);
//   2. thread t owns window column t and walks down the strip: the horizontal 7-sums Sx, Sy, Sxx, Syy, Sxy of the entering row come
//      from the byte tiles, the row that leaves is taken back out of a 7-deep ring the thread keeps in LDS (its own column of it,
//      so no barrier), all in exact int32 arithmetic; from the seventh row on the four fp32 terms and S are formed per position
//      and added into the thread's double.
// With channels-last inputs the passes after the first re-read lines the first one brought into L2.  The halo costs 6 / kR = 19 %
// extra rows and 6 / kTW = 2 % extra columns.  Partials (one double + one uint64 per tile) go to a workspace block and a second
// kernel sums them per image in a fixed order: no atomics, the same bits on every run and at every batch position.
#include "kernels.h"
#include "prof.h"
#include "runtime.h"

namespace e2v {

namespace {

constexpr int kTW = FrameMetricsTile::kCols;     // window columns per tile = threads
constexpr int kR = FrameMetricsTile::kRows;      // window rows per tile
constexpr int kWin = 7;
constexpr int kPitch = kTW + 8;                  // byte-tile row pitch: a multiple of 4, >= (kTW - 4) + 12 (the dword reads of a row)
constexpr int kPatchRows = kR + kWin - 1;

struct Partial {
    double s;                                    // sum of S over the tile's window positions, all channels
    unsigned long long q;                        // sum of (qa - qb)^2 over the pixels the tile owns, all channels
};

// element strides of one input as the kernel walks it
struct SrcView {
    const void* p;
    int f32;
    long long s_img, s_c, s_y, s_x;              // (i, f) image, channel, row, column -- in elements
    long long s_n;                               // clip
};

__device__ __forceinline__ unsigned quantise(float x) {
    x = x > 0.f ? x : 0.f;                       // NaN -> 0
    x = x < 1.f ? x : 1.f;
    return (unsigned)(x * 255.f);                // truncation, the bytes of frames_to_u8 on [0, 1]
}

template <bool F32>
__device__ __forceinline__ unsigned load_q(const SrcView& v, long long off) {
    if (F32) return quantise(static_cast<const float*>(v.p)[off]);
    return static_cast<const unsigned char*>(v.p)[off];
}

constexpr int kLoadBatch = 8;                    // patch elements a thread has in flight per input

template <bool AF32, bool BF32>
__global__ __launch_bounds__(256) void frame_metrics_tiles_kernel(SrcView a, SrcView b, int F, int C, int H, int W, int ntx, int nty,
                                                                   Partial* __restrict__ partials) {
    __shared__ __attribute__((aligned(8))) unsigned char ta[kPatchRows * kPitch], tb[kPatchRows * kPitch];
    __shared__ int ring[kWin][4][kTW];           // per thread: (Sx | Sy << 16), Sxx, Syy, Sxy of the last 7 rows
    __shared__ double red_s[4];
    __shared__ unsigned long long red_q[4];

    const int tid = threadIdx.x;
    const int ntiles = ntx * nty;
    const int img = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const int ty = tile / ntx, tx = tile % ntx;
    const int clip = img / F, f = img % F;
    const int y0 = ty * kR, x0 = tx * kTW;
    const int rows = min(kR, H - 6 - y0), cols = min(kTW, W - 6 - x0);     // window positions of this tile
    const int ph = rows + 6, pw = cols + 6;                                // its patch: inside the image by construction
    const int own_h = ty == nty - 1 ? ph : rows, own_w = tx == ntx - 1 ? pw : cols;
    const long long base_a = clip * a.s_n + f * a.s_img + y0 * a.s_y + x0 * a.s_x;
    const long long base_b = clip * b.s_n + f * b.s_img + y0 * b.s_y + x0 * b.s_x;

    double ssum = 0.0;
    unsigned sq = 0;                             // at most 40 pixels x 4 channels x 255^2 per thread
    for (int c = 0; c < C; ++c) {
        if (c) __syncthreads();                  // the previous channel's tiles are still being read
        // kLoadBatch loads of each input are issued before the first is used; an index past the patch is clamped to its last
        // element for the load (always an address inside the image) and dropped afterwards
        const int total = ph * pw;
        for (int i0 = tid; i0 < total; i0 += 256 * kLoadBatch) {
            unsigned qa[kLoadBatch], qb[kLoadBatch];
            int at[kLoadBatch];
#pragma unroll
            for (int u = 0; u < kLoadBatch; ++u) {
                const int idx = min(i0 + 256 * u, total - 1);
                const int py = idx / pw, px = idx - py * pw;
                qa[u] = load_q<AF32>(a, base_a + c * a.s_c + py * a.s_y + px * a.s_x);
                qb[u] = load_q<BF32>(b, base_b + c * b.s_c + py * b.s_y + px * b.s_x);
                at[u] = i0 + 256 * u < total ? (py * kPitch + px) | (py < own_h && px < own_w ? 1 << 30 : 0) : -1;
            }
#pragma unroll
            for (int u = 0; u < kLoadBatch; ++u) {
                if (at[u] < 0) continue;
                ta[at[u] & 0xFFFF] = (unsigned char)qa[u];
                tb[at[u] & 0xFFFF] = (unsigned char)qb[u];
                if (at[u] >> 30) {
                    const int d = (int)qa[u] - (int)qb[u];
                    sq += (unsigned)(d * d);
                }
            }
        }
        __syncthreads();
        if (tid < cols) {
            int vx = 0, vy = 0, vxx = 0, vyy = 0, vxy = 0;
            for (int r = 0; r < ph; ++r) {
                // bytes tid .. tid + 6 of the row: three aligned dwords (read past the patch only inside the row's pitch, and those
                // bytes are shifted or masked away), funnel-shifted into 4 + 3 bytes; the sums are byte dot products (v_dot4_u32_u8)
                const unsigned* ra = reinterpret_cast<const unsigned*>(ta + r * kPitch + (tid & ~3));
                const unsigned* rb = reinterpret_cast<const unsigned*>(tb + r * kPitch + (tid & ~3));
                const unsigned sh = tid & 3, ones = 0x01010101u;
                const unsigned xl = __builtin_amdgcn_alignbyte(ra[1], ra[0], sh), xh = __builtin_amdgcn_alignbyte(ra[2], ra[1], sh) & 0xFFFFFFu;
                const unsigned yl = __builtin_amdgcn_alignbyte(rb[1], rb[0], sh), yh = __builtin_amdgcn_alignbyte(rb[2], rb[1], sh) & 0xFFFFFFu;
                const int hx = (int)__builtin_amdgcn_udot4(xh, ones, __builtin_amdgcn_udot4(xl, ones, 0u, false), false);
                const int hy = (int)__builtin_amdgcn_udot4(yh, ones, __builtin_amdgcn_udot4(yl, ones, 0u, false), false);
                const int hxx = (int)__builtin_amdgcn_udot4(xh, xh, __builtin_amdgcn_udot4(xl, xl, 0u, false), false);
                const int hyy = (int)__builtin_amdgcn_udot4(yh, yh, __builtin_amdgcn_udot4(yl, yl, 0u, false), false);
                const int hxy = (int)__builtin_amdgcn_udot4(xh, yh, __builtin_amdgcn_udot4(xl, yl, 0u, false), false);
                const int slot = r % kWin;
                if (r >= kWin) {                 // the row that leaves the window
                    const int pxy = ring[slot][0][tid];
                    vx -= pxy & 0xFFFF; vy -= pxy >> 16;
                    vxx -= ring[slot][1][tid]; vyy -= ring[slot][2][tid]; vxy -= ring[slot][3][tid];
                }
                vx += hx; vy += hy; vxx += hxx; vyy += hyy; vxy += hxy;
                ring[slot][0][tid] = hx | (hy << 16);
                ring[slot][1][tid] = hxx; ring[slot][2][tid] = hyy; ring[slot][3][tid] = hxy;
                if (r >= kWin - 1) {
#pragma clang fp contract(off)                   // equal integers must give equal terms: identical images score exactly 1
                    // N = 49; every integer below fits int32 (the largest, 2 * 49 * 49 * 65025, is 3.1e8)
                    const float c1 = 6.5025f, c2 = 58.5225f;
                    const float inv_nn = 1.f / 2401.f, inv_nn1 = 1.f / 2352.f;
                    const float a1 = (float)(2 * vx * vy) * inv_nn + c1;
                    const float a2 = (float)(2 * (49 * vxy - vx * vy)) * inv_nn1 + c2;
                    const float b1 = (float)(vx * vx + vy * vy) * inv_nn + c1;
                    const float b2 = (float)(49 * (vxx + vyy) - vx * vx - vy * vy) * inv_nn1 + c2;
                    ssum += (double)((a1 * a2) / (b1 * b2));
                }
            }
        }
    }

    unsigned long long q = sq;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ssum += __shfl_xor(ssum, off);
        q += __shfl_xor(q, off);
    }
    if ((tid & 63) == 0) { red_s[tid >> 6] = ssum; red_q[tid >> 6] = q; }
    __syncthreads();
    if (tid == 0) {
        Partial p;
        p.s = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
        p.q = red_q[0] + red_q[1] + red_q[2] + red_q[3];
        partials[blockIdx.x] = p;
    }
}

// one image per wave: lane l sums tiles l, l + 64, ... in that order, then a butterfly over the lanes
__global__ __launch_bounds__(256) void frame_metrics_finalize_kernel(const Partial* __restrict__ partials, int images, int ntiles,
                                                                      double ssim_count, double mse_denom, float* __restrict__ ssim,
                                                                      float* __restrict__ mse) {
    const int img = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (img >= images) return;                   // (whole waves leave: the shuffles below see full waves)
    double s = 0.0;
    unsigned long long q = 0;
    for (int t = lane; t < ntiles; t += 64) {
        const Partial p = partials[(size_t)img * ntiles + t];
        s += p.s;
        q += p.q;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s += __shfl_xor(s, off);
        q += __shfl_xor(q, off);
    }
    if (lane == 0) {
        if (ssim) ssim[img] = (float)(s / ssim_count);
        if (mse) mse[img] = (float)((double)q / mse_denom);
    }
}

SrcView view_of(const FrameSrc& s, int F, int C, int H, int W) {
    SrcView v;
    v.p = s.p;
    v.f32 = s.f32;
    if (s.channels_last) {                       // [n, F, H, W, C]
        v.s_x = C; v.s_y = (long long)W * C; v.s_c = 1; v.s_img = (long long)H * W * C; v.s_n = v.s_img * F;
    } else {                                     // [n, C, F, H, W]
        v.s_x = 1; v.s_y = W; v.s_img = (long long)H * W; v.s_c = v.s_img * F; v.s_n = v.s_c * C;
    }
    return v;
}

}  // namespace

long long frame_metrics_tiles(int H, int W) {
    return (long long)((H - 6 + kR - 1) / kR) * ((W - 6 + kTW - 1) / kTW);
}

size_t frame_metrics_partials_bytes(int n, int F, int H, int W) {
    return (size_t)n * F * (size_t)frame_metrics_tiles(H, W) * sizeof(Partial);
}

void frame_metrics(const FrameSrc& a, const FrameSrc& b, int n, int F, int C, int H, int W, void* partials, float* ssim, float* mse,
                   hipStream_t s) {
    const int nty = (H - 6 + kR - 1) / kR, ntx = (W - 6 + kTW - 1) / kTW;
    const int images = n * F;
    const double px = (double)images * C * H * W;
    ProfScope ps("frame_metrics", 60.0 * px, px * ((a.f32 ? 4.0 : 1.0) + (b.f32 ? 4.0 : 1.0)), s);
    const dim3 grid((unsigned)(images * ntx * nty));
    const SrcView va = view_of(a, F, C, H, W), vb = view_of(b, F, C, H, W);
    Partial* const part = static_cast<Partial*>(partials);
    if (a.f32 && b.f32) E2V_KLAUNCH((frame_metrics_tiles_kernel<true, true>), grid, dim3(256), 0, s, va, vb, F, C, H, W, ntx, nty, part);
    else if (a.f32) E2V_KLAUNCH((frame_metrics_tiles_kernel<true, false>), grid, dim3(256), 0, s, va, vb, F, C, H, W, ntx, nty, part);
    else if (b.f32) E2V_KLAUNCH((frame_metrics_tiles_kernel<false, true>), grid, dim3(256), 0, s, va, vb, F, C, H, W, ntx, nty, part);
    else E2V_KLAUNCH((frame_metrics_tiles_kernel<false, false>), grid, dim3(256), 0, s, va, vb, F, C, H, W, ntx, nty, part);
    E2V_KLAUNCH(frame_metrics_finalize_kernel, dim3((unsigned)((images + 3) / 4)), dim3(256), 0, s, static_cast<const Partial*>(partials),
                images, ntx * nty, (double)C * (H - 6) * (double)(W - 6), 65025.0 * C * H * (double)W, ssim, mse);
}

}  // namespace e2v
