// Launchers of the hand-written gfx950 kernels of the EEG2Video generation hot path.
// All activations are CHANNEL-LAST fp32: a tensor [n, F, H, W, C] is a row-major matrix
// [rows = n*F*H*W][C]; every kernel takes explicit row strides so that slices of a wider
// buffer (fused QKV output, concatenated skip) are read in place.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <string>
#include <vector>

#include "gemm_sched.h"

namespace e2v {

// ---------------------------------------------------------------------------------------
// implicit-GEMM convolution / linear  (igemm.hip)
//   out[m][n] = epilogue( alpha * sum_{tap, c} A[src(m, tap)][c] * W[n][tap*Ctot + c] )
// A comes from up to two channel-last sources (the reference's torch.cat([h, skip], dim=1),
// unet_blocks.py:487,570, is never materialised); src() folds zero padding, stride and the
// nearest-neighbour resize of Upsample3D (resnet.py:58-61) into the gather.
// ---------------------------------------------------------------------------------------
struct IgemmArgs {
    const float* a0 = nullptr; const float* a1 = nullptr;
    int c0 = 0, c1 = 0;            // channels taken from a0 / a1 (multiples of 4)
    int lda0 = 0, lda1 = 0;        // row strides (floats)
    const float* w = nullptr;      // linear: [N][K]; 3x3: [N][chunk of 32][tap][32] (pack_conv3x3)
    int ldw = 0;
    int ldw16 = 0;                 // row length of w16 (3x3: chunks of 64)
    float* out = nullptr; int ldc = 0;
    const float* bias = nullptr;       // [N]
    const float* rowbias = nullptr;    // [samples][rb_ld] (time embedding added after conv1, resnet.py:186)
    int rb_ld = 0; int rows_per_sample = 1;
    const float* resid = nullptr; int ldr = 0;
    int M = 0, N = 0;
    int taps = 1;                  // 1 (linear / 1x1) or 9 (3x3)
    int Ho = 1, Wo = 1;            // output map
    int Hi = 1, Wi = 1;            // logical input map (after nearest resize)
    int Hs = 1, Ws = 1;            // physical source map
    int stride = 1, pad = 0;       // pad = rows/cols of zeros above/left (below/right is implied by Hi/Wi)
    // bgemm256.hip only (the sub-pixel form of a 2x nearest resize + 3x3 conv, bgemm_up2x): kernel width (taps = kh x kw, tap t =
    // (t / kw, t % kw)), the left pad if it differs from the top pad `pad` (-1: the same), and an output scatter -- output pixel
    // (oy, ox) of image i is written to row ((i Ho osy + oy osy + ooy) Wo osx + ox osx + oox) instead of row m (osy = 0: off)
    int kw = 3, pad_x = -1;
    int osy = 0, osx = 0, ooy = 0, oox = 0;
    int upsample = 0; float ups_h = 1.f, ups_w = 1.f;
    float alpha = 1.f;
    int relu = 0;                  // out = max(out, 0) after bias (semantic-predictor MLP)
    int geglu = 0;                 // W rows packed [32 value | 32 gate] per 64: out[m][n/2] = v * gelu(g)
    int batch = 1;                 // blockIdx.z; strides in floats
    long long sa0 = 0, sw = 0, sout = 0;
    const void* w16 = nullptr;     // the same packed weights rounded to bf16 (a_bf16 mode)
    int x3 = 0;                    // 1: fp32 products from three bf16 pieces per operand on the bf16 MFMA (igemm_tile_x3); needs w3
    const void* w3 = nullptr;      // three bf16 planes of w ([N][K] each, w3_plane elements apart; batch entries sw apart)
    long long w3_plane = 0;
    // bf16-ACTIVATION mode (bgemm.hip; e2v_set_compute_dtype(E2V_BF16)): a0 / a1 point at bf16 rows (lda in elements), the weights
    // are w16, the product is v_mfma_f32_32x32x16_bf16 with fp32 accumulation.  out is bf16 unless out_f32; resid is bf16 iff
    // resid_bf16 (it is an activation) -- bias and rowbias stay fp32.
    int a_bf16 = 0, out_f32 = 0, resid_bf16 = 0;
    int bm256 = 0;                 // filled by the launcher: 256-row tiles (bgemm256_kernel)
    int ablate = 0;                // timing experiments only (E2V_BGEMM_ABLATE): 1 = no output stores, 2 = A loads read zeros, 3 = both
    int rb1 = 0, w1 = 0, s1 = 0, s2 = 0, nbm = 0, nbm_per = 0, tail_rb = 0;   // filled by the launcher: tile schedule (see igemm_kernel)
    int rb0 = 0, col_off = 0, col_off2 = 0, col_stride = 0, nct_l = 0;   // filled by bgemm256.hip's launcher: first row block / column tiling of a partial launch (tail split)
    // GroupNorm statistics from the PRODUCER (bf16 mode): rbsum != null asks the launch to leave, beside the tensor, the sums a
    // following GroupNorm needs -- rbsum[m / 64][n][2] = (sum, sum of squares) of the STORED (bf16-rounded) outputs of rows
    // 64 b .. 64 b + 63, column n, in the canonical order of rowblock_sums (norm.hip).  Only the staged epilogue of bgemm_t256_kernel
    // writes it (igemm_writes_rbsum says whether a launch will); anything else leaves it untouched and the caller runs
    // rowblock_sums over the tensor instead -- same sums, bit for bit, so that which kernel serves a layer (a function of the
    // batch) never shows in a result.
    float* rbsum = nullptr;
    // Split-K (bgemm.hip: bgemm_splitk_kernel + splitk_reduce_kernel; 16-bit modes, the SMALL-BATCH dispatch family -- the reference
    // generates clip by clip, inference_eeg2video.py:90-100: two UNet samples leave a deep-level 3x3 conv 40 tiles for 256 CUs).
    // sk >= 2 and sk_ws != null: the K range is cut into sk runs of whole 64-channel chunks (each inside one source of a concat), run
    // z = blockIdx.y leaves its fp32 partial tile in sk_ws[z][M][N] and a second kernel adds the runs IN ORDER (run 0 first) and applies
    // the epilogue -- deterministic, but a different summation order than the unsplit kernels: results are equal to theirs up to fp32
    // rounding, not bit for bit (DESIGN: bit-identity across batch sizes holds within a dispatch family).  splitk_plan() sizes it.
    int sk = 0;
    float* sk_ws = nullptr;
    int sk_s0 = 0, sk_q0 = 0, sk_q1 = 0;      // filled by the launcher: runs inside source 0, chunks per run in source 0 / source 1
};
// The split a launch of `a` would take for a request of `want` runs: 0 = none (the launch is not eligible), else the number of runs
// actually used (<= want: whole chunks, every run non-empty); the caller then provides sk_ws of that many [M][N] fp32 planes.
int splitk_plan(const IgemmArgs& a, int want);
// the tile schedule a launch carries (gemm_sched.h), as the kernels decode it
E2V_SCHED_HD inline TileSched tile_sched(const IgemmArgs& p) { return TileSched{p.nbm, p.w1, p.s1, p.s2, p.tail_rb}; }
// Profile name and algorithmic flops / bytes of a GEMM launch, for its ProfScope: `cls` (null: the class of the launch's 16-bit type,
// "igemm_bf16" / "igemm_fp16") + (detailed profiles and dry runs) the shape tags " M.. N.. K.. t.. s2 up cat geglu b.." + `suffix`.
// in_b / w_b / out_b: bytes per activation, weight and output element; `terse` leaves out the taps / stride / resize / concat tags
// (the f32x3 launches never carried them).
struct GemmProf {
    std::string name;
    double flops, bytes;
};
GemmProf gemm_prof(const char* cls, const IgemmArgs& a, double in_b, double w_b, double out_b, const std::string& suffix = "", bool terse = false);
void igemm(const IgemmArgs& a, hipStream_t s);
bool igemm_writes_rbsum(const IgemmArgs& a);       // will igemm(a) fill a.rbsum?  (same rules as the launch itself)
// rows per lane pass of the canonical order: the staged epilogue of a 256 x 320 tile finishes 6 rows per pass, of a 256 x 256 tile 8
inline int rbsum_rows_per_pass(int N) { return N % 320 == 0 ? 6 : 8; }
// could a tensor [M][N] carry row-block sums at all (a property of the layer, never of the batch)?
inline bool rbsum_capable(long long M, int N) { return M % 64 == 0 && (N % 320 == 0 || N % 256 == 0); }
// Run-time switches: an int per name, initialised from the environment variable of that name on first use
// and settable through e2v_op_set_knob for A/B comparisons inside one process.  The returned pointer stays valid.
int* knob(const char* name, int dflt);
bool set_knob(const char* name, int value);
// Switches of variants that were MEASURED AND NOT ADOPTED (or are kept only as the other arm of a same-process A/B) exist in an
// `make AB=1` build (-DE2V_AB) only: the shipped library carries neither their kernels nor their switches (set_knob refuses the
// names, the environment variables are not read), and the launch rules read the default.
template <int V> inline const int* ab_const() { static const int v = V; return &v; }
#ifdef E2V_AB
#define E2V_AB_KNOB(name, dflt) ::e2v::knob(name, dflt)
#else
#define E2V_AB_KNOB(name, dflt) ::e2v::ab_const<dflt>()
#endif      // false: no kernel has asked for a knob of that name yet and it is not a known one
void bgemm_launch(const IgemmArgs& a, int ntiles, hipStream_t s);
void bgemm_splitk_launch(const IgemmArgs& a, hipStream_t s);            // the split-K form (a.sk, a.sk_ws; schedule filled by igemm())
bool bgemm_all_n64(const IgemmArgs& a);
bool bgemm_t256_writes_rbsum(const IgemmArgs& a);                         // bgemm256.hip: would that launch fill a.rbsum?
bool bgemm_t256_launch(const IgemmArgs& a, hipStream_t s);                 // bgemm256.hip: true = the layer was eligible and has been launched
// Exact 2x nearest resize in front of a stride-1, pad-1 3x3 conv as four 2x2 convs on the SOURCE map (one per output parity; weights
// summed over the taps that read the same source pixel: 4 / 9 of the multiplies).  `g` describes the conv as igemm() takes it.
bool bgemm_up2x_applies(const IgemmArgs& g);
int conv_up2x_packed_ld(int cin);                                        // row length of one parity's [O][chunk64][4 taps][64] layout
void pack_conv_up2x(const float* w_oihw, float* w_packed, int cout, int cin, hipStream_t s);    // [4 parities][O][ld], fp32
void bgemm_up2x_launch(const IgemmArgs& g, const void* w16_up2, hipStream_t s);                // w16_up2: the packed layout as bf16
bool bgemm_use_256(const IgemmArgs& a);                                  // schedule hint: 256-row tiles pay for this launch

// weight re-layout helpers (one-off, at finalize)
// [O][I][3][3] -> [O][ceil(I/bke)][9][bke] (bke = 32 for the fp32 kernel, 64 for the bf16 one); row length below
int conv3x3_packed_ld(int cin, int bke);
void pack_conv3x3(const float* w_oihw, float* w_packed, int cout, int cin, int bke, hipStream_t s);
void copy_rows(const float* src, int ld_src, float* dst, int ld_dst, int rows, int cols, hipStream_t s);
void to_bf16(const float* in, void* out_bf16, size_t n, hipStream_t s);
void to_h16(const float* in, void* out16, size_t n, int mode, hipStream_t s);      // mode: 1 bf16 / 2 fp16 (h16.h), round to nearest even
void split_bf16x3(const float* in, void* out_planes, size_t n, size_t plane_stride, hipStream_t s);   // exact 3-way truncation split

// ---------------------------------------------------------------------------------------
// Winograd F(2x2, 3x3) for the stride-1, pad-1 3x3 convolutions (wino.hip); output map = logical input map
// ---------------------------------------------------------------------------------------
struct WinoArgs {
    const float* x0 = nullptr; const float* x1 = nullptr;      // channel-last sources (x1: concatenated skip)
    int c0 = 0, c1 = 0, ld0 = 0, ld1 = 0;
    int nimg = 0, Hs = 1, Ws = 1;                              // physical source map
    int Ho = 1, Wo = 1;                                        // output map (= source map, or 2x with upsample)
    int upsample = 0; float ups_h = 1.f, ups_w = 1.f;
    const float* gn_scsh = nullptr; int gn_P = 1; int gn_silu = 0;   // fused GroupNorm affine (+ SiLU) on the way in
    int m = 2;                                                 // output tile: 2 = F(2x2,3x3), 4 = F(4x4,3x3)
    const float* U = nullptr;                                  // [(m+2)^2][N][c0+c1] (wino_pack_weights)
    const void* U3 = nullptr;                                  // its three-plane bf16 split (f32x3 mode), planes (m+2)^2*N*C apart
    int N = 0;
    float* out = nullptr; int ldc = 0;
    const float* bias = nullptr;
    const float* rowbias = nullptr; int rb_ld = 0; int rows_per_sample = 1;
    const float* resid = nullptr; int ldr = 0;
};
void wino_pack_weights(const float* w_oihw, float* U, int cout, int cin, int m, hipStream_t s);
size_t wino_workspace_floats(const WinoArgs& a, int nimg);       // V + M for `nimg` images
int wino_chunk_images(const WinoArgs& a, size_t max_floats);     // images per pass so that the workspace fits
void wino_conv3x3(const WinoArgs& a, float* workspace, int chunk_images, hipStream_t s);

// ---------------------------------------------------------------------------------------
// normalisation (norm.hip)
// ---------------------------------------------------------------------------------------
// GroupNorm over `samples` slabs of P rows.  Statistics are taken over (C/groups) channels x P rows
// (5-D GroupNorm of ResnetBlock3D: P = F*H*W, resnet.py:177; per-frame GroupNorm of
// Transformer3DModel: samples = n*F, P = H*W, attention.py:93,99).  Two sources = channel concat.
struct GroupNormArgs {
    const float* x0 = nullptr; const float* x1 = nullptr;
    int c0 = 0, c1 = 0, ld0 = 0, ld1 = 0;
    const float* gamma = nullptr; const float* beta = nullptr;   // [c0+c1]
    float* out = nullptr; int ldo = 0;                           // [samples*P][c0+c1]
    int samples = 0, P = 0, groups = 32;
    float eps = 1e-5f; int silu = 0;
    int bf16 = 0;                  // 1: x0 / x1 / out are bf16 (statistics, scale / shift and the arithmetic stay fp32)
    float* ws_part = nullptr;      // workspace: samples*chunks*(c0+c1)*2 floats
    float* ws_scale = nullptr;     // workspace: samples*(c0+c1)*2 floats
    // row-block sums that came with a source tensor (IgemmArgs::rbsum / rowblock_sums: [rows / 64][c_i][2]): the statistics pass
    // over that source is skipped and the fold reads them (needs P % 64 == 0; bf16 mode)
    const float* rb0 = nullptr; const float* rb1 = nullptr;
    // small-batch dispatch family (16-bit modes): where a (sample, group) slice fits LDS, ONE kernel reads it once, folds and applies
    // (gn_fused_small_kernel) instead of the three launches -- another summation order, so the family picks it, never the batch
    int fused_small = 0;
    int small_chunks = 0;          // the family's 64-row statistics / apply chunks at every level (two samples: 108 chunks of 256 rows for 256 CUs)
};
// the canonical row-block sums of a stored bf16 tensor x[rows][C] (rows % 64 == 0): out[rows / 64][C][2], bit-identical to what the
// staged epilogue of bgemm_t256_kernel leaves for a tensor of the same width (rpp = rbsum_rows_per_pass(C))
void rowblock_sums(const void* x_bf16, int ld, int C, long long rows, int rpp, float* out, hipStream_t s);
int  groupnorm_chunks(int P);
void groupnorm(const GroupNormArgs& a, hipStream_t s);
// statistics only: leaves per-(slab, channel) (scale, shift) pairs in a.ws_scale for a consumer that applies the affine
// (+ SiLU) itself while it reads the tensor anyway (the Winograd input transform)
void groupnorm_stats(const GroupNormArgs& a, hipStream_t s);
void layernorm(const float* x, int ldx, const float* gamma, const float* beta, float* out, int ldo,
               int rows, int C, float eps, hipStream_t s, int bf16 = 0);      // bf16: x / out are bf16 rows
// x16: bf16 / fp16 rows (h16: 1 / 2), out: fp32 rows -- the LayerNorm in front of a metric tower's head in 16-bit mode (the strided
// class rows, or the pooled rows).  fp32 statistics, the result is not rounded.  C a multiple of 4 up to 1280.
void layernorm_f32_out(const void* x16, int ldx, const float* gamma, const float* beta, float* out, int ldo, int rows, int C, float eps,
                       hipStream_t s, int h16);

// ---------------------------------------------------------------------------------------
// attention (attn.hip)
// ---------------------------------------------------------------------------------------
struct AttnArgs {
    const float* q = nullptr; int ldq = 0;
    const float* k = nullptr; const float* v = nullptr; int ldkv = 0;
    float* o = nullptr; int ldo = 0;
    int n = 0, F = 1, heads = 8, D = 40;
    int Nq = 0, Nk = 0;
    int mode = 0;      // 0: sparse-causal self-attention, keys = [frame 0 ; frame max(f-1,0)] (attention.py:292-301)
                       // 1: keys shared by all frames of a sample (cross-attention to the 77 cond tokens)
    float scale = 1.f;
    int x3 = 0;        // 1: fp32-equivalent QK^T and PV from exactly split bf16 pieces (six MFMAs per product, f32x3 mode)
    int io_bf16 = 0;   // 1: q / k / v / o are bf16 rows (strides in elements, multiples of 8); implies the bf16 MFMA
};
void flash_attention(const AttnArgs& a, hipStream_t s);      // throws Error(E2V_EINVAL) for a head dim without a kernel instance
bool flash_attention_supports(int D);
// attn_q64.hip: bf16 sparse-causal attention with 64 queries per wave (head dims 40 / 80).  _waves: waves per workgroup of the instance
// that would serve the call, 0 = not served (flash_attention falls back to flash_attn_b16io_kernel); the second launches it.
std::string attn_shape_tag(const AttnArgs& a);                // " D.. Nq.. Nk.. n.. F.. h.." for profile names
int flash_attention_q64_waves(const AttnArgs& a);
bool flash_attention_q64(const AttnArgs& a, hipStream_t s);
// temporal self-attention over the F frames of every pixel (attention.py:261-267), qkv = [n*F*HW][3C]
void temporal_attention(const float* qkv, int ld, float* out, int ldo, int n, int F, int HW, int heads, int D,
                        float scale, hipStream_t s, int bf16 = 0);          // bf16: qkv / out are bf16 rows
// in place (VAE attention); out_bf16 != null: the normalised probabilities are written there as bf16 ([rows][ld]) instead
void softmax_rows(float* x, int ld, int rows, int cols, hipStream_t s, void* out_bf16 = nullptr, int out_mode = 1);   // out_mode: 1 bf16 / 2 fp16

// ---------------------------------------------------------------------------------------
// CLIP text encoder (text.hip): fp32 in every compute mode
// ---------------------------------------------------------------------------------------
// out[row][:] = tok[ids[row]][:] + pos[row % T][:]  (ids: device int32, already range-checked on the host; C a multiple of 4)
void text_embed(const int* ids, const float* tok, const float* pos, float* out, int rows, int T, int C, hipStream_t s);
// causal self-attention over each of B prompts of T tokens, head dim 64, scale 64^-0.5: qkv [B*T][ldqkv] holds q | k | v of
// heads * 64 columns each, out [B*T][ldo].  K and V of a head live in LDS, which bounds T:
constexpr int kTextAttnMaxT = 128;      // 2 x 128 rows x 272 bytes = 68 KiB of the CU's 160; two keys per lane
void text_causal_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s);
// in place: act 0 = quick-GELU x sigmoid(1.702 x), 1 = erf GELU; count a multiple of 4
// h16 = 1 / 2: x is bf16 / fp16 storage (count a multiple of 8): widened, the activation in fp32, rounded once at the store
void text_activation(float* x, long long count, int act, hipStream_t s, int h16 = 0);

// ---------------------------------------------------------------------------------------
// ViT image classifier (vit.hip; e2v_image_classify): fp32 whatever the context's mode.  LayerNorm, the linears and the GELU are
// norm.hip's, igemm.hip's and text.hip's; the preprocess and the token rows are video.hip's (below).
// ---------------------------------------------------------------------------------------
struct FrameSrc;                            // (below: the input description e2v_frame_metrics shares)
// One axis of Pillow's antialiased resize as a table (host arithmetic; e2v_image_resize_table, e2v_image_resize_table_filter).
// The filter in Pillow's codes: 2 BILINEAR (the triangle, support 1), 3 BICUBIC (a = -0.5, support 2: negative coefficients).
constexpr int kResizeBilinear = 2, kResizeBicubic = 3;
struct ResizeAxis {
    int in = 0, out = 0, ksize = 0;
    std::vector<int> first, count;          // [out]
    std::vector<int> coeff;                 // [out][ksize], 22-bit fixed point
};
ResizeAxis resize_axis(int in_size, int out_size, int filter = kResizeBilinear);
// non-causal self-attention over each of B images of T tokens, head dim 64, scale 64^-0.5; layouts as text_causal_attention.
// K and V of an (image, head) live in LDS at the 68-float stride, which bounds T:
constexpr int kImageAttnMaxT = 288;     // 2 x 288 rows x 272 bytes = 153 KiB of the CU's 160; up to five keys per lane
void image_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s);
// one wave per image over logits [nimg][ld] (L <= ld columns used): logits_out [nimg][L] (copy), probs = softmax(logits), top3 = the
// three largest by (value, index) in ascending order; any of the three may be null.  L >= 3.
void image_head(const float* logits, int ld, int L, int nimg, float* logits_out, float* probs, int* top3, hipStream_t s);

// ---------------------------------------------------------------------------------------
// VideoMAE video classifier (video.hip; e2v_video_classify): fp32 whatever the context's mode; `h16` as above.  The encoder layers are the image
// classifier's; the head's softmax / top 3 is image_head.
// ---------------------------------------------------------------------------------------
// The frame preprocess of the three towers (Pillow's antialiased resize, of which only a window is computed, fused with the pixel
// table and the patch layout) and their token rows.
// A resize target (nh, nw) and the S x S window of it that is kept, from (top, left)
struct PrepWindow { int nh = 0, nw = 0, top = 0, left = 0; };
// VideoMAEImageProcessor's geometry (the CLIP processor's too): the shortest edge resized to `edge` with the aspect ratio kept, then
// the centre crop of S x S
PrepWindow video_crop(int H, int W, int edge, int S);
// The tables of the (H, W) -> (nh, nw) resize restricted to the window and the pixel table, as the preprocess kernel reads them: one
// block of 32-bit words, [hfirst S | hcount S | vfirst S | vcount S | hcoeff S * kh | vcoeff S * kv | lut 3 * 256 floats] (`first` in
// source coordinates), and the source columns [c0, c0 + cw) the window's horizontal taps read (the vertical-first order keeps only those)
struct PrepPlan {
    int H = 0, W = 0, S = 0, kh = 0, kv = 0;
    bool vfirst = false;                    // Pillow resizes an image more than 100 times as tall as wide vertically first
    int band = 0, band_rows = 0;            // output rows per workgroup and the most source rows such a band reads (0: does not fit)
    int c0 = 0, cw = 0;
    std::vector<int> words;
};
constexpr int kImagePrepLdsBytes = 48 * 1024;     // the band of resized rows a workgroup keeps
// `filter`: the processor's resample code.  The image classifier's processor: win = {S, S, 0, 0}, bilinear; the video classifier's
// and CLIP's: video_crop(H, W, edge, S), bilinear / the config's.
PrepPlan prep_plan(int H, int W, const PrepWindow& win, int S, int P, const float* lut768, int filter);
// frames img0 .. img0 + nimg - 1 of `src` (FrameSrc: fp32 quantised at load or bytes, planar [n,3,F,H,W] or channels-last [n,F,H,W,3],
// frames of plan.H x plan.W) -> rows [(nimg/ts)*(S/P)^2][3*ts*P*P]: frame ts*t + dt of a clip writes columns ((c*ts + dt)*P + y)*P + x
// of token rows (t, py, px).  ts >= 1 divides F, img0 and nimg (whole tubelets; at ts = 1 every frame is an image of its own and a range
// may start and end inside a clip), nimg <= 65535.  `plan_dev`: plan.words on the device; `name`: the profile class.
// h16 = 1 / 2: `rows` is bf16 / fp16 storage -- the pixel table's fp32 value rounded once at the store (the integer arithmetic in
// front of the table is the same)
void frame_preprocess(const FrameSrc& src, int n, int F, int ts, long long img0, int nimg, const PrepPlan& plan, const int* plan_dev, int P,
                      float* rows, const char* name, hipStream_t s, int h16 = 0);
// x[b*T + t][:] = (cls ? (t == 0 ? cls : patches[b*(T - 1) + t - 1]) : patches[b*T + t])[:] + pos[t][:]   (C a multiple of 4)
// h16 = 1 / 2: patches and x are bf16 / fp16 rows (cls and pos stay fp32; fp32 sum, one rounding at the store).  Profile class:
// image_embed with a class row, video_embed without.
void token_embed(const float* patches, const float* cls, const float* pos, float* x, int B, int T, int C, hipStream_t s, int h16 = 0);
// non-causal self-attention over each of B sequences of T tokens (any T >= 1), head dim 64, scale 64^-0.5; q | k | v in one row matrix
// as image_attention takes them (16-byte aligned rows, strides multiples of 4).  K and V are read per key tile, never resident.
void token_attention(const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, hipStream_t s);
// out[b][:] = (sum over t of x[b*T + t][:], t ascending) / T   (x rows of C columns, contiguous)
// h16 = 1 / 2: x is bf16 / fp16 rows, widened exactly; the sum, its order and the fp32 output are the same
void token_mean(const float* x, float* out, int B, int T, int C, hipStream_t s, int h16 = 0);

// ---------------------------------------------------------------------------------------
// CLIP vision tower and CLIP score (clip.hip; e2v_clip_embed, e2v_clip_similarity): the similarity is fp32 always, the tower as the classifiers.  The processor is
// frame_preprocess at ts = 1 over a bicubic plan (every frame its own image: rows [images * patches][3 P P]); the token rows, the
// attention and the layers are the image classifier's.
// ---------------------------------------------------------------------------------------
// torch.nn.functional.cosine_similarity(a, b, dim=-1, eps): dot(a, b) / (max(|a|, eps) * max(|b|, eps)).  a [na][D], b [nb][D],
// contiguous, 16-byte aligned, D a multiple of 4.  matrix = false: na == nb, out[i] = cos(a[i], b[i]); true: out[i][j] = cos(a[i],
// b[j]).  Every output runs the same sums in the same order (four strided partial sums over d ascending, joined at the end: a
// function of D alone), so out[i][j] of the matrix form carries the bits of the pair form on (a[i], b[j]).
void clip_similarity(const float* a, int na, const float* b, int nb, int D, bool matrix, float eps, float* out, hipStream_t s);

// ---------------------------------------------------------------------------------------
// Seq2Seq latent model (seq2seq.hip; e2v_seq2seq_latents): fp32 in every compute mode.  The linears, LayerNorm, the positions, the mean
// over the window rows and the appended rows are igemm, layernorm, token_embed, token_mean and copy_rows.
// ---------------------------------------------------------------------------------------
// Where the EEGNet kernel keeps things, in floats (every offset a multiple of 4): the pack of folded weights -- w1 [F1][64], w2 [FD][C],
// a2 / c2 [FD], w3 [FD][16], w4 [F2][FD], a3 / c3 [F2], offsets relative to `pack` -- and, behind it in LDS, the window xs [C][T], the
// spatial mixes zp [FD][T + 63], the pooled block-2 rows pp [FD][T/4 + 15], the depthwise rows dw [FD][T/4], block 3 before its pool
// qe [F2][T/4]
struct EegnetLayout {
    int w1, w2, a2, c2, w3, w4, a3, c3, pack_floats;
    int pack, xs, zp, pp, dw, qe;
    size_t total_floats;
};
E2V_SCHED_HD inline EegnetLayout eegnet_layout(int C, int T, int F1, int D, int F2) {
    const int FD = F1 * D, T4 = T / 4;
    auto up4 = [](long long v) { return (v + 3) / 4 * 4; };
    EegnetLayout L;
    long long o = 0;
    L.w1 = (int)o; o = up4(o + (long long)F1 * 64);
    L.w2 = (int)o; o = up4(o + (long long)FD * C);
    L.a2 = (int)o; o = up4(o + FD);
    L.c2 = (int)o; o = up4(o + FD);
    L.w3 = (int)o; o = up4(o + (long long)FD * 16);
    L.w4 = (int)o; o = up4(o + (long long)F2 * FD);
    L.a3 = (int)o; o = up4(o + F2);
    L.c3 = (int)o; o = up4(o + F2);
    L.pack_floats = (int)o;
    L.pack = 0;
    L.xs = (int)o; o = up4(o + (long long)C * T);
    L.zp = (int)o; o = up4(o + (long long)FD * (T + 63));
    L.pp = (int)o; o = up4(o + (long long)FD * (T4 + 15));
    L.dw = (int)o; o = up4(o + (long long)FD * T4);
    L.qe = (int)o; o = up4(o + (long long)F2 * T4);
    L.total_floats = (size_t)o;
    return L;
}
constexpr int kEegnetMaxLdsBytes = 156 * 1024;      // of the CU's 160 KiB; the reference's window (62 x 100, F1 16, D 4, F2 16) takes 111 KiB
// the torch-layout tensors of MyEEGNet_embedding on the HOST: block_1.1 [F1][1][1][64], block_2.0 [F1 D][1][C][1], block_3.1 [F1 D][1][1][16],
// block_3.2 [F2][F1 D][1][1], and each BatchNorm as weight | bias | running_mean | running_var, n values each
struct EegnetHostW { const float* w1; const float* bn1; const float* w2; const float* bn2; const float* w3; const float* w4; const float* bn3; };
std::vector<float> eegnet_pack(const EegnetHostW& h, int C, int F1, int D, int F2, float bn_eps);      // eegnet_layout(...).pack_floats floats
// One workgroup per (clip, window): out[(b W + w)][F2 ((T / 4) / 8)], the flattened block-3 output.  Sample t of channel c of window w
// of clip b is eeg[b clip_stride + w window_stride + c channel_stride + t] (element strides; 4-byte alignment is all a load assumes);
// mean / scale [W][C][T]: the optional input scaler (x - mean) / scale, both or neither.
struct EegnetArgs {
    const float* eeg = nullptr; long long clip_stride = 0, window_stride = 0, channel_stride = 0;
    const float* mean = nullptr; const float* scale = nullptr;
    const float* pack = nullptr;                 // eegnet_pack, on the device
    float* out = nullptr;
    int B = 0, W = 0, C = 0, T = 0, F1 = 0, D = 0, F2 = 0;
};
void eegnet_embed(const EegnetArgs& a, hipStream_t s);
// softmax(q k^T scale) v for the few tokens the model holds: Nq queries of every (clip, head) against Nk <= 32 keys.  Row i of clip b
// of q is q[b sq + i ldq + head D ..] (k, v: skv / ldkv; o: so / ldo; element strides, q and k rows 16-byte aligned with strides
// multiples of 4), D a multiple of 4 up to 128.  causal: query i sits at absolute position q_pos0 + i and sees keys 0 .. q_pos0 + i.
// fp32 softmax, sums in key order.
constexpr int kSeqAttnMaxKeys = 32;
struct SeqAttnArgs {
    const float* q = nullptr; long long sq = 0; int ldq = 0;
    const float* k = nullptr; const float* v = nullptr; long long skv = 0; int ldkv = 0;
    float* o = nullptr; long long so = 0; int ldo = 0;
    int B = 0, heads = 0, D = 0, Nq = 0, Nk = 0, q_pos0 = 0, causal = 0;
    float scale = 1.f;
};
void seq_attention(const SeqAttnArgs& a, hipStream_t s);
// [B][F][C][HW] -> [B][C][F][HW] (HW a multiple of 4, 16-byte aligned)
void seq_latents_bcfhw(const float* in, float* out, int B, int F, int C, int HW, hipStream_t s);

// ---------------------------------------------------------------------------------------
// EEG front end (eeg.hip; e2v_eeg_de_psd): the reference's DE_PSD of every (clip, window, electrode) row, fp32 in every compute mode.
// ---------------------------------------------------------------------------------------
constexpr int kDePsdN = 200;                         // the transform length, STFTN of DE_PSD.py:27, whatever the row length
constexpr int kDePsdBands = 5;                       // delta, theta, alpha, beta, gamma
constexpr int kDePsdThreads = 128;                   // one thread per bin of the half spectrum (at most 100)
constexpr int kDePsdPlanFloats = 3 * kDePsdN;        // the Hann row [200] | cos, sin (2 pi j / 200) interleaved [200][2]
std::vector<float> de_psd_plan(int m);               // of rows of m samples: host arithmetic in double, rounded once
// first[p] .. last[p], the bins band p sums at sampling rate fs (the reference's arithmetic); false: outside bins 0 .. 99
bool de_psd_bands(int fs, int* first, int* last);
// One workgroup per row: de / psd [B][W][C][5] (either may be null).  Sample t of electrode c of window w of clip b is eeg[b clip_stride +
// w window_stride + c channel_stride + t] (element strides; 4-byte alignment is all a load assumes); n = min(samples, 200) of them are
// read.  bins = the largest last[] + 1.  de_mean / de_scale [C][5]: the optional scaler (de - mean) / scale, both or neither.
struct DePsdArgs {
    const float* eeg = nullptr; long long clip_stride = 0, window_stride = 0, channel_stride = 0;
    const float* plan = nullptr;                     // de_psd_plan, on the device
    const float* de_mean = nullptr; const float* de_scale = nullptr;
    float* de = nullptr; float* psd = nullptr;
    int B = 0, W = 0, C = 0, n = 0, bins = 0;
    int first[kDePsdBands] = {}, last[kDePsdBands] = {};
};
void eeg_de_psd(const DePsdArgs& a, hipStream_t s);
// shallownet (EEG2Video/models/models.py:105-123) up to the flatten, its two convolutions and the BatchNorm folded into one filter:
// one workgroup per (clip, kShallowGroup output filters); the clip [C][T] and the group's columns [kShallowGroup][T - K + 1] in LDS
constexpr int kShallowGroup = 4;
constexpr int kShallowThreads = 256;
constexpr int kShallowMaxLdsBytes = 156 * 1024;      // of the CU's 160 KiB; the reference's clip (62 x 200) with its columns takes 52 KiB
E2V_SCHED_HD inline int shallownet_columns(int T, int K, int P, int S) { const int tc = T - K + 1; return tc >= P ? (tc - P) / S + 1 : 0; }
E2V_SCHED_HD inline size_t shallownet_lds_bytes(int C, int T, int K) {
    return ((((size_t)C * T + 3) / 4) * 4 + (size_t)kShallowGroup * (T - K + 1)) * sizeof(float);
}
// the torch-layout tensors of one shallownet on the HOST: net.0 [F][1][1][K] + bias, net.1 [F][F][C][1] + bias, net.2 as weight | bias |
// running_mean | running_var, F values each
struct ShallowHostW { const float* w1; const float* b1; const float* w2; const float* b2; const float* bn; };
// w [groups][C K][kShallowGroup] | c [groups kShallowGroup] (groups = ceil(F / kShallowGroup), zeros past F); shallownet_fold_floats of them
std::vector<float> shallownet_fold(const ShallowHostW& h, int C, int F, int K, float bn_eps);
inline size_t shallownet_fold_floats(int C, int F, int K) { return (size_t)((F + kShallowGroup - 1) / kShallowGroup) * kShallowGroup * ((size_t)C * K + 1); }
// Sample t of electrode c of clip b is eeg[b clip_stride + c channel_stride + t] (element strides; 4-byte alignment is all a load
// assumes) -- the occipital net starts `first` electrodes into the same clip.  mean / scale [C][T]: the optional input scaler
// (x - mean) / scale, both or neither.  out[b ldo + f cols + j]: the pooled maps in the reference's flatten order.
struct ShallowArgs {
    const float* eeg = nullptr; long long clip_stride = 0, channel_stride = 0;
    const float* mean = nullptr; const float* scale = nullptr;
    const float* w = nullptr; const float* c = nullptr;      // shallownet_fold, on the device (16-byte aligned): its filters, its constants
    float* out = nullptr; int ldo = 0;
    int B = 0, C = 0, T = 0, F = 0, K = 0, P = 0, S = 0;
};
void shallownet(const ShallowArgs& a, hipStream_t s);
// head [B][ldh] (L of its columns are logits), feat [B][E2] -> logits [B][L], features [B][E2], labels [B] (int32: argmax, the lowest
// index among equal maxima); any of the three may be null
void glm_outputs(const float* head, int ldh, const float* feat, int E2, int L, int B, float* logits, float* features, int* labels, hipStream_t s);

// ---------------------------------------------------------------------------------------
// element-wise / layout (misc.hip)
// ---------------------------------------------------------------------------------------
void ncfhw_to_cl(const float* in, float* out, int n, int C, int Cpad, int FHW, float scale, hipStream_t s, int out_bf16 = 0);
void cl_to_ncfhw(const float* in, int ld, float* out, int n, int C, int FHW, float mul, float add, int clamp, float lo,
                 float hi, hipStream_t s);
void nchw_frames_to_ncfhw(const float* in, int ld, float* out, int n, int F, int C, int HW, float mul, float add,
                          int clamp01, hipStream_t s);
void timestep_sinusoid(const long long* t, int nt, float* out, int n, int dim, int flip_sin_to_cos, float freq_shift,
                       hipStream_t s, int t_is_f32 = 0);      // t_is_f32: `t` points at nt floats instead
void silu(const float* in, float* out, long long count, hipStream_t s);
void transpose2d(const float* in, int ld_in, float* out, int ld_out, int rows, int cols, int batch,
                 long long sb_in, long long sb_out, hipStream_t s, int bf16 = 0);
// eps = eps_u + g (eps_c - eps_u); DDIM eta = 0 update (pipeline_tuneeeg2video.py:320-325)
void ddim_cfg_step(const float* eps_u, const float* eps_c, const float* x, float* x_out, long long count,
                   float guidance, float sqrt_a_t, float sqrt_1m_a_t, float sqrt_a_p, float sqrt_1m_a_p,
                   hipStream_t s);

// out = sum_{i<n} coefs[i] xs[i] (n <= 5) / out = eu + g (ec - eu): schedulers other than DDIM (PNDM) and the guidance line
void lincomb(int n, const float* const* xs, const float* coefs, float* out, long long count, hipStream_t s);
void cfg_combine(const float* eu, const float* ec, float g, float* out, long long count, hipStream_t s);

// (f) rows -------------------------------------------------------------------------------------------
// DANA noise (EEG2Video/models/DANA_module.py:52-72) fused with the caller's layout fix 'a b c d e -> a c b d e'
// (inference_eeg2video.py:77,82): x0, eps_div [B,F,C,HW], eps_same [B,1,C,HW] -> out [B,C,F,HW];
// coef [B][2] = (sqrt(abar_t), sqrt(1 - abar_t)) per clip (device).
void dana_noise(const float* x0, const float* eps_div, const float* eps_same, const float* coef, float sqrt_1m_beta,
                float sqrt_beta, float* out, int B, int F, int C, int HW, hipStream_t s);
// (x * 255) truncated to uint8, as save_videos_grid does (tuneavideo/util.py:29)
void frames_to_u8(const float* in, unsigned char* out, long long count, hipStream_t s);
void pad_cols(const float* in, int cols, float* out, int cols_pad, long long rows, hipStream_t s, int out_bf16 = 0);   // fp32 in; out fp32 or bf16

// Frame metrics (metrics.hip; e2v_frame_metrics): per-image SSIM (skimage's defaults at data_range = 255, exact integer window moments)
// and MSE of two clips of n * F images with C channels.  Each input is fp32 in [0,1] (quantised to bytes once, at load) or uint8, planar
// [n,C,F,H,W] or channels-last [n,F,H,W,C], of any alignment its type allows.  One workgroup scores kCols x kRows window positions of
// one image and leaves one partial in `partials` (frame_metrics_partials_bytes, caller-owned); a second kernel sums them per image in
// index order into ssim / mse [n * F] (either may be null).  H, W >= 7, 1 <= C <= 4, n * F * frame_metrics_tiles(H, W) < 2^31.
struct FrameMetricsTile { static constexpr int kCols = 256, kRows = 32; };
struct FrameSrc { const void* p = nullptr; int f32 = 0; int channels_last = 0; };
long long frame_metrics_tiles(int H, int W);
size_t frame_metrics_partials_bytes(int n, int F, int H, int W);
void frame_metrics(const FrameSrc& a, const FrameSrc& b, int n, int F, int C, int H, int W, void* partials, float* ssim, float* mse,
                   hipStream_t s);

// In-place weight update (e2v_update_tensor): one pass over a [rows][in] source (fp32, bf16 or fp16; src_mode as the h16.h flags:
// 0 / 1 / 2) that writes every form a finalized linear keeps of it -- the fp32 matrix, the bf16 and fp16 copies (rows zero-padded
// to ld16, a multiple of 8) and the three f32x3 planes -- with the roundings of to_h16 / split_bf16x3, so the bits equal a fresh
// finalize.  A null destination is skipped.  Source row j lands in row  row_off + j  of each destination (half == 0), or, for the
// GEGLU interleave (half > 0: rows [value 0..half) | gate 0..half)] -> blocks of [blk value | blk gate]), in row
// row_off + 2 blk (jj / blk) + jj % blk + (j >= half ? blk : 0)  with jj = j % half.  Columns in .. ld - 1 of a destination row are zeros.
struct WeightScatterArgs {
    const void* src = nullptr; int src_mode = 0;
    int rows = 0, in = 0;
    int row_off = 0, half = 0, blk = 1;
    float* d32 = nullptr; int ld32 = 0;
    void* d16b = nullptr; void* d16h = nullptr; int ld16 = 0;
    void* d3 = nullptr; int ld3 = 0; long long plane = 0;        // planes `plane` elements apart
};
void weight_scatter(const WeightScatterArgs& a, hipStream_t s);

// Weight read-back (e2v_read_tensor): the inverse of weight_scatter over the same row map.  ONE stored form of a linear is the source --
// fp32 (src_mode 0), the bf16 or fp16 copy (1 / 2), or the three f32x3 planes (x3 = 1: `src` is plane 0, the others `plane` elements
// on; the value is (p0 + p1) + p2 in fp32, which is the fp32 weight exactly) -- with row stride `ld` elements, of which the first
// `in` columns are the tensor's.  Destination row j, dense [rows][in] in dst_mode's type (0 fp32, 1 bf16, 2 fp16: round to nearest
// even, as to_h16), comes from source row  row_off + j  (half == 0) or from the GEGLU-interleaved row WeightScatterArgs describes.
// Nothing is read past column `in` of a source row and exactly rows * in destination elements are written; `dst` may have any alignment.
struct WeightGatherArgs {
    const void* src = nullptr; int src_mode = 0; int x3 = 0;
    int ld = 0; long long plane = 0;
    int rows = 0, in = 0;
    int row_off = 0, half = 0, blk = 1;
    void* dst = nullptr; int dst_mode = 0;
};
void weight_gather(const WeightGatherArgs& a, hipStream_t s);

// weight-streaming GEMV (gemv.hip): out[b][n] = act(x[b] . W[n] + bias[n]) for B <= 16 rows, x / out fp32 rows, W [N][ldw] fp32 or
// bf16 (rows zero-padded to ldw); the Semantic Predictor at the reference's batch sizes
bool gemv_rows_supported(int B, int K, int w_bf16);
void gemv_rows(const float* x, int ldx, const void* w, int ldw, int w_bf16, const float* bias, float* out, int ldo, int B, int N, int K,
               int relu, hipStream_t s);

// strided row copy between storage types (fp32 <-> bf16), zero-filling columns cols .. cols_out-1 of the output
void cvt_rows(const void* in, int ld_in, int in_bf16, void* out, int ld_out, int out_bf16, long long rows, int cols, int cols_out,
              hipStream_t s);

}  // namespace e2v
