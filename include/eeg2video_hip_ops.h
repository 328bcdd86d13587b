/* eeg2video_hip_ops.h -- kernel-level entry points of libeeg2video_hip.so.
 *
 * These expose the individual gfx950 kernels behind the model-level ABI of eeg2video_hip.h so that each
 * can be checked against the oracle and profiled on its own.  Activations are CHANNEL-LAST fp32 device
 * tensors: [n, F, H, W, C] is a row-major matrix [n*F*H*W][C].  Weights are device pointers in the
 * torch layouts the reference's modules hold (Conv2d [Cout,Cin,3,3], Linear [out,in]).
 * Reference op each one stands for is named per function (paths relative to the reference repo).
 *
 * In the 16-bit modes e2v_op_linear(_cat) and e2v_op_conv3x3 round their operands to the type and, by default, run the launch with an
 * fp32 output and an fp32 residual.  While the run-time switch "E2V_OP_IO16" (e2v_op_set_knob, or the environment variable; default
 * 0) is non-zero they run the launch the GRAPH makes instead: the output is a 16-bit workspace tensor of exactly M x N, the residual is
 * converted to the type first, and the 16-bit result is widened (exactly) into the caller's fp32 `out`; bias and rowbias stay fp32.
 * The fp32 and f32x3 modes ignore the switch.
 */
#ifndef EEG2VIDEO_HIP_OPS_H
#define EEG2VIDEO_HIP_OPS_H

#include "eeg2video_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* InflatedConv3d 3x3 (EEG2Video/models/resnet.py:10-18) over n_img frames of Hs x Ws, optionally after a
 * nearest resize to (Hi, Wi) (Upsample3D, resnet.py:58-61; Hi = Hs, Wi = Ws: none).  Input = channel concat
 * of x0 (c0) and x1 (c1, may be NULL/0).  Output map (Ho, Wo) = floor((Hi + pad_lo + pad_hi - 3)/stride) + 1
 * with pad_lo rows/cols of zeros above/left (pad_hi is implied by Ho).  Epilogue: + bias[cout]
 * + rowbias[row / rows_per_sample][cout] (time embedding, resnet.py:186) + resid[row][cout]. */
e2v_status e2v_op_conv3x3(e2v_ctx* ctx, const float* x0, int c0, const float* x1, int c1, int n_img, int Hs, int Ws,
                          int Hi, int Wi, int Ho, int Wo, int stride, int pad_lo, const float* w_oihw, const float* bias,
                          int cout, const float* rowbias, int rows_per_sample, const float* resid, float* out,
                          e2v_stream stream);

/* GroupNorm + SiLU + InflatedConv3d 3x3 as ResnetBlock3D runs them (resnet.py:177-180, 188-197) in the fp32 mode: the statistics pass of
 * e2v_op_groupnorm over slabs of gn_P source rows (n_img * Hs * Ws must be a multiple of gn_P), then the Winograd form of e2v_op_conv3x3
 * whose input transform applies the affine and the SiLU while it reads the tensor -- the normalised activation is never stored.  gamma /
 * beta: [c0 + c1].  Exists only where the library picks a Winograd form for the conv (stride 1, pad_lo 1, Ho = Hi, Wo = Wi, fp32
 * arithmetic, channel counts multiples of 4, e2v_set_conv_algo): any other shape is refused with E2V_ESHAPE, as the graph refuses it.
 * The concat seam c0 only has to be a multiple of 4 here (the direct kernels behind e2v_op_conv3x3 need 32; the transforms read quads).
 * That check needs no GPU: a host-only context answers it too (and then E2V_ESTATE for a shape that would run). */
e2v_status e2v_op_conv3x3_gn(e2v_ctx* ctx, const float* x0, int c0, const float* x1, int c1, int n_img, int Hs, int Ws, int Hi, int Wi,
                             int Ho, int Wo, int stride, int pad_lo, int gn_P, int groups, float eps, const float* gamma,
                             const float* beta, const float* w_oihw, const float* bias, int cout, const float* rowbias,
                             int rows_per_sample, const float* resid, float* out, e2v_stream stream);

/* nn.Linear / 1x1 conv: out[M][N] = x[M][K] w[N][K]^T + bias (+ resid).  geglu != 0: w is the GEGLU
 * projection [2*N2][K] in torch row order (value rows then gate rows, attention.py:189 via diffusers GEGLU);
 * out[M][N2] = (x w_v^T + b_v) * gelu_erf(x w_g^T + b_g). */
e2v_status e2v_op_linear(e2v_ctx* ctx, const float* x, int ldx, int64_t M, int K, const float* w, const float* bias,
                         int N, const float* resid, int geglu, float* out, e2v_stream stream);

/* The same with the K columns of a row coming from two tensors, [x0 (c0 columns, row stride ld0) ; x1 (c1, ld1)] -- the 1x1 shortcut of
 * the up-block resnets over the concat [h ; skip] (resnet.py:199-202 after unet_blocks.py's torch.cat), the K loop crossing the seam.
 * w: [N or 2 N][c0 + c1].  x1 = NULL, c1 = 0: e2v_op_linear.  With two sources c0 and c1 are multiples of 4 (16-bit modes: 8) and, in
 * the fp32 modes, so are the row strides: E2V_ESHAPE otherwise (checked before any device work: a host-only context answers too). */
e2v_status e2v_op_linear_cat(e2v_ctx* ctx, const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, int64_t M,
                             const float* w, const float* bias, int N, const float* resid, int geglu, float* out, e2v_stream stream);

/* nn.GroupNorm (+ SiLU) with statistics over (C/groups channels) x (P rows) per slab; slabs = samples.
 * 5-D GroupNorm of ResnetBlock3D (resnet.py:177): samples = n, P = F*H*W.  Per-frame GroupNorm of
 * Transformer3DModel (attention.py:99): samples = n*F, P = H*W. */
e2v_status e2v_op_groupnorm(e2v_ctx* ctx, const float* x0, int c0, const float* x1, int c1, int samples, int P,
                            int groups, float eps, const float* gamma, const float* beta, int silu, float* out,
                            e2v_stream stream);

/* nn.LayerNorm over the last dim (attention.py:167,184,190,202) */
e2v_status e2v_op_layernorm(e2v_ctx* ctx, const float* x, int64_t rows, int C, const float* gamma, const float* beta,
                            float eps, float* out, e2v_stream stream);

/* softmax(q k^T * scale) v per (sample, frame, head).
 * mode 0: SparseCausalAttention (attention.py:272-328): q, k, v are [n*F*Nq][ld]; keys of frame f are
 *         [frame 0 ; frame max(f-1, 0)].  mode 1: keys shared by the F frames of a sample, k, v [n*Nk][ldkv]. */
e2v_status e2v_op_attention(e2v_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldkv, float* o,
                            int ldo, int n, int F, int heads, int D, int Nq, int Nk, int mode, float scale,
                            e2v_stream stream);

/* attn_temp (attention.py:261-267): self-attention over the F frames of every pixel; qkv [n*F*HW][3C]. */
e2v_status e2v_op_temporal_attention(e2v_ctx* ctx, const float* qkv, float* out, int n, int F, int HW, int heads, int D,
                                     float scale, e2v_stream stream);

/* AttentionBlock of the VAE mid block (diffusers 0.11.1) between its qkv linear and its projection, the code e2v_vae_decode and
 * e2v_vae_encode run: per image, scores = q k^T * C^-0.5 (a batched GEMM whose A and W are column slices of the fused rows), a row
 * softmax, V transposed, out = P V (a second batched GEMM).  qkv [nimg*HW][3C]: q | k | v; out [nimg*HW][C].  scores / probs: NULL, or
 * fp32 device tensors [nimg*HW][HW] that receive the scaled scores as the first GEMM left them (fp32 in every mode) and the
 * probabilities as the second GEMM reads them (16-bit modes: the 16-bit copy, widened exactly).  16-bit modes: qkv is rounded once to
 * the type on entry and the 16-bit result widened exactly.  HW a multiple of 4 (16-bit modes: 8), as the graph requires, and so C. */
e2v_status e2v_op_vae_attention_core(e2v_ctx* ctx, const float* qkv, float* out, int nimg, int HW, int C, float* scores, float* probs,
                                     e2v_stream stream);

/* The row softmax of that block on its own, in place: x [rows][ld] fp32, columns 0 .. cols - 1 of every row (ld >= cols; the columns
 * between the rows are neither read nor written).  out_mode 0: x receives the probabilities; out16 NULL.  out_mode 1 (bf16) / 2 (fp16):
 * out16 [rows][ld] (2-byte elements, the same row stride) receives the probabilities rounded once, and x is left holding the
 * exponentials exp(x - max of the row), not normalised.  fp32 arithmetic in every compute mode. */
e2v_status e2v_op_softmax_rows(e2v_ctx* ctx, float* x, int ld, int rows, int cols, void* out16, int out_mode, e2v_stream stream);

/* The transpose of that block on its own: out[b][c][r] = in[b][r][c] for `batch` matrices of rows x cols, sb_in / sb_out elements
 * apart, row strides ld_in >= cols and ld_out >= rows (all in elements).  two_byte != 0: 2-byte elements (bf16 or fp16: one kernel),
 * else 4-byte.  The payload is moved as bits. */
e2v_status e2v_op_transpose2d(e2v_ctx* ctx, const void* in, int ld_in, void* out, int ld_out, int rows, int cols, int batch,
                              int64_t sb_in, int64_t sb_out, int two_byte, e2v_stream stream);

/* CLIPAttention under the causal mask (transformers modeling_clip.py, as e2v_text_encode runs it): self-attention over each of B
 * prompts of T tokens, head dim 64, scale 64^-0.5, query i attends to keys 0 .. i.  qkv [B*T][ldqkv]: q | k | v, heads * 64 columns
 * each (16-byte aligned, ldqkv a multiple of 4); out [B*T][ldo], columns 0 .. heads * 64 - 1 written.  1 <= T <= 128 (E2V_ESHAPE).
 * fp32 in every compute mode. */
e2v_status e2v_op_causal_attention(e2v_ctx* ctx, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads,
                                   e2v_stream stream);

/* One axis of Pillow's antialiased BILINEAR resize (src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc), as
 * e2v_image_classify applies it: output sample xx of out_size reads count[xx] <= *ksize input samples starting at first[xx], with the
 * 22-bit fixed-point weights coeff[xx * *ksize + k] (the rest of a row is zero):
 *   out[xx] = clip8((2^21 + sum_k coeff[xx * ksize + k] * in[first[xx] + k]) >> 22).
 * A two-pass resize applies the table of the width to every row, rounds to bytes, then the table of the height to every column.
 * HOST-ONLY: plain arithmetic, no context, no GPU.  first, count: out_size ints each; coeff: out_size * ksize entries; all three may be
 * NULL to ask for *ksize = 2 * ceil(max(in_size / out_size, 1)) + 1 alone.  E2V_EINVAL for a null ksize or a size below 1. */
e2v_status e2v_image_resize_table(int in_size, int out_size, int* first, int* count, int32_t* coeff, int* ksize);
/* The same with the filter named in Pillow's codes: 2 = BILINEAR (the table above, bit for bit), 3 = BICUBIC (Resample.c's
 * bicubic_filter, a = -0.5, support 2: *ksize = 2 * ceil(2 * max(in_size / out_size, 1)) + 1, coefficients negative in places; an
 * output's sum may leave [0, 255] and is clipped to a byte after the arithmetic >> 22, as Pillow does).  Any other filter: E2V_EINVAL. */
e2v_status e2v_image_resize_table_filter(int in_size, int out_size, int filter, int* first, int* count, int32_t* coeff, int* ksize);

/* The preprocess of e2v_image_classify on its own: n * F images of H x W (frames / kind as there) -> Pillow's bytes at S x S -> the
 * patch-row matrix rows [n*F*(S/P)^2][3*P*P] fp32 (device, 4-byte aligned), patch (py, px) of image i at row (i*(S/P) + py)*(S/P) + px,
 * column c*P*P + y*P + x (the flatten of the patch convolution's weight), value host_lut[c * 256 + byte].  host_lut: HOST [3][256]
 * floats, or NULL for the table of the context's config (E2V_ESTATE if it has no classifier).  S a multiple of P.  Needs no weights. */
e2v_status e2v_op_image_preprocess(e2v_ctx* ctx, const void* frames, int kind, int n, int F, int H, int W, int S, int P,
                                   const float* host_lut, float* rows, e2v_stream stream);

/* ViTSelfAttention (transformers modeling_vit.py, as e2v_image_classify runs it): NON-causal self-attention over each of B images of
 * T tokens, head dim 64, scale 64^-0.5, fp32 scores and softmax.  qkv [B*T][ldqkv]: q | k | v, heads * 64 columns each (16-byte
 * aligned, ldqkv a multiple of 4); out [B*T][ldo], columns 0 .. heads * 64 - 1 written.  1 <= T <= 288 (E2V_ESHAPE): K and V of an
 * (image, head) live in LDS.  fp32 in every compute mode. */
e2v_status e2v_op_image_attention(e2v_ctx* ctx, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads,
                                  e2v_stream stream);

/* The preprocess of e2v_video_classify on its own: n clips of F frames of H x W (frames / kind as there; F a multiple of ts) ->
 * Pillow's bytes of the shortest-edge resize to `edge`, centre-cropped to S x S -> the tubelet patch-row matrix
 * rows [n*(F/ts)*(S/P)^2][3*ts*P*P] fp32 (device, 4-byte aligned): frame f = ts*t + dt of clip i writes patch (py, px) into row
 * ((i*(F/ts) + t)*(S/P) + py)*(S/P) + px, column ((c*ts + dt)*P + y)*P + x (the flatten of the Conv3d weight), value
 * host_lut[c * 256 + byte].  host_lut: HOST [3][256] floats, or NULL for the table of the context's video config (E2V_ESTATE if it
 * has none).  S a multiple of P, edge >= S.  Needs no weights. */
e2v_status e2v_op_video_preprocess(e2v_ctx* ctx, const void* frames, int kind, int n, int F, int H, int W, int S, int P, int ts,
                                   int edge, const float* host_lut, float* rows, e2v_stream stream);

/* The preprocess of e2v_clip_embed on its own: e2v_op_video_preprocess at ts = 1 (every frame an image of its own: row
 * ((i*F + f)*(S/P) + py)*(S/P) + px, column (c*P + y)*P + x) with the resize filter named (2 = BILINEAR, 3 = BICUBIC; another:
 * E2V_EINVAL).  host_lut NULL: the table of the context's vision-tower config (E2V_ESTATE if it has none). */
e2v_status e2v_op_clip_preprocess(e2v_ctx* ctx, const void* frames, int kind, int n, int F, int H, int W, int S, int P, int edge,
                                  int filter, const float* host_lut, float* rows, e2v_stream stream);

/* Non-causal self-attention over each of B sequences of T tokens, ANY T >= 1, head dim 64, scale 64^-0.5, fp32 (exact fp32 matrix
 * instructions, online softmax over key tiles; K and V are read per tile and never resident).  qkv [B*T][ldqkv]: q | k | v, heads * 64
 * columns each (16-byte aligned, ldqkv a multiple of 4); out [B*T][ldo] (16-byte aligned, ldo a multiple of 4), columns
 * 0 .. heads * 64 - 1 written.  The order of a row's sums depends on T alone.  fp32 in every compute mode. */
e2v_status e2v_op_token_attention(e2v_ctx* ctx, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads,
                                  e2v_stream stream);

/* ---- the pieces of a metric tower in a 16-bit mode (e2v_set_tower_dtype), on their own.  dtype: E2V_BF16 or E2V_F16 (another:
 * E2V_EINVAL).  The boundary stays fp32: an fp32 input is rounded once to `dtype` (round to nearest even) where the tower would hold
 * 16-bit rows, and a 16-bit result is widened exactly.  They need no weights. ---- */

/* The preprocess storing 16-bit patch rows: tower = 16: e2v_op_image_preprocess (ts / edge / filter ignored), 32:
 * e2v_op_video_preprocess (filter ignored), 64: e2v_op_clip_preprocess (ts ignored); host_lut is required.  rows as there, each value
 * the pixel table's fp32 value rounded once to `dtype`: the fp32 preprocess rounded, bit for bit. */
e2v_status e2v_op_tower_preprocess(e2v_ctx* ctx, int tower, int dtype, const void* frames, int kind, int n, int F, int H, int W, int S,
                                   int P, int ts, int edge, int filter, const float* host_lut, float* rows, e2v_stream stream);

/* Non-causal self-attention over each of B sequences of T tokens (any T >= 1), head dim 64, scale 64^-0.5, as a 16-bit tower runs it:
 * qkv [B*T][ldqkv] (q | k | v, heads * 64 columns each, any alignment) rounded to `dtype`, the 16-bit MFMA attention of the UNet
 * (cross form: one "frame" per sequence, Nq = Nk = T; fp32 scores and softmax, 16-bit probabilities and output), out [B*T][ldo]. */
e2v_status e2v_op_tower_attention(e2v_ctx* ctx, int dtype, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads,
                                  e2v_stream stream);

/* out[b][:] = (sum over t ascending of round(x[b*T + t][:])) / T in fp32: the mean over the 16-bit token rows of a clip.  B <= 65535. */
e2v_status e2v_op_tower_token_mean(e2v_ctx* ctx, int dtype, const float* x, int B, int T, int C, float* out, e2v_stream stream);

/* LayerNorm of 16-bit rows into fp32 rows: x [(rows - 1) * stride + 1][C] rounded to `dtype`; rows 0, stride, 2 stride, ... (a tower's
 * class rows: stride = T) are normalised with fp32 statistics into out [rows][C], which is NOT rounded.  C a multiple of 4 up to 1280. */
e2v_status e2v_op_tower_layernorm(e2v_ctx* ctx, int dtype, const float* x, int64_t rows, int stride, int C, const float* gamma,
                                  const float* beta, float eps, float* out, e2v_stream stream);

/* The MLP activation on 16-bit storage: out = round(act(round(x))) widened, act 0 = quick-GELU, 1 = erf GELU, evaluated in fp32.
 * count a positive multiple of 8. */
e2v_status e2v_op_tower_activation(e2v_ctx* ctx, int dtype, const float* x, int64_t count, int act, float* out, e2v_stream stream);

/* The token rows of a 16-bit tower: cls != NULL: out[i][0] = cls + pos[0], out[i][1 + p] = round(patches[i*(T-1) + p]) + pos[1 + p]
 * (ViT, CLIP); cls == NULL: out[i*T + t] = round(patches[i*T + t]) + pos[t] (VideoMAE).  fp32 sums, rounded once; cls [C] and
 * pos [T][C] are fp32 (16-byte aligned).  C a multiple of 4. */
e2v_status e2v_op_tower_embed(e2v_ctx* ctx, int dtype, const float* patches, const float* cls, const float* pos, int nimg, int T, int C,
                              float* out, e2v_stream stream);

/* layout conversion at the boundary: [n][C][FHW] <-> [n][FHW][Cpad] */
e2v_status e2v_op_to_channels_last(e2v_ctx* ctx, const float* in, float* out, int n, int C, int Cpad, int FHW,
                                   e2v_stream stream);
e2v_status e2v_op_from_channels_last(e2v_ctx* ctx, const float* in, int ld, float* out, int n, int C, int FHW,
                                     e2v_stream stream);

/* Test aid: UNet3DConditionModel.forward (EEG2Video/models/unet.py:278-413, as e2v_unet_forward) that also copies out the
 * intermediate tensors oracle/unet3d.py exposes as `taps`, in this order: "emb" (time embedding before the resnets' SiLU, unet.py:345,
 * [N, 1280, 1, 1, 1]), "down0".."down3" (after each down block incl. its downsampler, unet.py:362-373), "mid" (unet.py:376-378),
 * "up0".."up3" (after each up block incl. its upsampler, unet.py:381-404).  Each is written to `taps` (device, fp32) as a contiguous
 * NCFHW tensor, back to back; shapes[5 i ..] = {n, C, F, H, W} of tap i (host, room for 16 taps = 80 entries), *n_taps their number.
 * taps_cap = capacity of `taps` in floats (E2V_EINVAL when too small).  In the bf16 mode the taps are the bf16 tensors widened. */
e2v_status e2v_op_unet_forward_taps(e2v_ctx* ctx, const float* sample, const int64_t* host_t, int n_t, const float* cond, int N,
                                    int F, int H, int W, int T, float* out, float* taps, int64_t taps_cap, int64_t* shapes,
                                    int* n_taps, e2v_stream stream);

/* Test aid: the row-block sums that a conv of the bf16 mode leaves with its output for the GroupNorm that follows (resnet.py:177,188:
 * the statistics pass over the tensor is then skipped): x [rows][C] (device fp32, rounded to bf16 first; rows % 64 == 0, C % 8 == 0)
 * -> out[rows / 64][C][2] = (sum, sum of squares) over each 64-row block, in the library's canonical summation order. */
e2v_status e2v_op_rowblock_sums(e2v_ctx* ctx, const float* x, int64_t rows, int C, float* out, e2v_stream stream);

/* Which kernel and tile would every launch of a configuration take?  On a HOST-ONLY context (e2v_create(cfg, -1, &ctx): no GPU, no
 * weights) this runs e2v_generate -- one guided DDIM step + VAE decode of B clips of [4, F, h, w] latents with T conditioning tokens, the
 * walk of UNet3DConditionModel.forward (EEG2Video/models/unet.py:278-413) and AutoencoderKL.decode -- as a dry run: every launch rule
 * executes, nothing is launched, and each launch leaves a record "class shape -> kernel tile".  `buf` receives one line per distinct
 * record in first-occurrence order, "<count>x <record>\n" (NUL-terminated); *needed = bytes required (call with cap = 0 to size).
 * dtype: E2V_F32 or E2V_BF16.  E2V_ESTATE on a context that owns a device.  No reference counterpart. */
e2v_status e2v_op_describe_dispatch(e2v_ctx* ctx, int dtype, int B, int F, int h, int w, int T, char* buf, int64_t cap, int64_t* needed);

/* Test / profiling aid: set one of the run-time switches of DESIGN.md section 10 (the integer an environment variable of the
 * same name would give it at first use), for same-process A/B comparisons of kernel variants -- e.g. "E2V_BGEMM_PERS" 0/1.
 * Process-wide; E2V_EINVAL for an unknown name.  No reference counterpart. */
e2v_status e2v_op_set_knob(const char* name, int value);

/* Test aid: which kernel served the launch I just made?  While the run-time switch "E2V_OP_RECORD" (default 0) is non-zero, every
 * conv / linear / norm / attention entry point of this header clears a string of the calling thread when it is entered and the
 * launchers append their decision to it (" -> kernel tile", the text e2v_op_describe_dispatch records in a dry run) for each launch
 * they make.  This call copies that string to buf (NUL-terminated, cut at cap); switch off: "".  It makes no HIP call, so any thread
 * may ask, with or without a GPU.  E2V_EINVAL for cap < 0 or a null buf with cap > 0.  No reference counterpart. */
e2v_status e2v_op_last_dispatch(char* buf, int64_t cap);

/* Test aid for e2v_update_tensor: which forms of the tensor behind state-dict key `key` (of a finalized part) exist on the device right
 * now -- one bit each in *mask.  A linear (or 1x1 conv) weight: its fp32 matrix, the bf16 copy finalize makes, the fp16 copy the fp16
 * mode builds on first use, the three bf16 planes of the f32x3 mode.  A 3x3 conv weight: F32 = the torch-layout weight, BF16 / F16 = the
 * direct 16-bit layouts, and the remaining bits the layouts built on first use by the kernel that needs them.  Norm affines and biases
 * have the F32 bit only, and so does every tensor of the text encoder ("text." keys: fp32 in every compute mode).  A matrix of a metric
 * tower ("image." / "video." / "clipv.": the layers' linears and the patch embedding) has F32 after finalize and gains BF16 / F16 on the
 * tower's first call in that mode (e2v_set_tower_dtype); the classifier / projection of the fp32 head stays F32.  The update tests use it to prove that an update ran against each form.  E2V_ENOWEIGHT for an unknown key,
 * E2V_ESTATE when the key's part is not finalized (and on a host-only context).  The bits are the E2V_FORM_* values of
 * eeg2video_hip.h (e2v_read_tensor names one of them as its source).  No reference counterpart. */
e2v_status e2v_op_weight_forms(e2v_ctx* ctx, const char* key, int* mask);

/* Test aid for the bounds tests: the guarded workspace pool.  While the run-time switch "E2V_POOL_GUARD" (e2v_op_set_knob, or the
 * environment variable; default 0) is N > 0, every block the library allocates for its own kernels -- workspace-pool blocks (activations,
 * converted operands of the 16-bit op entry points, split-K and Winograd workspaces), the weight layouts of e2v_finalize_weights and those
 * built on first use, the GroupNorm workspaces -- lies between two guard zones of N KiB inside a larger allocation; the second zone starts
 * at the payload's exact last byte.  Guards and payload are filled with 0x7FC07FC0 (a NaN as fp32, and per half as bf16 and IEEE half)
 * before the block is handed out, so a result that depends on memory nobody wrote carries NaNs.  A pool block's zones are compared with
 * the pattern on the context's stream when it is released.  This call drains the stream, compares the zones of the blocks still live
 * (weight layouts and GroupNorm workspaces always are) and returns the totals since the previous report: blocks compared, zones found
 * altered, and one text line per altered zone in buf (NUL-terminated, cut at cap): kind of block, payload bytes, side, byte offset of
 * the first altered word.  Every released block keeps a result slot (8 bytes of device memory and a host record) until the next
 * report, so a guarded run that never calls this grows by 128 KiB per 16384 released blocks.  The switch takes effect for blocks allocated from then on (the pool drops its free blocks when it flips):
 * set it before e2v_create to have the weights guarded.  Off, the library makes no extra launch, byte or synchronisation.
 * E2V_ESTATE on a host-only context.  No reference counterpart. */
e2v_status e2v_op_pool_guard_report(e2v_ctx* ctx, int64_t* blocks_checked, int64_t* violations, char* buf, int64_t cap);

/* Test aid: how many blocks the context's workspace pool has handed out so far (guarded or not) -- the number of pool tensors a call
 * takes is the difference across it; a guarded run of the same call must report at least that many blocks checked. */
int64_t e2v_op_pool_gets(const e2v_ctx* ctx);

/* Test aid: the test of the detector above.  With the switch on, takes one pool block of payload_bytes (a multiple of 4), sets the 32-bit
 * word `offset` bytes (a multiple of 4, inside the zone) into its TRAILING guard zone to zero with hipMemsetAsync on `stream` -- an
 * address inside the block the pool allocated -- and releases the block: the next report shows exactly that violation, the one after it
 * none.  E2V_ESTATE while the switch is off.  No reference counterpart. */
e2v_status e2v_op_pool_guard_selftest(e2v_ctx* ctx, int64_t payload_bytes, int64_t offset, e2v_stream stream);

/* Test aid: the update arithmetic of e2v_generate_plan without a model -- the same executor, the same validation, with the UNet
 * replaced by the caller's tensors.  Everything is elementwise over `count` floats: slot 0 starts as x0 [count]; UNET op number k
 * (in plan order) takes eps_u[k] and, with guidance on (guidance_scale > 1), eps_c[k] from device arrays [n_unet][count] (eps_c may
 * be NULL with guidance off; n_unet must be the plan's number of UNET ops, else E2V_EINVAL); noise: device [n_noise][count]; out
 * [count] receives the final slot.  Timesteps are validated and otherwise unused.  No reference counterpart. */
e2v_status e2v_op_run_plan(e2v_ctx* ctx, const e2v_plan_op* ops, int n_ops, int n_slots, int final_slot, const float* x0,
                           const float* eps_u, const float* eps_c, int n_unet, const float* noise, int n_noise,
                           float guidance_scale, float* out, int64_t count, e2v_stream stream);

/* Test aid: the EEGNet embedding kernel of e2v_seq2seq_latents on its own (MyEEGNet_embedding up to the flatten, eval mode), from
 * torch-layout DEVICE tensors: w1 [F1][64], w2 [F1 D][C], w3 [F1 D][16], w4 [F2][F1 D], bn1 / bn2 / bn3 [4][n] = weight | bias |
 * running_mean | running_var.  eeg, the three strides, mean and scale ([W][C][T], both or neither NULL) as e2v_seq2seq_latents takes
 * them; out: [B * W][F2 * ((T / 4) / 8)].  The weights are folded on the host as finalize folds them: the call synchronises the stream.
 * Needs no Seq2Seq config in the context.  T < 32 or a window that does not fit the kernel's LDS: E2V_ESHAPE. */
e2v_status e2v_op_eegnet_embed(e2v_ctx* ctx, const float* eeg, int64_t clip_stride, int64_t window_stride, int64_t channel_stride,
                               const float* mean, const float* scale, int B, int W, int C, int T, int F1, int D, int F2, const float* w1,
                               const float* bn1, const float* w2, const float* bn2, const float* w3, const float* w4, const float* bn3,
                               float bn_eps, float* out, e2v_stream stream);

/* Test aid: the ShallowNet kernel of e2v_glmnet_raw on its own (shallownet up to the flatten, eval mode), from torch-layout DEVICE
 * tensors: w1 [F][K] and b1 [F] (net.0), w2 [F][F][C] and b2 [F] (net.1), bn [4][F] = weight | bias | running_mean | running_var
 * (net.2).  eeg, the two strides, mean and scale ([C][T], both or neither NULL) as e2v_glmnet_raw takes them; out: [B][F * columns],
 * columns = (T - K + 1 - P) / S + 1, filter-major.  The weights are folded on the host as finalize folds them: the call synchronises
 * the stream.  Needs no GLMNet config in the context.  T < K + P - 1 or a clip that does not fit the kernel's LDS: E2V_ESHAPE. */
e2v_status e2v_op_shallownet(e2v_ctx* ctx, const float* eeg, int64_t clip_stride, int64_t channel_stride, const float* mean, const float* scale,
                             int B, int C, int T, int F, int K, int P, int S, const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* bn, float bn_eps, float* out, e2v_stream stream);

/* Test aid: the attention kernel of e2v_seq2seq_latents on its own: Nq queries of every (clip, head) against Nk <= 32 keys, head dim D a
 * multiple of 4 up to 128, scale D^-0.5.  q [B][Nq][ldq], k, v [B][Nk][ldkv], out [B][Nq][ldo] (row strides in elements, multiples of 4;
 * heads * D columns used; clips Nq ldq / Nk ldkv / Nq ldo apart).  causal != 0: query i sits at absolute position q_pos0 + i and sees
 * keys 0 .. q_pos0 + i.  Needs no Seq2Seq config in the context. */
e2v_status e2v_op_seq_attention(e2v_ctx* ctx, const float* q, int ldq, const float* k, const float* v, int ldkv, float* out, int ldo, int B,
                                int heads, int D, int Nq, int Nk, int q_pos0, int causal, e2v_stream stream);

#ifdef __cplusplus
}
#endif
#endif
