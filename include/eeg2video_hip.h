/* eeg2video_hip.h -- C ABI of libeeg2video_hip.so: the MI355X (gfx950) implementation of the
 * EEG2Video generation hot path (Tune-A-Video denoising loop + Stable-Diffusion VAE).
 *
 * Each entry point names the reference interface it replaces (paths relative to the reference
 * repository gaspachoo/EEG2Video, snapshot 2025-07-11).  The reference is pure Python; its FFI for
 * this path would be a ctypes binding, shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an e2v_status (0 = ok, < 0 = error); e2v_last_error() gives the text.
 *   - tensors are plain pointers + sizes.  Activations at the boundary are fp32, contiguous, in the
 *     reference's own layouts (latents NCFHW, conditioning [N,T,D], videos NCFHW).  Unless a
 *     parameter says "host", pointers are DEVICE pointers of the ctx's device, owned by the caller.
 *   - the library owns weights and workspace inside the ctx; after e2v_finalize_weights() and one
 *     warm-up call of a given shape no further device allocation happens (workspace is cached).
 *     (The debug switch E2V_POOL_GUARD -- eeg2video_hip_ops.h: e2v_op_pool_guard_report, off by default --
 *     puts guard zones around these blocks; while it is on, allocations are larger, some calls synchronise and
 *     the tally of released blocks grows until e2v_op_pool_guard_report is called.)
 *   - one ctx per device; calls on one ctx must be externally serialised (the reference is a single
 *     Python thread on the default stream, @torch.no_grad()).  `stream` is a hipStream_t (NULL = the
 *     default stream); all work of a call is enqueued on it and the call does not synchronise unless
 *     stated.
 */
#ifndef EEG2VIDEO_HIP_H
#define EEG2VIDEO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct e2v_ctx e2v_ctx;
typedef void* e2v_stream;          /* hipStream_t */

typedef enum {
    E2V_OK = 0,
    E2V_EINVAL = -1,     /* bad argument (ValueError in the reference) */
    E2V_ESHAPE = -2,     /* shape mismatch ("Unexpected latents shape", pipeline_tuneeeg2video.py:239-240) */
    E2V_ENOWEIGHT = -3,  /* missing / unknown / mis-shaped state-dict key (RuntimeError, unet.py:442-448) */
    E2V_EHIP = -4,       /* HIP runtime error */
    E2V_ESTATE = -5      /* call order (weights not finalized, ...) */
} e2v_status;

typedef enum { E2V_F32 = 0, E2V_F16 = 1, E2V_BF16 = 2, E2V_F32X3 = 3 } e2v_dtype;

/* Mirror of the UNet3DConditionModel ctor kwargs the path uses (EEG2Video/models/unet.py:41-78) and of
 * the AutoencoderKL config (diffusers 0.11.1 vae/config.json).  e2v_default_config()
 * fills the Stable-Diffusion v1-4 values. */
typedef struct {
    int in_channels, out_channels;          /* 4, 4 */
    int block_out_channels[4];              /* 320, 640, 1280, 1280 */
    int layers_per_block;                   /* 2 */
    int cross_attention_dim;                /* 768 */
    int attention_heads;                    /* `attention_head_dim` = 8 = NUMBER of heads (unet_blocks.py:257-259) */
    int norm_num_groups;                    /* 32 */
    float norm_eps;                         /* 1e-5 */
    int flip_sin_to_cos;                    /* 1 */
    float freq_shift;                       /* 0 */
    /* VAE */
    int vae_in_channels, vae_latent_channels;   /* 3, 4 */
    int vae_block_out_channels[4];          /* 128, 256, 512, 512 */
    int vae_layers_per_block;               /* 2 */
    int vae_norm_num_groups;                /* 32 */
    float vae_norm_eps;                     /* 1e-6 */
    double vae_scaling_factor;              /* 0.18215 (pipeline_tuneeeg2video.py:177) */
    /* DDIM (SD-v1-4 scheduler config) */
    int num_train_timesteps;                /* 1000 */
    double beta_start, beta_end;            /* 0.00085, 0.012, "scaled_linear" */
    int steps_offset;                       /* 1 (forced by pipeline_tuneeeg2video.py:59-71) */
    /* Semantic Predictor MLP (EEG2Video/models/train_semantic_predictor.py:11-32):
     * in -> hidden -> hidden -> hidden -> hidden -> sem_tokens * cross_attention_dim, ReLU between */
    int sem_in_features;                    /* 310 */
    int sem_hidden;                         /* 10000 */
    int sem_tokens;                         /* 77 */
    /* Per-block head counts (`attention_head_dim` given as a tuple, unet.py:71,110-111: down block i takes [i] (:131), the mid block
     * [3] (:151), up block i the reversed list's [i] (:165,194); the SD-2.x UNet's 5 / 10 / 20 / 20).  All zero (the default): every
     * block has `attention_heads` heads.  Appended in round 5: e2v_config_size() tells a binding which layout a library has. */
    int attention_heads_per_block[4];
    /* CLIP text encoder (transformers CLIPTextModel, text_encoder/config.json of the SD checkpoint: vocab_size, hidden_size,
     * num_attention_heads, num_hidden_layers, intermediate_size, max_position_embeddings, hidden_act, layer_norm_eps; SD-v1-4:
     * 49408, 768, 12, 12, 3072, 77, quick_gelu, 1e-5).  All zero (the default): the context has no text encoder and expects none of
     * its keys.  text_layers > 0: text_hidden must be 64 * text_heads (64 is the head dim of both SD text towers and of the
     * attention kernel's only instance), a multiple of 4 and at most 1280 (the LayerNorm kernel), text_intermediate a multiple of 4,
     * text_max_positions at most 128 (the attention kernel keeps K and V of a prompt in LDS, two keys per lane). */
    int text_vocab_size, text_hidden, text_heads, text_layers, text_intermediate, text_max_positions;
    int text_act;                           /* 0 = quick_gelu (x sigmoid(1.702 x)), 1 = gelu (erf) */
    float text_norm_eps;
    /* ViT image classifier (transformers ViTForImageClassification, config.json of google/vit-base-patch16-224: hidden_size,
     * num_attention_heads, num_hidden_layers, intermediate_size, image_size, patch_size, the number of labels, layer_norm_eps: 768, 12,
     * 12, 3072, 224, 16, 1000, 1e-12; erf GELU, biased q / k / v) and its ViTImageProcessor (preprocessor_config.json: rescale_factor
     * 1 / 255, image_mean, image_std 0.5 each; the resize is Pillow's BILINEAR to image_size x image_size).  All zero (the default):
     * the context has no classifier and expects none of its keys.  vit_layers > 0: vit_hidden must be 64 * vit_heads, a multiple of 4
     * and at most 1280 (the LayerNorm kernel), vit_intermediate a multiple of 4, vit_image_size a multiple of vit_patch_size,
     * 3 * vit_patch_size^2 a multiple of 4, (vit_image_size / vit_patch_size)^2 + 1 tokens at most 288 (the attention kernel keeps K and
     * V of an image's head in LDS), vit_num_labels at least 3 (the top-3 head), every vit_std non-zero.  Appended after the text encoder:
     * e2v_config_size() tells a binding which layout a library has. */
    int vit_hidden, vit_heads, vit_layers, vit_intermediate, vit_image_size, vit_patch_size, vit_num_labels;
    float vit_norm_eps;
    double vit_rescale;                     /* pixel value of a byte b: ((float)(b * vit_rescale) - vit_mean[c]) / vit_std[c], in fp32 */
    float vit_mean[3], vit_std[3];
    /* VideoMAE video classifier (transformers VideoMAEForVideoClassification, config.json of MCG-NJU/videomae-base-finetuned-kinetics:
     * hidden_size, num_attention_heads, num_hidden_layers, intermediate_size, image_size, patch_size, tubelet_size, num_frames, the
     * number of labels, layer_norm_eps: 768, 12, 12, 3072, 224, 16, 2, 16 (the reference loads it with num_frames = 6), 400, 1e-12; erf
     * GELU, use_mean_pooling) and its VideoMAEImageProcessor (preprocessor_config.json: size.shortest_edge 224 = vmae_resize_edge,
     * then a centre crop of image_size x image_size, rescale_factor 1 / 255, the ImageNet mean and std).  All zero (the default): the
     * context has no video classifier and expects none of its keys.  vmae_layers > 0: vmae_hidden must be 64 * vmae_heads, a
     * multiple of 4 and at most 1280 (the LayerNorm kernel), vmae_intermediate a multiple of 4, vmae_num_frames a multiple of
     * vmae_tubelet_size, vmae_image_size a multiple of vmae_patch_size, 3 * vmae_tubelet_size * vmae_patch_size^2 a multiple of 4,
     * vmae_resize_edge >= vmae_image_size, vmae_num_labels at least 3, every vmae_std non-zero.  The token count
     * (num_frames / tubelet_size) * (image_size / patch_size)^2 has no kernel limit.  Appended after the image classifier. */
    int vmae_hidden, vmae_heads, vmae_layers, vmae_intermediate, vmae_image_size, vmae_patch_size, vmae_tubelet_size, vmae_num_frames;
    int vmae_num_labels;
    float vmae_norm_eps;                    /* the encoder layers' LayerNorms; fc_norm is nn.LayerNorm's default 1e-5 whatever this says */
    int vmae_resize_edge;                   /* the processor's shortest_edge */
    double vmae_rescale;                    /* pixel value of a byte b: ((float)(b * vmae_rescale) - vmae_mean[c]) / vmae_std[c], in fp32 */
    float vmae_mean[3], vmae_std[3];
} e2v_config;

void e2v_default_config(e2v_config* cfg);
/* sizeof(e2v_config) as THIS build of the library sees it: a binding that declares the struct itself (ctypes, cgo, JNA ...) asserts
 * its own size against this before the first e2v_default_config / e2v_create, so that a stale field list fails loudly instead
 * of having the library write past the caller's object. */
int64_t e2v_config_size(void);
const char* e2v_version(void);

/* ---- context ------------------------------------------------------------------------------------ */
/* replaces: UNet3DConditionModel.__init__ / TuneAVideoPipeline.__init__ + .to("cuda")
 * (unet.py:41-207, pipeline_tuneeeg2video.py:43-113, inference_eeg2video.py:69-70) */
/* device = -1 creates a HOST-ONLY context: it serves the key scheme and the DDIM schedule (no HIP call is
 * made, so it works on a machine without a GPU); every device entry point then returns E2V_ESTATE. */
e2v_status e2v_create(const e2v_config* cfg, int device, e2v_ctx** out);

/* CLIP vision tower (transformers CLIPVisionModelWithProjection, vision_config of openai/clip-vit-base-patch32: hidden_size,
 * num_attention_heads, num_hidden_layers, intermediate_size, image_size, patch_size, projection_dim, hidden_act, layer_norm_eps:
 * 768, 12, 12, 3072, 224, 32, 512, quick_gelu, 1e-5) and its CLIPImageProcessor (preprocessor_config.json: size.shortest_edge
 * 224 = clipv_resize_edge, resample 3 = BICUBIC, a centre crop of image_size x image_size, rescale_factor 1 / 255, CLIP's mean
 * and std).  A struct of its own, handed to e2v_create_clip_vision beside the e2v_config: e2v_config keeps its layout, and a binding
 * made for an earlier library keeps working.  clipv_hidden must be 64 * clipv_heads, a multiple of 4 and at most 1280 (the LayerNorm
 * kernel), clipv_intermediate and clipv_projection_dim multiples of 4, clipv_image_size a multiple of clipv_patch_size,
 * 3 * clipv_patch_size^2 a multiple of 4, (image_size / patch_size)^2 + 1 tokens at most 288 (B/32: 50, B/16: 197, L/14: 257),
 * clipv_resize_edge >= clipv_image_size, clipv_resample 2 or 3, every clipv_std non-zero. */
typedef struct {
    int clipv_hidden, clipv_heads, clipv_layers, clipv_intermediate, clipv_image_size, clipv_patch_size, clipv_projection_dim;
    int clipv_act;                          /* 0 = quick_gelu, 1 = gelu (erf) */
    float clipv_norm_eps;
    int clipv_resize_edge;                  /* the processor's shortest_edge */
    int clipv_resample;                     /* Pillow's filter code: 2 = BILINEAR, 3 = BICUBIC */
    double clipv_rescale;                   /* pixel value of a byte b: ((float)(b * clipv_rescale) - clipv_mean[c]) / clipv_std[c], in fp32 */
    float clipv_mean[3], clipv_std[3];
} e2v_clipv_config;
/* sizeof(e2v_clipv_config) as this build sees it: a binding asserts its own against it, as with e2v_config_size */
int64_t e2v_clipv_config_size(void);
/* e2v_create with a CLIP vision tower: the context also expects the "clipv." keys (part 64 of e2v_finalize_weights) and serves
 * e2v_clip_embed.  clipv NULL or all zero: exactly e2v_create (no tower).  A bad tower config: E2V_EINVAL. */
e2v_status e2v_create_clip_vision(const e2v_config* cfg, const e2v_clipv_config* clipv, int device, e2v_ctx** out);
/* Seq2Seq latent model (the reference's myTransformer, EEG2Video_New/Seq2Seq/my_autoregressive_transformer.py:123-192: an EEGNet
 * embedding of each EEG window, a post-LN nn.TransformerEncoder over the windows, a post-LN nn.TransformerDecoder run autoregressively
 * from a zero token, a linear to the latent of every token and a linear on the mean encoder row).  A struct of its own, handed to
 * e2v_create_ex; the reference's values: electrodes 62, samples 100, windows 7, F1 / D / F2 16 / 4 / 16, d_model 512, heads 4, ffn 2048,
 * encoder / decoder layers 2 / 4, steps 6, latent 4 x 36 x 64, 13 text classes, both eps 1e-5 (e2v_default_s2s_config).  d_model is a
 * multiple of heads and at most 1280 (the LayerNorm kernel), the head dim a multiple of 4 and at most 128 (the attention kernel),
 * windows and steps + 1 at most 32 (one key per lane of half a wave), samples at least 32, and d_model, ffn, the EEGNet feature count
 * F2 * ((samples / 4) / 8) and latent_channels * latent_h * latent_w multiples of 4; one window with its intermediates has to fit the
 * embedding kernel's 156 KiB of LDS. */
typedef struct {
    int s2s_electrodes, s2s_samples, s2s_windows;      /* C, T of one window, windows per clip */
    int s2s_f1, s2s_d, s2s_f2;                         /* MyEEGNet_embedding's F1, D, F2 */
    int s2s_d_model, s2s_heads, s2s_ffn, s2s_encoder_layers, s2s_decoder_layers;
    int s2s_steps;                                     /* decoder passes of the reference's forward: steps + 1 tokens */
    int s2s_latent_channels, s2s_latent_h, s2s_latent_w;
    int s2s_txt_classes;
    float s2s_norm_eps, s2s_bn_eps;
} e2v_s2s_config;
void e2v_default_s2s_config(e2v_s2s_config* s2s);
/* sizeof(e2v_s2s_config) as this build sees it: a binding asserts its own against it, as with e2v_config_size */
int64_t e2v_s2s_config_size(void);
/* e2v_create with either optional part: clipv as e2v_create_clip_vision takes it; s2s non-NULL and not all zero: the context also
 * expects the "s2s." keys (part 128 of e2v_finalize_weights) and serves e2v_seq2seq_latents.  Both NULL: exactly e2v_create.  A bad
 * config of either: E2V_EINVAL, with a message that names the limit. */
e2v_status e2v_create_ex(const e2v_config* cfg, const e2v_clipv_config* clipv, const e2v_s2s_config* s2s, int device, e2v_ctx** out);
/* The GLMNet pair (the reference's EEG2Video/models/models.py:105-123, 352-413).  glfnet(raw_out, emb, electrodes, samples) over raw
 * EEG: a global shallownet over all electrodes and one over the occipital electrodes occ_first .. occ_first + occ_count - 1 -- each
 * Conv2d(1, filters, (1, taps)), Conv2d(filters, filters, (C, 1)), BatchNorm2d on running statistics, ELU, AvgPool2d((1, pool), (1,
 * pool_stride)), flatten, Linear(-> emb) -- and Linear(2 emb, raw_out) on the concatenation.  glfnet_mlp(mlp_out, emb, electrodes *
 * bands) over DE features: two mlpnets -- Linear(-> hidden1), erf GELU, Linear(-> hidden2), GELU, Linear(-> emb) -- over the flattened
 * [electrodes][bands] block and its occipital rows, and Linear(2 emb, mlp_out).  A struct of its own, handed to e2v_create_ex2; the
 * reference's values: electrodes 62, samples 200, occipital 50 / 12, filters 40, taps 25, pool 51 / 5, bands 5, hidden 512 / 256, emb
 * 64, raw_out 2, mlp_out 40, eps 1e-5 (e2v_default_glm_config).  raw_out / mlp_out 0: that model is absent (not both).  Refused, each
 * with a message that names the limit: an occipital range outside the electrodes; emb, hidden1 or hidden2 not a multiple of 4; with a raw
 * model, samples below taps + pool - 1, a width filters * pooled columns that is not a multiple of 4, at the reference's filter and
 * pool sizes a width other than the reference's own 1040 * (samples / 200) (it sizes its linear that way: only samples 200 .. 204
 * agree, 205 and 400 fail inside the reference), and a clip that does not fit the ShallowNet kernel's 156 KiB of LDS. */
typedef struct {
    int glm_electrodes, glm_samples;                   /* C, T of one clip */
    int glm_occ_first, glm_occ_count;                  /* the occipital electrodes */
    int glm_filters, glm_taps, glm_pool, glm_pool_stride;
    int glm_bands, glm_hidden1, glm_hidden2;           /* glfnet_mlp: features per electrode, the two hidden widths */
    int glm_emb;                                       /* width of each net's embedding */
    int glm_raw_out, glm_mlp_out;                      /* width of glfnet's / glfnet_mlp's head; 0: the model is absent */
    float glm_bn_eps;
} e2v_glm_config;
void e2v_default_glm_config(e2v_glm_config* glm);
/* sizeof(e2v_glm_config) as this build sees it: a binding asserts its own against it, as with e2v_config_size */
int64_t e2v_glm_config_size(void);
/* e2v_create_ex with the GLMNet pair beside the other optional parts: glm non-NULL and not all zero: the context also expects the
 * "glm." keys (part 256 of e2v_finalize_weights) and serves e2v_glmnet_raw / e2v_glmnet_mlp.  glm NULL: exactly e2v_create_ex. */
e2v_status e2v_create_ex2(const e2v_config* cfg, const e2v_clipv_config* clipv, const e2v_s2s_config* s2s, const e2v_glm_config* glm,
                          int device, e2v_ctx** out);
void e2v_destroy(e2v_ctx* ctx);
const char* e2v_last_error(const e2v_ctx* ctx);      /* ctx may be NULL: last error of a failed e2v_create */

/* ---- weights ------------------------------------------------------------------------------------ */
/* replaces: ModelMixin.from_pretrained / load_state_dict (unet.py:415-449, inference_eeg2video.py:69).
 * `key` is the reference state-dict key; UNet keys as they are ("conv_in.weight", "down_blocks.0....",
 * SURVEY App. D), VAE keys prefixed "vae." ("vae.decoder.conv_in.weight").  `data` is a HOST pointer in
 * the torch layout (Conv2d [Cout,Cin,kh,kw], Linear [out,in]); the shape is checked against the config.
 * dtype: E2V_F32, E2V_F16 or E2V_BF16 (16-bit checkpoints are widened to fp32, exactly). */
e2v_status e2v_load_tensor(e2v_ctx* ctx, const char* key, const void* host_data, e2v_dtype dtype,
                           const int64_t* shape, int ndim);
/* number of keys the config expects / a key by index (for loaders that iterate) */
int64_t e2v_num_expected_keys(const e2v_ctx* ctx);
const char* e2v_expected_key(const e2v_ctx* ctx, int64_t i, int64_t* shape4, int* ndim);
/* re-layout to the kernels' formats (tap-major convs, fused QKV / KV, GEGLU row interleave).
 * which: bit 0 = UNet, bit 1 = VAE, bit 2 = semantic predictor (keys "semantic.mlp.{0,2,4,6,8}.{weight,bias}"), bit 3 = CLIP text
 * encoder (config with text_layers > 0; the keys of the checkpoint's text_encoder under the prefix "text.":
 * "text.text_model.embeddings.{token,position}_embedding.weight", per layer "text.text_model.encoder.layers.{i}."
 * "self_attn.{q,k,v,out}_proj.{weight,bias}", "layer_norm{1,2}.{weight,bias}", "mlp.fc{1,2}.{weight,bias}", and
 * "text.text_model.final_layer_norm.{weight,bias}"; q / k / v become one [3C][C] matrix with its [3C] bias).  The text part keeps
 * fp32 matrices only, in every compute mode (E2V_F32X3 included).
 * bit 4 (16) = ViT image classifier (config with vit_layers > 0; the keys of the google/vit-base-patch16-224 checkpoint under the
 * prefix "image.": "image.vit.embeddings.{cls_token,position_embeddings}", "image.vit.embeddings.patch_embeddings.projection.{weight,bias}",
 * per layer "image.vit.encoder.layer.{i}." "attention.attention.{query,key,value}.{weight,bias}", "attention.output.dense.*",
 * "layernorm_{before,after}.*", "intermediate.dense.*", "output.dense.*", and "image.vit.layernorm.*", "image.classifier.*";
 * query / key / value become one [3C][C] matrix with its [3C] bias).  fp32 matrices only, as the text part.
 * bit 5 (32) = VideoMAE video classifier (config with vmae_layers > 0; the names of transformers' VideoMAEForVideoClassification
 * state dict under the prefix "video.": "video.videomae.embeddings.patch_embeddings.projection.{weight,bias}" -- the Conv3d weight
 * [C][3][ts][P][P] with its channel and tubelet axes merged, [C][3 * ts][P][P]: expected-key shapes have at most four axes --, per layer
 * "video.videomae.encoder.layer.{i}." "attention.attention.{query,key,value}.{weight,bias}", "attention.output.dense.*",
 * "layernorm_{before,after}.*", "intermediate.dense.*", "output.dense.*", then "video.fc_norm.*", "video.classifier.*", and one key
 * that is not in a checkpoint: "video.videomae.embeddings.position_embeddings" [T][C], the fixed sinusoid transformers computes at
 * construction for the model's num_frames, supplied by the caller).  fp32 matrices only.
 * bit 6 (64) = CLIP vision tower (a context made by e2v_create_clip_vision; the names of transformers' CLIPVisionModelWithProjection state dict
 * under the prefix "clipv.": "clipv.vision_model.embeddings.class_embedding" [C], "...patch_embedding.weight" [C][3][P][P] (no
 * bias), "...position_embedding.weight" [T][C], "clipv.vision_model.pre_layrnorm.*" (the checkpoint's spelling), per layer
 * "clipv.vision_model.encoder.layers.{i}." "self_attn.{q,k,v,out}_proj.*", "layer_norm{1,2}.*", "mlp.fc{1,2}.*", then
 * "clipv.vision_model.post_layernorm.*" and "clipv.visual_projection.weight" [projection_dim][C] (no bias); the position_ids
 * buffer of older checkpoints is not a weight and not expected).  fp32 matrices only.
 * bit 7 (128) = Seq2Seq latent model (a context made by e2v_create_ex with an e2v_s2s_config -- on any other context the bit is outside
 * the mask, E2V_EINVAL as before the part existed; the names of the reference's
 * myTransformer state dict under the prefix "s2s.": "s2s.eeg_embedding.block_1.1.weight" [F1][1][1][64], "...block_1.2.{weight,bias,
 * running_mean,running_var}", "...block_2.0.weight" [F1 D][1][C][1], "...block_2.1.*", "...block_3.1.weight" [F1 D][1][1][16],
 * "...block_3.2.weight" [F2][F1 D][1][1], "...block_3.3.*", "s2s.eeg_embedding.embedding.*", per encoder layer
 * "s2s.transformer_encoder.layers.{i}." "self_attn.in_proj_{weight,bias}", "self_attn.out_proj.*", "linear{1,2}.*", "norm{1,2}.*", per
 * decoder layer the same with "multihead_attn.*" and "norm3.*", then "s2s.txtpredictor.*", "s2s.predictor.*", and one key that is
 * ours: "s2s.positional_encoding.pe" [windows][d_model], the first rows of the reference's sinusoid buffer, supplied by the caller
 * (it is fp32 torch arithmetic of the reference: the caller hands over its bits).  NOT expected, because inference never reads them:
 * "embedding.weight", "img_embedding.*", every "num_batches_tracked", and the [1][5000][d_model] buffer itself.  Finalize folds the three
 * BatchNorms (running statistics) into the embedding kernel's pack and keeps every loaded tensor: fp32 matrices only, and
 * e2v_read_tensor returns every "s2s." key with the loaded bits.
 * bit 8 (256) = the GLMNet pair (a context made by e2v_create_ex2 with an e2v_glm_config -- on any other context the bit is outside the
 * mask, E2V_EINVAL as before the part existed): "glm.raw." + the names of the reference's glfnet state dict -- per net n in
 * {globalnet, occipital_localnet}: "n.net.0.{weight [F][1][1][taps], bias}", "n.net.1.{weight [F][F][C][1], bias}",
 * "n.net.2.{weight, bias, running_mean, running_var}", "n.out.*"; then "out.*" -- and "glm.mlp." + glfnet_mlp's -- per net
 * "n.net.{1,3,5}.*", then "out.*" --, each set only if its model is configured.  NOT expected: "num_batches_tracked".  Finalize folds
 * each net's two convolutions and its BatchNorm into one filter and keeps every loaded tensor: fp32 only, and e2v_read_tensor returns
 * every "glm." key with the loaded bits.
 * every expected key of the selected parts must have been loaded. */
e2v_status e2v_finalize_weights(e2v_ctx* ctx, int which);
/* replaces: optimizer.step() as the validation pipeline sees it (train_finetune_videodiffusion.py:117-121,196-200,320-335: the
 * pipeline is built around the LIVE unet, and only attn1.to_q, attn2.to_q and attn_temp.* move between two validations, :47-51)
 * and load_state_dict(partial, strict=False) on a built model.
 * Overwrites one tensor of a FINALIZED part in place: every form of it that exists on the device (the fp32 matrix or its slice of a
 * fused / interleaved one, the bf16 and fp16 copies, the f32x3 planes, every 3x3-conv layout already built) receives the new values,
 * with the roundings finalize uses -- the device state is bit-identical to a fresh context that loaded the state dict with this
 * tensor replaced and was finalized in the same mode.  Forms not built yet stay unbuilt and derive from the new values on first use.
 * `key`: any expected key (UNet, "vae.", "semantic.").  dtype: E2V_F32, E2V_F16 or E2V_BF16 (E2V_F32X3: E2V_EINVAL).
 * on_device = 1: `data` is a device pointer on the ctx's device, read on `stream` (no host round trip); on_device = 0: a host
 * pointer, copied into the workspace pool in its own type (hipMemcpyAsync: pinned memory must stay valid until the stream has
 * passed the call) and widened on the device.  Stream-ordered: calls queued earlier on `stream` see the old weights, later ones
 * the new; no device synchronisation, and no allocation once the workspace of such a call is cached (e2v_device_bytes does not move).
 * Part not finalized: E2V_ESTATE (use e2v_load_tensor); unknown key / shape mismatch: E2V_ENOWEIGHT as e2v_load_tensor.
 * A "text." key: E2V_EINVAL -- the text encoder is frozen on this path (train_finetune_videodiffusion.py:115
 * `text_encoder.requires_grad_(False)`); another text encoder is loaded with e2v_load_tensor + e2v_finalize_weights(ctx, 8).
 * An "image." key: E2V_EINVAL as well -- the classifier is a frozen yardstick (40_class_run_metrics.py:70-72 loads it and only
 * calls it); another one is loaded with e2v_load_tensor + e2v_finalize_weights(ctx, 16).  A "video." key: the same (part 32).
 * An "s2s." key: E2V_EINVAL too -- the Seq2Seq model is trained by its own script and only called here, and its BatchNorms are folded
 * at finalize; load a new one with e2v_load_tensor + e2v_finalize_weights(ctx, 128).
 * A "glm." key: E2V_EINVAL as well, for the same reason (its BatchNorms are folded at finalize); reload and e2v_finalize_weights(ctx, 256).
 * A "clipv." key (part 64) is updated like a UNet key: the fp32 form, and the bf16 / fp16 copy of a matrix (the layers' linears, the
 * patch embedding) once the tower has built it in a 16-bit mode (e2v_set_tower_dtype) -- every copy that exists is refreshed. */
e2v_status e2v_update_tensor(e2v_ctx* ctx, const char* key, const void* data, e2v_dtype dtype, int on_device,
                             const int64_t* shape, int ndim, e2v_stream stream);

/* The stored forms of one tensor of a finalized part, one bit each (the mask e2v_op_weight_forms reports; the `form` of e2v_read_tensor). */
enum {
    E2V_FORM_F32 = 1 << 0,
    E2V_FORM_BF16 = 1 << 1,
    E2V_FORM_F16 = 1 << 2,
    E2V_FORM_X3 = 1 << 3,              /* f32x3 planes of a linear */
    E2V_FORM_CONV_DIRECT32 = 1 << 4,   /* fp32 direct implicit-GEMM layout */
    E2V_FORM_WINO2 = 1 << 5,           /* Winograd F(2x2,3x3) domain */
    E2V_FORM_WINO4 = 1 << 6,           /* Winograd F(4x4,3x3) domain */
    E2V_FORM_BF16_UP2 = 1 << 7,        /* sub-pixel form of resize + conv, bf16 */
    E2V_FORM_F16_UP2 = 1 << 8,         /* the same as IEEE half */
    E2V_FORM_WINO2_X3 = 1 << 9,        /* f32x3 planes of the F(2x2) form */
    E2V_FORM_WINO4_X3 = 1 << 10        /* f32x3 planes of the F(4x4) form */
};
/* replaces: model.state_dict() / pipeline.save_pretrained(output_dir) on the live modules (unet.py:445 walks model.state_dict();
 * train_semantic_predictor.py:146-147 saves it; train_finetune_videodiffusion.py:343-350,355-362 builds a pipeline around the trained
 * modules and saves it).  The counterpart of e2v_update_tensor: after an update with on_device = 1 the device holds the only current
 * copy of a weight, and this call reads it back.
 * Writes one tensor of a FINALIZED part to `out` in the torch layout of the reference state dict -- the inverse of every re-layout
 * finalize makes: a 3x3 conv [Cout,Cin,3,3] from the torch-layout weight the context keeps, a row range of a fused QKV / KV matrix
 * (and of its fused bias), the GEGLU row interleave of ff.net.0.proj undone, the K-padded first layer of the Semantic Predictor
 * without its padding columns, plain linears, 1x1 convs, norm affines and embeddings as they are.
 * `key`: any expected key (UNet, "vae.", "semantic.", "text.", "image.", "video.", "clipv.": reading a text or classifier tensor is allowed, only updating one is refused).
 * `form`: which stored form is read -- 0 or E2V_FORM_F32: the fp32 values (every tensor has them).  For the weight of a linear
 * (or 1x1 conv) also E2V_FORM_BF16 / E2V_FORM_F16: that stored 16-bit copy, widened exactly, and E2V_FORM_X3: (p0 + p1) + p2 of the
 * three planes in fp32, which is the fp32 weight exactly.  A form e2v_op_weight_forms does not report for the key: E2V_ESTATE ("form
 * not built").  More than one bit, an unknown bit, a form with no index-map inverse (the conv kernel layouts, the Winograd domains,
 * the UP2 forms), or a 16-bit / X3 form of anything but a linear's weight: E2V_EINVAL.
 * `dtype`: the type of `out`, E2V_F32, E2V_BF16 or E2V_F16 (round to nearest even, the casts finalize uses; E2V_F32X3: E2V_EINVAL).
 * `shape` / `ndim`: the key's expected shape, else E2V_ENOWEIGHT as e2v_load_tensor.
 * on_device = 1: `out` is a device pointer of ANY alignment on the ctx's device; exactly numel elements are written, on `stream`:
 * a read queued before an update sees the old values, one queued after it the new.  No synchronisation and no allocation at all.
 * on_device = 0: `out` is a host pointer; the tensor is gathered into a workspace-pool block in `dtype` and copied out, and the call
 * returns when the copy has landed.  It waits for `stream` ONLY: work queued on other streams is neither waited for nor ordered.
 * No allocation once the staging block of that size is cached (e2v_device_bytes does not move).
 * The argument checks come before anything is enqueued and before the host-only check: null ctx / key / out / shape E2V_EINVAL,
 * unknown key E2V_ENOWEIGHT, part not finalized E2V_ESTATE; a well-formed call on a host-only context: E2V_ESTATE. */
e2v_status e2v_read_tensor(e2v_ctx* ctx, const char* key, int form, void* out, e2v_dtype dtype, int on_device,
                           const int64_t* shape, int ndim, e2v_stream stream);

/* ---- schedule (host, integer-exact) ---------------------------------------------------------------- */
/* replaces: DDIMScheduler.set_timesteps (call site pipeline_tuneeeg2video.py:287-288).
 * t_i = (i * (T // n))[::-1] + steps_offset, int64; n=50 -> 981, 961, ..., 21, 1. */
e2v_status e2v_ddim_timesteps(const e2v_ctx* ctx, int num_inference_steps, int64_t* host_out);
/* alpha-bar table (fp32 cumprod of 1 - linspace(sqrt(b0), sqrt(b1), T)^2), host copy of T floats.
 * The library computes it with scalar fp32 arithmetic; torch.linspace's vectorised CPU kernel can differ in
 * the last bit depending on the host's SIMD width, so a host that wants the very table its own diffusers
 * install would build hands it in with e2v_set_alphas_cumprod (the Python mirror does). */
e2v_status e2v_ddim_alphas_cumprod(const e2v_ctx* ctx, float* host_out);
e2v_status e2v_set_alphas_cumprod(e2v_ctx* ctx, const float* host_table, int n);
/* replaces: the scheduler config the pipeline reads (scheduler.config.steps_offset / num_train_timesteps,
 * pipeline_tuneeeg2video.py:59-71; tuneavideo/util.py:58).  Hands the ctx the whole schedule of the scheduler object the
 * caller holds -- table of n = num_train_timesteps alpha-bars and steps_offset -- so that the fused loop (e2v_generate,
 * e2v_ddim_invert) and the caller's own stepped loop walk the same timesteps with the same coefficients. */
e2v_status e2v_set_ddim_schedule(e2v_ctx* ctx, const float* host_alphas_cumprod, int n, int steps_offset);

/* ---- the hot path --------------------------------------------------------------------------------- */
/* replaces: UNet3DConditionModel.forward (unet.py:278-413).
 * sample [N,C,F,H,W], timesteps int64 HOST array of length n_t (1 = broadcast, else N),
 * cond [N,T,cross_attention_dim], out [N,out_channels,F,H,W]. */
e2v_status e2v_unet_forward(e2v_ctx* ctx, const float* sample, const int64_t* host_timesteps, int n_t,
                            const float* cond, int N, int F, int H, int W, int T, float* out, e2v_stream stream);

/* The same with FRACTIONAL timesteps, as the sigma-space schedulers the pipeline's constructor accepts produce them
 * (pipeline_tuneeeg2video.py:48-55: LMSDiscrete / EulerDiscrete / EulerAncestralDiscrete: timesteps = linspace(0, T-1, n)[::-1];
 * unet.py:324-339 turns a float timestep into the fp32 argument of the sinusoid).  host_timesteps: n_t floats. */
e2v_status e2v_unet_forward_ft(e2v_ctx* ctx, const float* sample, const float* host_timesteps, int n_t, const float* cond,
                               int N, int F, int H, int W, int T, float* out, e2v_stream stream);

/* replaces: noise_pred chunk + guidance + scheduler.step (pipeline_tuneeeg2video.py:320-325), eta = 0.
 * eps_cond may be NULL (guidance off).  t, t_prev are train timesteps (t_prev < 0 -> final alpha = abar[0]). */
e2v_status e2v_ddim_cfg_step(e2v_ctx* ctx, const float* eps_uncond, const float* eps_cond, const float* x,
                             float* x_out, int64_t count, float guidance_scale, int64_t t, int64_t t_prev,
                             e2v_stream stream);

/* replaces: the guidance line noise_pred_uncond + guidance_scale * (noise_pred_text - noise_pred_uncond)
 * (pipeline_tuneeeg2video.py:320-322) for schedulers whose update is not fused with it (everything but DDIM). */
e2v_status e2v_cfg_combine(e2v_ctx* ctx, const float* eps_uncond, const float* eps_cond, float guidance_scale, float* out,
                           int64_t count, e2v_stream stream);

/* out = sum_{i<n} coefs[i] * xs[i], 1 <= n <= 5 (host arrays of n device pointers / n coefficients): the arithmetic of the
 * linear multistep schedulers the pipeline's constructor accepts (pipeline_tuneeeg2video.py:48-55) -- PNDM/PLMS's
 * (55 e1 - 59 e2 + 37 e3 - 9 e4) / 24 and its sample update; host side in eeg2video_amd/scheduler.py: PNDMScheduler. */
e2v_status e2v_lincomb(e2v_ctx* ctx, int n, const float* const* xs, const float* coefs, float* out, int64_t count,
                       e2v_stream stream);

/* replaces: next_step (EEG2Video_New/Generation/tuneavideo/util.py:56-66), the deterministic DDIM update run towards
 * noise: alpha_t = abar[min(t - T/n, 999)] (final alpha when negative), alpha_next = abar[t];
 * x_next = sqrt(alpha_next) (x - sqrt(1-alpha_t) eps) / sqrt(alpha_t) + sqrt(1-alpha_next) eps. */
e2v_status e2v_ddim_next_step(e2v_ctx* ctx, const float* eps, const float* x, float* x_out, int64_t count, int64_t t,
                              int num_inference_steps, e2v_stream stream);

/* replaces: ddim_loop / ddim_inversion (util.py:74-101; caller train_finetune_videodiffusion.py:326-328): num_inv_steps
 * times { eps = unet(latent, t_i, cond); latent = next_step(eps, t_i, latent) } over the ascending DDIM timesteps, no
 * guidance.  latents [B,4,F,h,w], cond [B,T,cross_attention_dim]; all_latents (may be NULL) receives the reference's
 * list [latent_0 .. latent_n] as [n+1][B,4,F,h,w]; final_latent (may be NULL) = all_latents[-1], what the caller feeds
 * back as `latents=`. */
e2v_status e2v_ddim_invert(e2v_ctx* ctx, const float* latents, const float* cond, int B, int F, int h, int w, int T,
                           int num_inv_steps, float* all_latents, float* final_latent, e2v_stream stream);

/* postprocess = 1 replaces TuneAVideoPipeline.decode_latents (pipeline_tuneeeg2video.py:175-184) without the
 * D2H copy: latents [B,4,F,h,w] -> (vae.decode(latents / 0.18215).sample / 2 + 0.5).clamp(0,1) as videos
 * [B,3,F,8h,8w].  postprocess = 0 replaces AutoencoderKL.decode (call site :179): z [B,4,F,h,w] is decoded as
 * given (no 1/0.18215, no clamp); the (b f) frames of the reference are B = n, F = 1. */
e2v_status e2v_vae_decode(e2v_ctx* ctx, const float* latents, int B, int F, int h, int w, int postprocess,
                          float* videos, e2v_stream stream);
/* replaces: AutoencoderKL.encode(...).latent_dist (train_finetune_videodiffusion.py:264,
 * EEG2Video_New/Seq2Seq/generate_1200_latent.py:38): images [n,3,H,W] -> mean, logvar [n,4,H/8,W/8]
 * (logvar clamped to [-30,20]); no 0.18215 factor (that is the caller's, as in the reference). */
e2v_status e2v_vae_encode(e2v_ctx* ctx, const float* images, int n, int H, int W, float* mean, float* logvar,
                          e2v_stream stream);

/* replaces: the body of TuneAVideoPipeline.__call__ after _encode_eeg (pipeline_tuneeeg2video.py:287-334):
 * set_timesteps, the denoising loop with classifier-free guidance (guidance_scale > 1) and the VAE decode,
 * all enqueued on `stream` without a host round trip per step.
 * latents [B,4,F,h,w] (already scaled by init_noise_sigma = 1), cond [B,T,D], uncond [Bu,T,D] with Bu = 1
 * (broadcast, the reference's negative.npy) or B; videos [B,3,F,8h,8w] (may be NULL: skip decode);
 * latents_out [B,4,F,h,w] (may be NULL). */
e2v_status e2v_generate(e2v_ctx* ctx, const float* latents, const float* cond, const float* uncond, int Bu,
                        int B, int F, int h, int w, int T, int num_inference_steps, float guidance_scale,
                        float eta, float* videos, float* latents_out, e2v_stream stream);

/* ---- sampler plans: every scheduler the pipeline accepts in the device loop ---------------------------------------------------------
 * replaces: the same loop body (pipeline_tuneeeg2video.py:311-331) for the scheduler types other than deterministic DDIM that
 * TuneAVideoPipeline.__init__ accepts (:48-55: PNDM -- what a stock SD-v1-4 directory names, inference_eeg2video.py:70,92 --
 * LMSDiscrete, EulerDiscrete, EulerAncestralDiscrete, DPMSolverMultistep) and for DDIM with eta > 0.
 * The scheduler arithmetic is NOT in the library: a plan is the flat list of the updates the host-side scheduler would have issued
 * through e2v_lincomb, recorded once (eeg2video_amd/sampler_plan.py: trace_plan), over numbered work slots of [B,4,F,h,w] floats.
 *   E2V_PLAN_UNET     reads slot src[0] (n_src = 1), evaluates the UNet at `timestep` (fractional = 0: an integral value in
 *                     [0, num_train_timesteps), the path of e2v_unet_forward; fractional != 0: the fp32 value, the path of
 *                     e2v_unet_forward_ft) and writes the guided eps, eps_u + g (eps_c - eps_u) as e2v_cfg_combine computes it
 *                     (:320-322), or eps itself when guidance is off, into slot dst;
 *   E2V_PLAN_LINCOMB  dst = sum_{k < n_src} (float)coef[k] * src[k], 1 <= n_src <= 5, as e2v_lincomb computes it; src[k] >= 0 is
 *                     a work slot, src[k] = -1 - j tensor j of the caller's noise array.
 * Slot 0 holds the latents on entry; no op writes a slot it reads.  New fields are appended (e2v_plan_op_size() tells a binding
 * which layout a library has); `reserved` must be 0. */
enum { E2V_PLAN_UNET = 0, E2V_PLAN_LINCOMB = 1 };
enum { E2V_PLAN_MAX_SLOTS = 8, E2V_PLAN_MAX_TERMS = 5 };
typedef struct {
    int32_t kind;                           /* E2V_PLAN_UNET / E2V_PLAN_LINCOMB */
    int32_t dst;                            /* work slot written */
    int32_t n_src;                          /* UNET: 1; LINCOMB: 1..5 */
    int32_t src[5];
    double coef[5];                         /* LINCOMB: cast to float where it is used */
    double timestep;                        /* UNET */
    int32_t fractional;                     /* UNET: timestep differs from its rounding */
    int32_t reserved;
} e2v_plan_op;
int64_t e2v_plan_op_size(void);

/* e2v_generate with the per-step update given as a plan: latents / cond / uncond / videos / latents_out, guidance (off at
 * guidance_scale <= 1), stream order, no synchronisation and no allocation once the workspaces of a shape (and n_slots, n_noise)
 * are cached -- all as e2v_generate; the two share one loop.  final_slot: the slot holding the latents after the last op.
 * noise: device [n_noise][B,4,F,h,w] (NULL with n_noise = 0), read once at the start of the call.
 * The plan is validated on the host before anything is enqueued, and before the host-only check: E2V_EINVAL, the text naming the op
 * ("plan op 3: ..."), for a slot or noise index out of range, a term count outside 1..5 (UNET: 1), a slot read before any op wrote
 * it (slot 0 excepted), an op writing a slot it reads, a non-finite coefficient or timestep, an integral timestep outside
 * [0, num_train_timesteps); and for a plan with n_slots outside 1..E2V_PLAN_MAX_SLOTS, without a UNET op, or with a final_slot out
 * of range or never written.  A well-formed plan on a host-only context: E2V_ESTATE. */
e2v_status e2v_generate_plan(e2v_ctx* ctx, const float* latents, const float* cond, const float* uncond, int Bu, int B, int F,
                             int h, int w, int T, const e2v_plan_op* ops, int n_ops, int n_slots, int final_slot,
                             const float* noise, int n_noise, float guidance_scale, float* videos, float* latents_out,
                             e2v_stream stream);

/* ---- the steps either side of the path -------------------------------------------------------- */
/* rank 1 -- replaces CLIP.forward of the Semantic Predictor (EEG2Video/models/train_semantic_predictor.py:11-32, called
 * at pipeline_tuneeeg2video.py:149): eeg [B, sem_in_features] -> embeddings [B, sem_tokens * cross_attention_dim]
 * (the caller reshapes to [B,77,768], :150), all on device. */
e2v_status e2v_semantic_predict(e2v_ctx* ctx, const float* eeg, int B, float* out, e2v_stream stream);

/* replaces: CLIPTextModel.forward(input_ids)[0] (pipelines/pipeline_tuneavideo.py:174-177,220-223; train_finetune_videodiffusion.py:281)
 * -- the prompt embeddings, the unconditional embedding (negative.npy) and the targets the Semantic Predictor regresses to.
 * host_ids: HOST [B][T] token ids (as host_timesteps / host_t: the tokenizer's output never has to visit the device); every id is
 * checked against [0, text_vocab_size) before anything is enqueued (E2V_EINVAL); 1 <= T <= text_max_positions (else E2V_ESHAPE).
 * out: device [B][T][text_hidden] fp32, 16-byte aligned (E2V_EINVAL otherwise), the last hidden state after final_layer_norm -- directly usable as cond / uncond of
 * e2v_generate.  Causal mask, no padding mask (use_attention_mask is absent from the SD text_encoder config); no pooled output.
 * ARITHMETIC IS FP32 IN EVERY COMPUTE MODE (fp32 rows, fp32 matrices, the linears of the time-embedding MLP's kind): the same
 * ids give the same bits under E2V_F32, E2V_BF16, E2V_F16 and E2V_F32X3 contexts.  (The reference runs this model in fp16; at
 * 13 GFLOP per prompt against the 600 TFLOP of a clip the tighter choice costs nothing.)
 * No text config / text part not finalized / host-only context: E2V_ESTATE.  Stream-ordered, does not synchronise, allocates nothing
 * once the workspace of a (B, T) is cached. */
e2v_status e2v_text_encode(e2v_ctx* ctx, const int64_t* host_ids, int B, int T, float* out, e2v_stream stream);

/* rank 9 -- replaces myTransformer.forward in eval mode (EEG2Video_New/Seq2Seq/my_autoregressive_transformer.py:151-192) and the
 * `out[:, :-1]` its inference keeps (:383-384): EEG windows in, the latents DANA or the pipeline takes out.
 * eeg: device fp32, 4-byte aligned; sample t of electrode c of window w of clip b is eeg[b clip_stride + w window_stride +
 * c channel_stride + t] (element strides, non-negative).  Stacked windows [B][windows][electrodes][samples] are (windows electrodes
 * samples, electrodes samples, samples); a raw segment [B][electrodes][L] under the reference's sliding windows of `samples` with
 * step s (:309-314: 100 and 50 over L = 400) is (electrodes L, s, L) -- no host-side windowing.
 * mean, scale: device [windows][electrodes][samples] fp32, both or neither NULL: the input scaler (x - mean) / scale applied as a
 * value is read, true division -- the reference's StandardScaler over the stacked windows (:320-330; its features run (electrode,
 * sample, window): the caller reorders).
 * The decoder starts from a zero token and appends one token per step; token j of the steps + 1 is the latent predictor's input j.
 * first, count: the tokens [first, first + count) are returned; only first + count - 1 decoder steps run (each new token is one row
 * against per-layer cached keys and values, the same arithmetic as the reference's recomputation of all rows under the causal mask).
 * The reference's [:, :-1] is first = 0, count = steps: its last pass is never run.  Token 0 is predictor.bias for every clip.
 * layout 0: latents [B][count][latent_channels][h][w] (what e2v_dana_noise takes as x0); 1: [B][latent_channels][count][h][w] (the
 * pipeline's layout).  txt_logits: [B][txt_classes], txtpredictor of the mean encoder row.  tokens: [B][steps + 1][d_model], the decoder's
 * token rows; rows 0 .. first + count - 1 are written, the rest left alone.  Any of the three may be NULL, not all; first / count /
 * layout are checked whenever latents or tokens is given, and a call for txt_logits alone runs no decoder step.
 * ARITHMETIC IS FP32 IN EVERY COMPUTE MODE, as e2v_text_encode; a clip's bits do not depend on B or on its place in the batch.
 * Checked before anything is enqueued, in this order: NULL eeg / no output / mean without scale / a pointer off its alignment (eeg,
 * mean, scale, txt_logits 4 bytes; latents, tokens 16) / negative stride / layout not 0 or 1 / first < 0, count < 1, first + count >
 * steps + 1 / B < 1: E2V_EINVAL; then no Seq2Seq config, part 128 not finalized, host-only context: E2V_ESTATE.
 * Stream-ordered, does not synchronise, allocates nothing once the workspace of a (B, first + count) is cached. */
e2v_status e2v_seq2seq_latents(e2v_ctx* ctx, const float* eeg, int64_t clip_stride, int64_t window_stride, int64_t channel_stride,
                               const float* mean, const float* scale, int B, int first, int count, int layout, float* latents,
                               float* txt_logits, float* tokens, e2v_stream stream);

/* rank 10 -- replaces DE_PSD (EEG_preprocessing/DE_PSD.py:8-71) and the loops of its three extractors over clips, windows and
 * electrodes: differential entropy and power spectral density of the five bands of every EEG row.  No weights: any context with a
 * device serves it.
 * eeg: device fp32, 4-byte aligned; sample t of electrode c of window w of clip b is eeg[b clip_stride + w window_stride +
 * c channel_stride + t] (element strides, non-negative).  The one 2-s window of a raw segment [B][62][400] is windows = 1, samples = 400,
 * strides (24800, 0, 400); its seven 500-ms windows are windows = 7, samples = 100, strides (24800, 50, 400) -- no host-side windowing.
 * Per row, as the reference: the Hann row 0.5 - 0.5 cos(2 pi k / (samples + 1)), k = 1 .. samples; the 200-point transform of the
 * windowed row WHATEVER samples is -- a row of more than 200 samples is truncated to its first 200 windowed samples, a shorter one
 * zero-padded; band p = (1,4), (4,8), (8,14), (14,31), (31,99) Hz is the mean of |X[j]|^2 over bins int(fStart / fs * 200) - 1 ..
 * int(fEnd / fs * 200) - 1 (at fs = 200: 0..3, 3..7, 7..13, 13..30, 30..98; the bands overlap); psd = that mean E, de = log2(100 E).
 * de, psd: [B][windows][electrodes][5] fp32, either may be NULL, not both.  de_mean, de_scale: device [electrodes * 5] fp32, both or
 * neither NULL: the per-feature scaler (de - mean) / scale applied to de on the way out, true division -- the StandardScaler of
 * train_semantic_predictor.py:46-47 over the 310 features of a window.
 * The one deviation: a band with E = 0 (an all-zero row) gives psd 0 and de -inf; the reference raises ValueError in math.log there.
 * ARITHMETIC IS FP32 IN EVERY COMPUTE MODE (tables made in double on the host, sums in index order): a row's bits depend on the row,
 * samples and fs alone, not on B, its place in the batch or the compute dtype.
 * Checked before anything is enqueued, in this order: NULL eeg / no output / mean without scale / a pointer off 4-byte alignment /
 * negative stride / B < 1 / windows, electrodes, samples < 1 or samples > 65536 / an fs at which a band's first bin would be below 0
 * or its last above 99, where the reference indexes from the end of the spectrum or past its half (fs = 100 and fs = 256 do):
 * E2V_EINVAL; then a host-only context: E2V_ESTATE.
 * Stream-ordered, does not synchronise, allocates nothing once one call has been made. */
e2v_status e2v_eeg_de_psd(e2v_ctx* ctx, const float* eeg, int64_t clip_stride, int64_t window_stride, int64_t channel_stride, int B,
                          int windows, int electrodes, int samples, int fs, const float* de_mean, const float* de_scale, float* de,
                          float* psd, e2v_stream stream);

/* rank 10 -- replaces glfnet.forward in eval mode (EEG2Video/models/models.py:352-373), whose fast / slow label selects DANA's
 * dynamic_beta.  eeg: device fp32, 4-byte aligned; sample t of electrode c of clip b is eeg[b clip_stride + c channel_stride + t] (element
 * strides, non-negative): a contiguous [B][electrodes][samples] is (electrodes samples, samples); the first 200 samples of a raw 2-s
 * segment [B][62][400] are (24800, 400).  The occipital net reads its electrodes of the same clip through the stride.
 * in_mean, in_scale: device [electrodes][samples] fp32, both or neither NULL: the input scaler (x - mean) / scale applied as a value
 * is read, true division.  logits [B][raw_out] fp32; features [B][2 emb] fp32, the concatenated embeddings the head reads; labels [B]
 * int32, argmax of the logits (the lowest index among equal maxima).  Any of the three may be NULL, not all.
 * ARITHMETIC IS FP32 IN EVERY COMPUTE MODE; a clip's bits do not depend on B or on its place in the batch.
 * Checked before anything is enqueued, in this order: NULL eeg / no output / mean without scale / a pointer off 4-byte alignment /
 * negative stride / B < 1: E2V_EINVAL; then no GLMNet config, no raw model in it, part 256 not finalized, host-only context: E2V_ESTATE.
 * Stream-ordered, does not synchronise, allocates nothing once the workspace of a B is cached. */
e2v_status e2v_glmnet_raw(e2v_ctx* ctx, const float* eeg, int64_t clip_stride, int64_t channel_stride, int B, const float* in_mean,
                          const float* in_scale, float* logits, float* features, int32_t* labels, e2v_stream stream);
/* rank 10 -- replaces glfnet_mlp.forward (EEG2Video/models/models.py:375-413).  de: device [B][electrodes][bands] fp32, 4-byte aligned,
 * for instance the output of e2v_eeg_de_psd for one window.  logits [B][mlp_out], features [B][2 emb], labels [B] as e2v_glmnet_raw;
 * the same arithmetic contract, checks (NULL de / no output / alignment / B < 1, then the state) and stream behaviour. */
e2v_status e2v_glmnet_mlp(e2v_ctx* ctx, const float* de, int B, float* logits, float* features, int32_t* labels, e2v_stream stream);

/* rank 2 -- replaces Diffusion.forward of DANA (EEG2Video/models/DANA_module.py:52-72) given its random draws, fused with
 * the latent layout fix 'a b c d e -> a c b d e' of inference_eeg2video.py:77,82:
 *   out[b,c,f] = sqrt(abar_t_b) x0[b,f,c] + sqrt(1 - abar_t_b) (sqrt(1 - beta) eps_div[b,f,c] + sqrt(beta) eps_same[b,0,c])
 * x0, eps_div [B,F,C,H,W]; eps_same [B,1,C,H,W]; host_t int64 [B] in [0, time_steps); linear betas 1e-4 .. 0.02 over
 * time_steps (:42-52); out [B,C,F,H,W] (the pipeline's latent layout). */
e2v_status e2v_dana_noise(e2v_ctx* ctx, const float* x0, const float* eps_div, const float* eps_same,
                          const int64_t* host_t, int time_steps, float dynamic_beta, int B, int F, int C, int H, int W,
                          float* out, e2v_stream stream);

/* rank 3 -- replaces `(x * 255).numpy().astype(np.uint8)` of save_videos_grid (EEG2Video_New/Generation/tuneavideo/
 * util.py:29) on the device, so that frames cross xGMI / PCIe as 1 byte per sample: videos in [0,1] -> uint8. */
e2v_status e2v_frames_to_uint8(e2v_ctx* ctx, const float* videos, uint8_t* out, int64_t count, e2v_stream stream);

/* rank 5 -- replaces ssim_metric / mse_metric and the per-frame loops ssim_score_only / mse_score_only around them
 * (EEG2Video/40_class_run_metrics.py:201-233: skimage.metrics.structural_similarity(img1, img2, data_range=255, channel_axis=-1)
 * and mse_loss(img1 / 255, img2 / 255) of each generated frame against its ground-truth frame), on the device, where the frames are.
 * a, b: two batches of n clips, n * F images with C channels, H x W.  `kind` = type | layout bit, chosen per input: E2V_FRAMES_F32 (fp32,
 * 4-byte aligned) or E2V_FRAMES_U8 (bytes of ANY alignment: slices of a gathered buffer, odd W * C); layout bit clear: planar
 * [n,C,F,H,W], the library's `videos`; E2V_FRAMES_CHANNELS_LAST: [n,F,H,W,C], what imageio.mimread and the reference stack.
 * ssim, mse: device [n,F] fp32 each, entry (i, f) = the score of image f of clip i; either may be NULL, not both.
 * Quantisation: a u8 input is used as it is; an fp32 input is quantised once at load, q = (uint8)(min(max(x, 0), 1) * 255.f)
 * (truncation: the bytes of e2v_frames_to_uint8 on [0,1]; NaN -> 0).  Everything after that is defined on the bytes.
 * SSIM per image and channel, skimage's defaults as the reference calls it: 7x7 uniform window, sample covariance (NP / (NP - 1)),
 * K1 = 0.01, K2 = 0.03, L = 255, the map cropped by 3 on every side (only windows fully inside the image count: no border rule),
 * the mean over the (H-6)(W-6) map per channel, then over the channels.  Window moments are exact integers: with N = 49 and
 * Sx, Sy, Sxx, Syy, Sxy over the window,
 *   A1 = 2 Sx Sy / N^2 + C1,  A2 = 2 (N Sxy - Sx Sy) / (N (N-1)) + C2,  B1 = (Sx^2 + Sy^2) / N^2 + C1,
 *   B2 = (N (Sxx + Syy) - Sx^2 - Sy^2) / (N (N-1)) + C2,  S = A1 A2 / (B1 B2),  C1 = 6.5025, C2 = 58.5225;
 * every integer fits int32; the four terms and S are fp32, S is summed in double and rounded to fp32 once, after the division by the
 * count.  Identical inputs give exactly 1; the result is symmetric in (a, b) bit for bit.
 * MSE per image: sum (qa - qb)^2 / (65025 C H W) over ALL pixels, the border included; the integer sum is exact (64-bit), divided in
 * double and rounded to fp32 once -- the reference's mse_loss without its per-element fp32 roundings.
 * Fixed reduction order: per-workgroup partials in a workspace-pool block, summed per image in index order by a second kernel, no
 * atomics -- an image's result does not depend on n or on its position in the batch and is bit-identical from run to run.
 * Stream-ordered, does not synchronise, allocates nothing once the partials block of a shape is cached (e2v_device_bytes does not move).
 * The argument checks come before anything is enqueued and before the host-only check: null ctx / a / b, both outputs NULL or unknown
 * bits in a kind E2V_EINVAL; n or F <= 0 E2V_ESHAPE; C outside 1..4 E2V_ESHAPE; H or W < 7 E2V_ESHAPE ("window exceeds the image",
 * where skimage raises); a well-formed call on a host-only context: E2V_ESTATE. */
enum { E2V_FRAMES_F32 = 0, E2V_FRAMES_U8 = 1, E2V_FRAMES_CHANNELS_LAST = 2 };   /* kind = type | layout bit */
e2v_status e2v_frame_metrics(e2v_ctx* ctx, const void* a, int a_kind, const void* b, int b_kind,
                             int n, int F, int C, int H, int W, float* ssim, float* mse, e2v_stream stream);

/* rank 6 -- replaces the classifier half of img_classify_metric (EEG2Video/40_class_run_metrics.py:86-98, called per clip at :302-328):
 * ViTImageProcessor(images=frame) and ViTForImageClassification(...).logits of every frame, its softmax and the indices of the three
 * largest logits (`.argsort(-1)[-3:]`, :97), on the device, where the frames are -- one call for a whole batch of clips instead of one
 * fp16 forward per image.  The N-way trial loop on top of it (n_way_top_k_acc, :57-70) stays on the host: eeg2video_amd/metrics.py.
 * frames, kind: as e2v_frame_metrics -- E2V_FRAMES_F32 (4-byte aligned) or E2V_FRAMES_U8 (bytes of ANY alignment), planar [n,3,F,H,W]
 * or, with E2V_FRAMES_CHANNELS_LAST, [n,F,H,W,3].  An fp32 input is quantised to the bytes of e2v_frames_to_uint8 first (clamped to
 * [0,1], NaN -> 0); everything after that is defined on bytes.
 * Preprocess: Pillow's Image.resize((S, S), BILINEAR) with S = vit_image_size -- the two-pass antialiased triangle filter in 22-bit
 * fixed point, horizontal pass first, the intermediate rounded to bytes (e2v_image_resize_table of eeg2video_hip_ops.h is one axis of
 * it) -- then the pixel value of the config (vit_rescale, vit_mean, vit_std), bit-identical to ViTImageProcessor on Pillow 12.
 * Model: patch embedding, class token, position embeddings, vit_layers pre-LN encoder layers (non-causal attention, head dim 64,
 * erf GELU), the final LayerNorm on the class row, the classifier.  ARITHMETIC IS FP32 IN EVERY COMPUTE MODE, as e2v_text_encode:
 * the same frames give the same bits under E2V_F32, E2V_BF16, E2V_F16 and E2V_F32X3 contexts.  (The reference runs the model in fp16.)
 * Outputs, per image in n * F order (image f of clip i at i * F + f), device, 4-byte aligned, any two may be NULL but not all three:
 *   logits [n*F][vit_num_labels];  probs [n*F][vit_num_labels], the fp32 softmax of the logits;
 *   top3 [n*F][3] int32, the indices of the three largest logits in ASCENDING order of logit -- what argsort(-1)[-3:] gives; equal
 *   logits rank as a stable ascending sort ranks them (the larger index counts as larger; -0 equals +0).
 * Large n * F is walked in chunks of images; the result of an image does not depend on the chunking, on n or on its neighbours, and is
 * bit-identical from run to run.  Stream-ordered, does not synchronise, allocates nothing outside the workspace pool (and nothing
 * once the blocks of a shape are cached: e2v_device_bytes does not move).
 * The argument checks come before anything is enqueued and before the state checks: null ctx / frames, all three outputs NULL, a
 * misaligned output, unknown bits in kind, n < 1: E2V_EINVAL; F, H or W < 1, or a downscale so strong that one output row's source
 * rows do not fit the preprocess kernel's LDS band (48 KiB: H / S beyond about 100 at S = 224): E2V_ESHAPE.  Then: no classifier in
 * the config (vit_layers = 0), the part not finalized, or a host-only context: E2V_ESTATE. */
e2v_status e2v_image_classify(e2v_ctx* ctx, const void* frames, int kind, int n, int F, int H, int W,
                              float* logits, float* probs, int32_t* top3, e2v_stream stream);

/* rank 7 -- replaces the classifier half of video_classify_metric (EEG2Video/40_class_run_metrics.py:108-142, called per clip at
 * :332-374): VideoMAEImageProcessor(list of frames) and VideoMAEForVideoClassification(...).logits of every CLIP, its softmax and the
 * indices of the three largest logits, on the device -- one call for a batch of clips instead of one fp16 forward per clip.
 * frames, kind: as e2v_image_classify.  F must equal vmae_num_frames.
 * Preprocess: Pillow's Image.resize((nw, nh), BILINEAR) with the SHORTEST edge at vmae_resize_edge = E and the aspect ratio kept --
 * (nh, nw) = (E, int(E * W / H)) for H <= W, else (int(E * H / W), E) --, of which only the centre crop of S x S (S = vmae_image_size;
 * rows top .. top + S - 1, top = (nh - S) / 2, columns left = (nw - S) / 2 likewise) is computed, then the pixel value of the config;
 * bit-identical to VideoMAEImageProcessor on Pillow 12.
 * Model: the tubelet embedding (a Conv3d of kernel and stride (ts, P, P): frames 2t and 2t + 1 of a clip feed token (t, py, px)), the
 * caller's position table added, vmae_layers pre-LN encoder layers (non-causal attention over all T tokens of a clip, head dim 64, erf
 * GELU), the mean over the tokens, fc_norm (eps 1e-5), the classifier.  FP32 IN EVERY COMPUTE MODE.
 * Outputs, per CLIP, device, 4-byte aligned, any two may be NULL but not all three: logits, probs [n][vmae_num_labels], top3 [n][3]
 * int32 (ascending order of logit, ties as a stable sort: as e2v_image_classify).
 * Clips are walked in chunks; a clip's result does not depend on the chunking, on n, on its position, on the compute mode or on the
 * run.  Stream-ordered, does not synchronise, allocates nothing outside the workspace pool (nothing once a shape's blocks are cached).
 * Errors, in this order: null ctx / frames, all outputs NULL, misaligned, unknown bits in kind, n < 1: E2V_EINVAL; F !=
 * vmae_num_frames (with a video config), H or W < 1, or a downscale whose band does not fit the preprocess kernel's LDS: E2V_ESHAPE;
 * no video classifier in the config, the part not finalized, or a host-only context: E2V_ESTATE. */
e2v_status e2v_video_classify(e2v_ctx* ctx, const void* frames, int kind, int n, int F, int H, int W,
                              float* logits, float* probs, int32_t* top3, e2v_stream stream);

/* rank 8 -- replaces the model half of the CLIP score (EEG2Video/40_class_run_metrics.py:20-55: the clip_score class, called per
 * frame pair by clip_score_only :176-188 and per comparison by n_way_scores :145-174): CLIPImageProcessor(image) and
 * CLIPVisionModelWithProjection(...).image_embeds of every frame, on the device -- one call for a batch of frames instead of one
 * fp16 forward per image of every comparison.
 * frames, kind: as e2v_image_classify.  embeds [n*F][clipv_projection_dim] fp32 on the device, 4-byte aligned: the model's
 * image_embeds, NOT normalised (e2v_clip_similarity divides by the norms).
 * Preprocess: Pillow's Image.resize((nw, nh), clipv_resample) with the SHORTEST edge at clipv_resize_edge = E and the aspect ratio
 * kept -- (nh, nw) = (E, int(E * W / H)) for H <= W, else (int(E * H / W), E) --, of which only the centre crop of S x S
 * (S = clipv_image_size) is computed, then the pixel value of the config; bit-identical to CLIPImageProcessor on Pillow 12.
 * Model: the patch embedding (no bias), the class embedding, position embeddings, pre_layrnorm over every token row,
 * clipv_layers pre-LN encoder layers (non-causal attention, head dim 64, clipv_act), post_layernorm on the class row,
 * visual_projection (no bias).  FP32 IN EVERY COMPUTE MODE.
 * Images are walked in chunks; an image's embedding does not depend on the chunking, on n * F, on its position, on the compute mode
 * or on the run.  Stream-ordered, does not synchronise, allocates nothing outside the workspace pool.
 * Errors, in this order: null ctx / frames / embeds, misaligned, unknown bits in kind, n < 1: E2V_EINVAL; F, H or W < 1, or a
 * downscale whose band does not fit the preprocess kernel's LDS: E2V_ESHAPE; no vision tower in the context (e2v_create_clip_vision), the part not finalized,
 * or a host-only context: E2V_ESTATE. */
e2v_status e2v_clip_embed(e2v_ctx* ctx, const void* frames, int kind, int n, int F, int H, int W, float* embeds, e2v_stream stream);

/* The score half: torch.nn.functional.cosine_similarity(a, b, dim=-1) with its eps = 1e-8,
 * dot(a, b) / (max(|a|, eps) * max(|b|, eps)), of fp32 rows on the device.  a [na][D], b [nb][D], contiguous and 16-byte aligned,
 * D a positive multiple of 4 (any D: the rows need not come from e2v_clip_embed and the context needs no vision tower).
 * matrix = 0: na == nb, out[na], out[i] = cos(a[i], b[i]); matrix = 1: out[na][nb], out[i][j] = cos(a[i], b[j]).
 * fp32 products summed in a fixed order that depends on D alone, no atomics: out[i][j] of the matrix form carries the bits of the
 * pair form on (a[i], b[j]); a zero row gives 0, not NaN.  Stream-ordered, allocates nothing.
 * Errors: a null or misaligned pointer, matrix not 0 or 1: E2V_EINVAL; na or nb < 1, D < 4 or not a multiple of 4, na != nb in the
 * pair form, more than 65535 * 16 rows of a in the matrix form: E2V_ESHAPE; a host-only context: E2V_ESTATE. */
e2v_status e2v_clip_similarity(e2v_ctx* ctx, const float* a, int na, const float* b, int nb, int D, int matrix, float* out,
                               e2v_stream stream);

/* ---- multi-GPU: the one exchange of the path ------------------------------------------------------------------
 * replaces: nothing in the reference (it generates its 200 clips serially on one GPU, inference_eeg2video.py:90); clips shard
 * over one process per GPU with no data-path exchange, and the decoded frames of all ranks are gathered at the end.  The
 * library opens its own RCCL communicator: rank 0 draws an id (128 bytes, HOST memory), the host side ships it to the other
 * ranks by any channel it has, every rank calls e2v_comm_init (collective: returns when all `world` ranks have called it).
 * RCCL is resolved at run time from the librccl already in the process (else the ROCm one): E2V_ESTATE if there is none. */
e2v_status e2v_comm_unique_id(void* id128_host);
e2v_status e2v_comm_init(e2v_ctx* ctx, const void* id128_host, int rank, int world);
int e2v_comm_world(const e2v_ctx* ctx);                 /* 0: no communicator */
/* `frames`: this rank's `count` floats (e.g. [b,3,F,H,W], the same count on every rank); `out`: world * count elements, rank r's
 * shard at offset r * count -- fp32, or (as_uint8) the (x * 255) truncation save_videos_grid applies (tuneavideo/util.py:29), a
 * quarter of the xGMI bytes.  One ncclAllGather on `stream`; does not synchronise. */
e2v_status e2v_allgather_frames(e2v_ctx* ctx, const float* frames, int64_t count, int as_uint8, void* out, e2v_stream stream);
e2v_status e2v_comm_destroy(e2v_ctx* ctx);              /* also done by e2v_destroy */

/* Per-kernel-class timing with HIP events on the launch stream (used by bench.py for the roofline figures).
 * Between begin and end every kernel launch of the library is bracketed by an event pair and tagged with its
 * algorithmic flops / bytes.  e2v_profile_end synchronises and writes a JSON object
 * {"<kernel class>": {"launches": n, "ms": total, "flops": total, "bytes": total}, ...} into `json`
 * (NUL-terminated, truncated to `cap`); it returns the untruncated length or -1. */
e2v_status e2v_profile_begin(e2v_ctx* ctx);
int64_t e2v_profile_end(e2v_ctx* ctx, char* json, int64_t cap);

/* Arithmetic and storage of the graph's tensors: E2V_F32 (default; fp32 MFMA, fp32 activations, the parity configuration of
 * BASELINE configs[1]) or E2V_BF16 (BASELINE configs[2]: every tensor the graph stores between kernels is bf16 in HBM, bf16
 * MFMA with fp32 accumulation; what stays fp32: the latents / DDIM state, eps, the decoded frames, VAE moments and attention
 * scores, GroupNorm / LayerNorm statistics, softmax, the time-embedding MLP) or E2V_F16 (the same kernels on IEEE half --
 * v_mfma_f32_*_f16, fp16 rows in HBM, fp32 everything listed above: the reference's own inference arithmetic,
 * EEG2Video/inference_eeg2video.py:69-70,76,81 `torch_dtype=torch.float16`, pipelines/pipeline_tuneeeg2video.py:150; three more
 * mantissa bits than bf16 -- every block within 2e-3 of the fp32 oracle where bf16 sits at 1.6e-2 -- at fp16's range: a stored
 * activation beyond 65 504 becomes inf exactly where the reference's .half() run would).  The boundary tensors of this header are
 * fp32 in every mode.  Takes effect for the following calls (the fp16 weight copies are derived on first use).
 * E2V_F32X3 (opt-in, experimental): fp32 results from the bf16 matrix pipe -- every operand of a linear / Winograd-domain
 * GEMM is split exactly into three bf16 pieces and the six significant piece products are accumulated in fp32 (error at
 * the level of the fp32 FMA chain); must be selected BEFORE e2v_finalize_weights (the weights are split there), else
 * E2V_ESTATE.  Also selectable with E2V_F32X3=1 in the environment at e2v_create.
 * The metric towers (e2v_image_classify, e2v_video_classify, e2v_clip_embed) and the text encoder do NOT follow this switch: the
 * towers have their own (e2v_set_tower_dtype, fp32 by default), the text encoder is fp32 always. */
e2v_status e2v_set_compute_dtype(e2v_ctx* ctx, int dtype);

/* Arithmetic of ONE metric tower -- part 16 (e2v_image_classify), 32 (e2v_video_classify) or 64 (e2v_clip_embed) -- whatever
 * e2v_set_compute_dtype says.  E2V_F32 (default): the fp32 path, bit for bit what it was before any switch.  E2V_BF16 / E2V_F16: the
 * reference's own arithmetic for these models (EEG2Video/40_class_run_metrics.py:41,50-51 / :89,97-98 / :125,134-135:
 * `.to(device, torch.float16)`).  One rounding rule for the three towers:
 *   - the preprocess keeps Pillow's integer arithmetic and the fp32 pixel table and rounds each value once, storing the patch rows;
 *   - the token rows live in HBM as 16-bit: patch / tubelet linear and the encoder linears are 16-bit MFMA with fp32 accumulation,
 *     fp32 bias and residual added before the single store rounding; the class row and positions are added in fp32; LayerNorm has
 *     fp32 statistics (the tower's eps); GELU / quick-GELU is computed in fp32 on 16-bit storage; attention keeps scores and softmax
 *     fp32, the probabilities and the output are 16-bit;
 *   - the head is fp32: the final / post / fc_norm LayerNorm reads 16-bit rows (VideoMAE: the fp32 mean over the 16-bit token rows,
 *     summed in index order) and writes fp32, the classifier / projection, softmax, top 3 and e2v_clip_similarity are unchanged.
 * The outputs keep their fp32 types and shapes.  An image's or clip's bits depend on neither the batch, its position, the chunking,
 * the context's compute dtype nor the run, as in fp32.  The 16-bit copies of the tower's matrices are derived from the fp32 ones on
 * the first call in that mode and KEPT when the mode changes (freed when the part is finalized again); e2v_update_tensor refreshes
 * every copy that exists, e2v_op_weight_forms reports them, e2v_read_tensor reads them (E2V_FORM_BF16 / E2V_FORM_F16).
 * May be called before or after e2v_finalize_weights, and repeatedly; takes effect for the following calls.  In a 16-bit mode the
 * patch row length (3 P^2, VideoMAE 3 ts P^2) and the intermediate width must be multiples of 8, else the call answers E2V_ESHAPE.
 * E2V_EINVAL: a null ctx, any other part (8, the text encoder, included), E2V_F32X3 or an unknown dtype.  E2V_ESTATE: the context
 * has no such tower.  No HIP call: a host-only context answers too. */
e2v_status e2v_set_tower_dtype(e2v_ctx* ctx, int part, int dtype);
/* the dtype a tower is set to (E2V_F32 / E2V_BF16 / E2V_F16); -1 for a null ctx or a part that is not 16, 32 or 64 */
int e2v_tower_dtype(const e2v_ctx* ctx, int part);

/* Algorithm of the stride-1 3x3 convolutions in fp32 arithmetic.  E2V_CONV_AUTO (default): Winograd F(4x4,3x3) -- 4x
 * fewer matrix-core flops than the direct implicit GEMM -- where min(Cin, Cout) >= 128 and the map padded to multiples of
 * 4 grows by at most 1.7x, else F(2x2,3x3) (2.25x fewer) where min(Cin, Cout) >= 256, else direct.  Measured deviation
 * of a full 50-step B = 8 generate from the all-direct result: frames 1.4e-5 (F(2x2) only: 5.8e-6), against the 1e-3
 * parity tolerance.  E2V_CONV_DIRECT / E2V_CONV_WINOGRAD / E2V_CONV_WINOGRAD4 force one form wherever it applies.
 * The Winograd-domain weights are made by e2v_finalize_weights, so for the graph entry points call this BEFORE finalizing;
 * the kernel-level e2v_op_conv3x3 follows it immediately.  (The reference leaves this choice to cuDNN: F.conv2d,
 * resnet.py:24-31.) */
enum { E2V_CONV_AUTO = 0, E2V_CONV_DIRECT = 1, E2V_CONV_WINOGRAD = 2, E2V_CONV_WINOGRAD4 = 3 };
e2v_status e2v_set_conv_algo(e2v_ctx* ctx, int algo);

/* bytes of device memory currently held by the ctx (weights + cached workspace) */
int64_t e2v_device_bytes(const e2v_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* EEG2VIDEO_HIP_H */
