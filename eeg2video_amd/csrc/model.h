// The model graphs of the hot path, run as sequences of gfx950 kernel launches on one stream:
// UNet3DConditionModel.forward (unet.py:278-413), AutoencoderKL encode/decode (diffusers 0.11.1,
// SURVEY App. C.5) and the DDIM denoising loop of TuneAVideoPipeline.__call__
// (pipeline_tuneeeg2video.py:287-334).
#pragma once
#include <array>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "kernels.h"
#include "runtime.h"

namespace e2v {

struct NormW { const float* g = nullptr; const float* b = nullptr; int c = 0; };
struct LinW { const float* w = nullptr; const float* b = nullptr; int in = 0, out = 0;
              mutable const void* w16 = nullptr;   // the bf16 copy: made by finalize(), or -- the metric towers, whose finalize() keeps fp32 only -- on first use (e2v_ctx::lin_b16)
              const void* w3 = nullptr;         // three bf16 planes of w (out*in elements apart) for the f32x3 mode
              int in16 = 0;                     // row length of w16: `in` rounded up to 8 (zero columns; 16-byte DMA pieces)
              int part = 0;                     // which finalize() group owns the lazily built fp16 form
              mutable const void* w16h = nullptr; };   // the same matrix as IEEE half (fp16 mode), built on first use (e2v_ctx::lin_f16)
// A 3x3 conv keeps its torch-layout weight and builds the kernel layouts ON FIRST USE (e2v_ctx::conv_form): which of them a
// layer ever needs depends on the arithmetic mode and on the map size it is called with -- fp32 direct-packed, F(2x2) / F(4x4)
// Winograd-domain (x2.25 / x4 the raw size), bf16 direct-packed -- and building all of them cost 18 GiB where one mode uses 4-9.
struct ConvW {
    const float* raw = nullptr;                  // [O][I][3][3] fp32, as uploaded
    const float* b = nullptr;
    int cin = 0, cin_pad = 0, cout = 0;
    int ldw = 0, ldw16 = 0;                      // row lengths of the fp32 (32-channel chunks) / bf16 (64-channel chunks) packed forms
    int cin_pad16 = 0;                           // channels of the bf16 input: cin rounded up to 8
    int part = 0;                                // 0 UNet, 1 VAE: which finalize() group owns the lazily built forms
    mutable const float* w = nullptr;            // [O][chunk32][tap][32]
    mutable const void* w16 = nullptr;           // [O][chunk64][tap][64] bf16
    mutable const void* w16_up2 = nullptr;       // [4 parities][O][chunk64][4 taps][64] bf16: the sub-pixel form of resize + conv (bgemm_up2x)
    mutable const void* w16h = nullptr;          // the two 16-bit layouts as IEEE half (fp16 mode)
    mutable const void* w16h_up2 = nullptr;
    mutable const float* wino = nullptr;         // [16][O][I]
    mutable const float* wino4 = nullptr;        // [36][O][I]
    mutable const void* wino_x3 = nullptr; mutable const void* wino4_x3 = nullptr;   // three-plane bf16 splits (f32x3 mode)
};

struct ResW {
    NormW n1, n2;
    ConvW c1, c2;
    LinW temb;        // w == nullptr: no time embedding (VAE)
    LinW sc;          // w == nullptr: identity shortcut
    int cin = 0, cout = 0;
};

struct TransW {
    NormW norm, ln1, ln2, ln3, lnt;
    LinW proj_in, proj_out;
    LinW a1_qkv, a1_out;            // sparse-causal self-attention, fused [3C][C]
    LinW a2_q, a2_kv, a2_out;       // cross-attention, fused [2C][cross]
    LinW ff1, ff2;                  // ff1 rows interleaved [32 value | 32 gate] for the GEGLU epilogue
    LinW at_qkv, at_out;            // temporal attention
    int C = 0;
};

struct UNetW {
    ConvW conv_in, conv_out;
    LinW te1, te2;
    NormW norm_out;
    struct Block {
        std::vector<ResW> res;
        std::vector<TransW> attn;       // empty for DownBlock3D / UpBlock3D
        bool resample = false;
        ConvW rs;                       // downsampler / upsampler conv
    };
    std::vector<Block> down, up;
    ResW mid_r0, mid_r1;
    TransW mid_attn;
};

struct VAEAttnW { NormW norm; LinW qkv, proj; int C = 0; };
struct VAEW {
    struct Block { std::vector<ResW> res; bool resample = false; ConvW rs; };
    // decoder
    LinW post_quant;
    ConvW dec_in, dec_out;
    ResW dec_mid0, dec_mid1;
    VAEAttnW dec_attn;
    std::vector<Block> dec_up;
    NormW dec_norm_out;
    // encoder
    LinW quant;
    ConvW enc_in, enc_out;
    ResW enc_mid0, enc_mid1;
    VAEAttnW enc_attn;
    std::vector<Block> enc_down;
    NormW enc_norm_out;
};

// CLIPTextModel (transformers: the text tower of SD-v1-4, keys "text.text_model...."): fp32 matrices only, in every compute mode.
// The metric towers (parts 16 / 32 / 64) share the packing; finalize() gives them fp32 matrices too, and a tower switched to a 16-bit
// mode (e2v_set_tower_dtype) derives the bf16 / fp16 copy of each matrix on first use (LinW::w16 / w16h).
struct TextLayerW { NormW ln1, ln2; LinW qkv, out, fc1, fc2; };      // qkv: q_proj | k_proj | v_proj fused [3C][C] with its [3C] bias
struct TextW {
    const float* tok = nullptr; const float* pos = nullptr;          // [vocab][C], [max_positions][C]
    std::vector<TextLayerW> layers;
    NormW ln_f;
};

// A frame-input metric tower: the text tower's layer packing -- fp32 matrices only, q | k | v fused -- behind a patch embedding.
//   image  ViTForImageClassification (transformers; keys "image.vit....", "image.classifier...."): a class token, the final LayerNorm
//          and a classifier on the class row
//   video  VideoMAEForVideoClassification (keys "video.videomae....", "video.fc_norm.*", "video.classifier.*"): a tubelet embedding and
//          a fixed position table, no class token; the classifier reads fc_norm of the mean over the tokens
//   clipv  CLIPVisionModelWithProjection (keys "clipv.vision_model....", "clipv.visual_projection.weight"): a LayerNorm in front of the
//          layers, a patch embedding without bias, and a projection without bias in place of the classifier
struct VisionTowerW {
    const float* cls = nullptr;                                      // [C]; null: no class token
    const float* pos = nullptr;                                      // [T][C]
    LinW patch;                                                      // the patch / tubelet convolution as [C][3 (ts) P P]
    NormW pre_ln;                                                    // g == nullptr: none
    std::vector<TextLayerW> layers;
    NormW head_ln;                                                   // the final LayerNorm / fc_norm / post_layernorm
    LinW head;                                                       // [labels rounded up to 4][C] (the linear kernels store quads) / [projection_dim][C]
};

// The Seq2Seq latent model (the reference's myTransformer, my_autoregressive_transformer.py:123-192; keys "s2s." + its state-dict
// names): fp32 matrices only, every loaded tensor kept as it is.  nn.MultiheadAttention packs q | k | v as in_proj_weight [3C][C]: the
// self-attention uses it whole, the cross-attention as its rows 0 .. C - 1 (q, from the token) and C .. 3C - 1 (k | v, from the memory)
// -- two views of the one loaded block.
struct S2sEncLayerW { NormW ln1, ln2; LinW qkv, out, fc1, fc2; };
struct S2sDecLayerW { NormW ln1, ln2, ln3; LinW qkv, out, q2, kv2, out2, fc1, fc2; };
struct S2sW {
    const float* eegnet = nullptr;                                   // eegnet_pack (kernels.h): the convs with the three BatchNorms folded
    const float* pe = nullptr;                                       // [windows][C]
    LinW embed;                                                      // [C][F2 ((T / 4) / 8)]
    std::vector<S2sEncLayerW> enc;
    std::vector<S2sDecLayerW> dec;
    LinW txt;                                                        // [classes rounded up to 4][C]
    LinW pred;                                                       // [latent C h w][C]
};

// The GLMNet pair (the reference's glfnet and glfnet_mlp, EEG2Video/models/models.py:352-413; keys "glm.raw." / "glm.mlp." + their
// state-dict names): fp32 matrices only, every loaded tensor kept as it is.  Each model is a global and an occipital net and a head
// over the concatenated embeddings; either model may be absent (head.w == nullptr).
struct GlmNetW { const float* fold = nullptr; LinW out; };              // shallownet: shallownet_fold (kernels.h) and the linear behind the flatten
struct GlmMlpW { LinW l1, l2, l3; int in = 0; };                        // mlpnet: l1's K padded to a multiple of 4 (zero columns)
struct GlmW {
    GlmNetW raw_global, raw_occ; LinW raw_head;                         // heads: [out rounded up to 4][2 emb]
    GlmMlpW mlp_global, mlp_occ; LinW mlp_head;
};

// Where one raw state-dict tensor lives in the packed world of a finalized part (recorded by finalize(), used by e2v_update_tensor):
//   RAW   the fp32 block the kernels read -- norm affines, plain biases (the uploaded block itself), a slice of a fused bias, the
//         GEGLU bias (32-element groups interleaved);
//   LIN   rows of a LinW: the whole matrix (plain linear / 1x1 conv, K-padded first layer of the Semantic Predictor), a row range
//         of a fused one (a1_qkv, a2_kv, at_qkv, the VAE's qkv) or the GEGLU interleave of ff1 -- every form the LinW holds;
//   CONV  a 3x3 conv: ConvW::raw, from which each layout that has been built is derived again.
struct WBind {
    enum Kind { RAW, LIN, CONV } kind = RAW;
    const void* anchor = nullptr;    // LinW::w / ConvW::raw of the owner as finalize() made it; resolved to `lin` / `conv` once the part is in place
    LinW* lin = nullptr;
    ConvW* conv = nullptr;
    float* dst = nullptr;            // RAW: destination
    int rows = 1, in = 0;            // the source viewed as a matrix
    int row_off = 0, half = 0, blk = 1;      // destination row map (kernels.h: WeightScatterArgs)
};

// The SMALL-BATCH dispatch family (16-bit modes), decided ONCE per API call and handed to the graph runner by value: the call runs at
// most 8 UNet samples (B <= 4 clips with their guidance pairs: the reference's clip-by-clip loop, inference_eeg2video.py:90-100, and
// a caller that batches a few clips; the boundary was measured -- B = 3 / 4 gain 7 / 4 %, B = 5 / 6 / 8 2.4 / 1.7 / 0.5 %:
// profiles/r05_family_boundary.json).  Launches that would leave most of the chip idle then take split-K (kernels.h: IgemmArgs::sk)
// -- another summation order, so bit-identity across batch sizes holds WITHIN a family (B >= 5: every kernel choice is a
// bit-identical alternative; B <= 4: held to the oracle bounds).
int small_family_clips();      // the boundary E2V_SMALL_FAMILY_CLIPS, read live (an A/B; 0: the large family at every batch -- the parity tests hold BOTH families to the oracle with one clip)
inline bool unet_small_family(int N) { return N <= 2 * small_family_clips(); }   // in SAMPLES (ADVICE.md finding 3 would count clips)

// One 3x3 conv launch as the graph runner (Runner::conv3) and e2v_op_conv3x3 both describe it; the packed weight and the
// arithmetic-mode flags stay with the caller
struct Conv3 {
    const float* x0 = nullptr; int c0 = 0;       // channel-last sources (row stride = channels); x1: the concatenated skip
    const float* x1 = nullptr; int c1 = 0;
    int nimg = 0, Hs = 1, Ws = 1;                // images and their physical source map
    int Hi = 1, Wi = 1, Ho = 1, Wo = 1;          // logical input (after nearest resize) and output maps
    int stride = 1, pad = 0;
    int cout = 0; float* out = nullptr; const float* bias = nullptr;
    const float* rowbias = nullptr; int rb_ld = 0, rows_per_sample = 1;
    const float* resid = nullptr;
    int resized() const { return (Hi != Hs || Wi != Ws) ? 1 : 0; }      // nearest resize in front of the conv (Upsample3D)
    float ups_h() const { return (float)Hs / (float)Hi; }               // torch: scale = (float)input_size / output_size
    float ups_w() const { return (float)Ws / (float)Wi; }
};
IgemmArgs conv3_igemm(const Conv3& d);          // the geometry part of the direct form's arguments
// the Winograd form F(m x m, 3x3), workspace sizing and chunking included (U3: the f32x3 planes of U or null; gn_P > 0:
// GroupNorm's affine + SiLU from gn_scsh, slabs of gn_P rows, applied on the way in)
void conv3_wino(e2v_ctx* c, const Conv3& d, int m, const float* U, const void* U3, const float* gn_scsh, int gn_P, hipStream_t s);
// rows [value 0..half) | gate 0..half)] of w [2 half][in] and b [2 half] -> per 64: [32 value | 32 gate] (the GEGLU epilogue's layout)
void geglu_interleave(const float* w, const float* b, int half, int in, float* dw, float* db, hipStream_t s);
// ask for `want` split-K runs of launch g: where it is eligible the workspace is attached and returned (alive until the launch is queued)
Act splitk_attach(Pool& pool, IgemmArgs& g, int want);
// the tables of a preprocess plan (plan.words) in a pool block, copied on stream s: `plan` must live until the copy has run
Act upload_plan(Pool& pool, const PrepPlan& plan, hipStream_t s);

}  // namespace e2v

struct e2v_ctx {
    // THE part table.  A model part is one row: its slot (the enum: owned_part, alloc_part, ready), its bit of e2v_finalize_weights'
    // `which`, the prefix of its state-dict keys, what a context without it / a call before its finalize() is told, whether it is a
    // metric tower (e2v_set_tower_dtype), whether its linears keep fp32 matrices only (Packer::f32_only) and, where e2v_update_tensor refuses its keys, why.  has_part() (model.cpp) is the one
    // switch next to it: the config fields that say whether this context holds the part.
    enum Part { UNET, VAE, SEM, TEXT, IMAGE, VIDEO, CLIPV, S2S, GLM, N_PARTS };
    struct PartRow {
        int bit; const char* prefix; const char* absent; const char* not_ready; bool tower; bool f32_only; const char* frozen;
        bool owns(const std::string& k) const { return *prefix && k.rfind(prefix, 0) == 0; }
    };
    static constexpr PartRow kParts[N_PARTS] = {
        {1, "", nullptr, "UNet weights are not finalized", false, false, nullptr},
        {2, "vae.", nullptr, "VAE weights are not finalized", false, false, nullptr},
        {4, "semantic.", "the config has no semantic predictor", "semantic predictor weights are not finalized", false, false, nullptr},
        {8, "text.", "the config has no text encoder (text_layers = 0)", "text encoder weights are not finalized", false, true,
         "the text encoder is frozen on this path (train_finetune_videodiffusion.py:115); load a new one with e2v_load_tensor + e2v_finalize_weights"},
        {16, "image.", "the config has no image classifier (vit_layers = 0)", "image classifier weights are not finalized", true, true,
         "the image classifier is a frozen yardstick (40_class_run_metrics.py:88-90); load a new one with e2v_load_tensor + e2v_finalize_weights"},
        {32, "video.", "the config has no video classifier (vmae_layers = 0)", "video classifier weights are not finalized", true, true,
         "the video classifier is a frozen yardstick (40_class_run_metrics.py:113-118); load a new one with e2v_load_tensor + e2v_finalize_weights"},
        {64, "clipv.", "the context has no CLIP vision tower (e2v_create_clip_vision)", "CLIP vision tower weights are not finalized", true, true, nullptr},
        {128, "s2s.", "the context has no Seq2Seq latent model (e2v_create_ex)", "Seq2Seq weights are not finalized", false, true,
         "the Seq2Seq model is only called here and its BatchNorms are folded at finalize; load a new one with e2v_load_tensor + e2v_finalize_weights(ctx, 128)"},
        {256, "glm.", "the context has no GLMNet (e2v_create_ex2)", "GLMNet weights are not finalized", false, true,
         "the GLMNet models are only called here and their BatchNorms are folded at finalize; load new ones with e2v_load_tensor + e2v_finalize_weights(ctx, 256)"},
    };
    // which part owns a state-dict key: the one whose prefix it carries, else the UNet
    static Part key_part(const std::string& k) {
        for (int p = 0; p < N_PARTS; ++p)
            if (kParts[p].owns(k)) return (Part)p;
        return UNET;
    }
    static int tower_part(int bit) {                             // the API's 16 / 32 / 64 -> Part; -1: not a metric tower's bit
        for (int p = 0; p < N_PARTS; ++p)
            if (kParts[p].tower && kParts[p].bit == bit) return p;
        return -1;
    }
    bool has_part(Part p) const;                                 // does this context's config hold the part
    bool ready[N_PARTS] = {};                                    // finalize() has put the part in place
    void require_part(Part p) const { E2V_REQUIRE(has_part(p), E2V_ESTATE, kParts[p].absent); }
    void require_ready(Part p) const { E2V_REQUIRE(ready[p], E2V_ESTATE, kParts[p].not_ready); }

    e2v_config cfg;
    int device = 0;
    std::string err;
    std::vector<std::string> keys;                               // expected keys, in state-dict order
    std::unordered_map<std::string, e2v::WTensor> raw;           // uploaded tensors (torch layout)
    e2v::Pool pool;
    e2v::GuardTally guard_tally;                                 // E2V_POOL_GUARD (runtime.h): the tally of this context
    e2v_ctx() { pool.bind(&last_stream, &guard_tally); }
    e2v_ctx(const e2v_ctx&) = delete;
    e2v_ctx& operator=(const e2v_ctx&) = delete;
    e2v::UNetW unet;
    e2v::VAEW vae;
    e2v::TextW text;
    e2v::VisionTowerW image, video, clipv;
    e2v::S2sW s2s;
    e2v::GlmW glm;
    float image_lut[3 * 256] = {};                               // the processor's pixel value of a byte, per channel (e2v_create)
    float video_lut[3 * 256] = {};                               // the same for the video classifier
    e2v_clipv_config vcfg = {};                                  // the CLIP vision tower's config (e2v_create_clip_vision); all zero: none
    float clipv_lut[3 * 256] = {};                               // and for the CLIP vision tower's processor (bicubic tables)
    std::map<std::array<int, 3>, e2v::PrepPlan> prep_plans;      // host resize tables of a tower's preprocess per (part, H, W): prep_cached (model.cpp)
    const e2v::PrepPlan& prep_plan(Part tower, int H, int W);    // IMAGE, VIDEO or CLIPV, by the tower's config and pixel table
    e2v_s2s_config scfg = {};                                    // the Seq2Seq model's config (e2v_create_ex); all zero: none
    int s2s_features() const { return scfg.s2s_f2 * ((scfg.s2s_samples / 4) / 8); }     // the EEGNet embedding's flattened width
    int s2s_latent() const { return scfg.s2s_latent_channels * scfg.s2s_latent_h * scfg.s2s_latent_w; }
    std::map<std::array<int, 2>, std::vector<float>> de_psd_plans; // host Hann row and twiddles of e2v_eeg_de_psd per row length: prep_cached (model.cpp)
    const std::vector<float>& de_psd_plan(int samples);
    e2v_glm_config gcfg = {};                                    // the GLMNet pair's config (e2v_create_ex2); all zero: none
    int glm_columns() const { return e2v::shallownet_columns(gcfg.glm_samples, gcfg.glm_taps, gcfg.glm_pool, gcfg.glm_pool_stride); }
    int glm_raw_features() const { return gcfg.glm_filters * glm_columns(); }      // width of a shallownet's flattened maps (the reference's 1040)
    int conv_algo = 0;                                           // e2v_set_conv_algo: 0 auto, 1 direct, 2 / 3 Winograd F(2x2) / F(4x4) wherever it applies
    bool wino_f4 = true;                                         // auto: F(4x4,3x3) where min(Cin, Cout) >= wino4_min_c and the map, padded to
    int wino4_min_c = 128;                                       //   multiples of 4, grows by <= wino_f4_pad (E2V_WINO_F4 / _F4_MIN_C / _F4_PAD)
    double wino_f4_pad = 1.7;
    int wino_min_c = 256;                                        // auto: F(2x2,3x3) when min(Cin, Cout) >= this (E2V_WINO_MIN_C)
    size_t wino_ws_floats = (size_t)1 << 30;                     // workspace cap per pass (E2V_WINO_WS_MB)
    bool x3_compute = false;                                     // E2V_F32X3: fp32 products from split bf16 pieces on the bf16 MFMA
    bool bf16_compute = false;                                   // e2v_set_compute_dtype: a 16-bit activation mode (16-bit MFMA, 16-bit rows in HBM) ...
    int h16_mode = 0;                                            // ... and which: 0 none, 1 bf16 (E2V_BF16), 2 fp16 (E2V_F16) -- the flag every 16-bit launch carries (h16.h)
    void set_h16_mode(int m) { h16_mode = m; bf16_compute = m != 0; }
    // e2v_set_tower_dtype: the arithmetic of the three metric towers, each on its own and whatever the mode above -- 0 fp32 (the
    // default), 1 bf16, 2 fp16 (h16.h), indexed by Part (the towers' entries are the ones used)
    int tower_h16[N_PARTS] = {};
    std::vector<e2v::LinW> sem;                                  // semantic predictor layers (first one K-padded to 4)
    int sem_in_pad = 0;
    std::vector<float> alphas;                                   // host alpha-bar table
    e2v::GrowBuf gn_part, gn_scale;                              // GroupNorm workspaces (guarded under E2V_POOL_GUARD; not in weight_bytes)
    e2v::GrowBuf d_timesteps;                                    // int64 (or fp32) timesteps of the running call (never guarded)
    // per-generate caches of what does not depend on the latents: time_emb_proj(SiLU(emb(t_i))) of every resnet and step
    // ([steps][cout] each, call order) and to_k / to_v of the conditioning of every transformer ([N*T][2C] each)
    bool step_cache_on = false; int step_cache_step = 0;
    std::vector<e2v::Act> temb_cache, kv_cache;
    long long* timesteps(int n, hipStream_t s) { return static_cast<long long*>(d_timesteps.ensure(sizeof(long long) * n, 0, s)); }
    // the timestep of one UNet evaluation: integral (`t`, the int64 sinusoid path of e2v_unet_forward) or fractional (`tf`, the fp32
    // path of e2v_unet_forward_ft)
    struct EvalTime { int64_t t; float tf; bool frac; };
    void build_step_caches(const EvalTime* ev, int steps, const float* cond, int N, int T, bool small_family, hipStream_t s);

    // stream of the previous call (workspace reuse is stream-ordered): see enter_stream
    hipStream_t last_stream = nullptr; bool has_last_stream = false; hipEvent_t stream_ev = nullptr;
    void enter_stream(hipStream_t s);
    // device blocks made by dev_alloc, per part, so that finalizing a part again frees what it replaces
    std::vector<e2v::DevBlock> owned_part[N_PARTS];
    size_t weight_bytes() const;                                 // what the uploaded tensors and the parts' blocks hold (e2v_device_bytes)
    void* comm = nullptr; int comm_rank = 0, comm_world = 0;     // RCCL communicator of e2v_comm_init (comm.cpp)
    // e2v_op_unet_forward_taps (test aid): while set, unet_forward_cl copies the tensors the oracle exposes (emb, down0..3, mid,
    // up0..3) out as fp32 NCFHW, back to back; shapes = {n, C, F, H, W} per tap
    struct TapSink { float* buf = nullptr; int64_t cap = 0, used = 0; int count = 0; int64_t shapes[16][5]; };
    TapSink* tap_sink = nullptr;
    int alloc_part = -1;                                         // the part dev_alloc files its blocks under (every caller selects one)
    struct AllocPart {                                           // dev_alloc files under `part` for the guard's lifetime
        e2v_ctx* c; int saved;
        AllocPart(e2v_ctx* ctx, int part) : c(ctx), saved(ctx->alloc_part) { c->alloc_part = part; }
        ~AllocPart() { c->alloc_part = saved; }
    };
    void free_part(int part) { owned_part[part].clear(); }
    std::unordered_map<std::string, e2v::WBind> bind;            // raw key -> its place in the packed weights (keys of finalized parts)
    void resolve_bindings();
    // e2v_update_tensor: overwrite every existing form of `key` on stream s (data: [numel] of dtype, device or host)
    void update_tensor(const std::string& key, const void* data, e2v_dtype dtype, bool on_device, hipStream_t s);
    int weight_forms(const std::string& key);                    // e2v_op_weight_forms
    // e2v_read_tensor: where `form` (one of E2V_FORM_F32 / BF16 / F16 / X3) of `key` is read from -- chosen from the binding as
    // update_tensor chooses its destinations; throws for a form the binding kind cannot have or that is not built.  No HIP call.
    e2v::WeightGatherArgs read_source(const std::string& key, int form);
    // gather it into `out` ([numel] of dtype, device or host) in the torch layout, on stream s
    void read_tensor(const std::string& key, int form, void* out, e2v_dtype dtype, bool on_device, hipStream_t s);

    float* dev_alloc(size_t floats);
    enum ConvForm { FORM_DIRECT32, FORM_BF16, FORM_WINO2, FORM_WINO4, FORM_BF16_UP2, FORM_F16, FORM_F16_UP2 };
    const void* lin_f16(const e2v::LinW& w, hipStream_t s);              // the fp16 copy of a linear's weight (built on first use)
    const void* lin_b16(const e2v::LinW& w, hipStream_t s);              // the bf16 copy: finalize()'s, or built on first use (metric towers)
    void conv_form(const e2v::ConvW& w, ConvForm f, hipStream_t s);     // build the layout if this is its first use
    void conv_fill(const e2v::ConvW& w, ConvForm f, hipStream_t s);     // derive the (allocated) layout from w.raw: first use and weight updates
    // THE Winograd policy: the output tile a 3x3 conv of this shape runs with -- 0 direct, 2 F(2x2,3x3), 4 F(4x4,3x3)
    int conv_wino_tile(int cin, int cout, int stride, int pad, int Hi, int Wi, int Ho, int Wo) const;
    void expected_keys();
    void finalize(int which);
    // graphs (channel-last in/out); see model.cpp
    // cfg_pair: sample_cl holds N / 2 samples standing for the [x ; x] input of a classifier-free-guidance step
    // host_tf != null: fractional timesteps (fp32) instead of host_t
    e2v::Act unet_forward_cl(const float* sample_cl, const int64_t* host_t, int n_t, const float* cond, int N, int F,
                             int H, int W, int T, hipStream_t s, bool cfg_pair = false, const float* host_tf = nullptr);
    void vae_decode_frames(const float* z_cl, int nframes, int h, int w, float* out_cl3, hipStream_t s, bool small_family);
    void vae_encode_frames(const float* img_cl4, int n, int H, int W, float* moments_cl8, hipStream_t s);
    // the VAE mid-block attention between its qkv linear and its projection, as both graphs above run it (e2v_op_vae_attention_core):
    // qkv [nimg*HW][3C] fp32 -> out [nimg*HW][C]; scores / probs: fp32 [nimg*HW][HW] or null
    void vae_attention_core(const float* qkv, int nimg, int HW, int C, float* out, float* scores, float* probs, hipStream_t s);
    // CLIPTextModel.forward(input_ids)[0]: ids [B*T] int32 on the device (range-checked by the caller), out [B*T][text_hidden] fp32
    void text_encode(const int* ids, int B, int T, float* out, hipStream_t s);
    // ViTImageProcessor + ViTForImageClassification over images img0 .. img0 + nimg - 1 of `src` ([n][F] images of H x W), walked in
    // chunks; logits / probs [nimg][labels], top3 [nimg][3] (any may be null)
    void image_classify(const e2v::FrameSrc& src, int n, int F, int H, int W, float* logits, float* probs, int* top3, hipStream_t s);
    int image_tokens() const { const int g = cfg.vit_patch_size > 0 ? cfg.vit_image_size / cfg.vit_patch_size : 0; return g * g + 1; }
    // VideoMAEImageProcessor + VideoMAEForVideoClassification over the n clips of `src` ([n][F] frames of H x W, F = vmae_num_frames),
    // walked in chunks of clips; logits / probs [n][labels], top3 [n][3] (any may be null)
    void video_classify(const e2v::FrameSrc& src, int n, int F, int H, int W, float* logits, float* probs, int* top3, hipStream_t s);
    int video_tokens() const {
        const int g = cfg.vmae_patch_size > 0 ? cfg.vmae_image_size / cfg.vmae_patch_size : 0;
        return (cfg.vmae_tubelet_size > 0 ? cfg.vmae_num_frames / cfg.vmae_tubelet_size : 0) * g * g;
    }
    // CLIPImageProcessor + CLIPVisionModelWithProjection over the n * F frames of `src`, walked in chunks of images;
    // embeds [n*F][clipv_projection_dim]: image_embeds, not normalised
    void clip_embed(const e2v::FrameSrc& src, int n, int F, int H, int W, float* embeds, hipStream_t s);
    // myTransformer.forward in eval mode (see e2v_seq2seq_latents): tokens [first, first + count) of the steps + 1; any output may be null
    void seq2seq_latents(const e2v::EegnetArgs& eeg, int B, int first, int count, int layout, float* latents, float* txt_logits, float* tokens,
                         hipStream_t s);
    // glfnet / glfnet_mlp in eval mode (see e2v_glmnet_raw / e2v_glmnet_mlp); any output may be null
    void glmnet_raw(const e2v::ShallowArgs& eeg, int B, float* logits, float* features, int* labels, hipStream_t s);
    void glmnet_mlp(const float* de, int B, float* logits, float* features, int* labels, hipStream_t s);
    int clipv_tokens() const { const int g = vcfg.clipv_patch_size > 0 ? vcfg.clipv_image_size / vcfg.clipv_patch_size : 0; return g * g + 1; }
};
