// extern "C" surface of libeeg2video_hip.so (include/eeg2video_hip.h, include/eeg2video_hip_ops.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <unordered_map>
#include <mutex>

#include "../../include/eeg2video_hip_ops.h"
#include "h16.h"
#include "model.h"
#include "prof.h"

using namespace e2v;

namespace {

std::string g_create_error;

template <typename Fn>
e2v_status guarded(e2v_ctx* ctx, Fn&& fn) {
    try {
        if (ctx && !dry_run()) {                             // (a dry run -- e2v_op_describe_dispatch -- makes no HIP call)
            E2V_REQUIRE(ctx->device >= 0, E2V_ESTATE, "host-only context (device = -1): no GPU work possible");
            E2V_HIP(hipSetDevice(ctx->device));
        }
        fn();
        return E2V_OK;
    } catch (const Error& e) {
        if (ctx) ctx->err = e.what(); else g_create_error = e.what();
        return e.code;
    } catch (const std::exception& e) {
        if (ctx) ctx->err = e.what(); else g_create_error = e.what();
        return E2V_EINVAL;
    }
}

// The skeleton of an entry point that answers a malformed call on ANY context: a null context is E2V_EINVAL; `check` holds the
// argument and state checks and makes no HIP call, so a host-only context gets the same answer -- its Error's text and code; `run` is
// the work, under guarded().
template <typename Check, typename Run>
e2v_status entry(e2v_ctx* c, Check&& check, Run&& run) {
    if (!c) return E2V_EINVAL;
    try {
        check();
    } catch (const Error& e) {
        c->err = e.what();
        return e.code;
    }
    return guarded(c, run);
}

// the frames of an entry point as the kernels take them: `kind` is E2V_FRAMES_U8 | E2V_FRAMES_CHANNELS_LAST bits
FrameSrc frame_src(const void* frames, int kind) { return FrameSrc{frames, (kind & E2V_FRAMES_U8) == 0, (kind & E2V_FRAMES_CHANNELS_LAST) != 0}; }

float half_to_float(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000) << 16;
    uint32_t exp = (h >> 10) & 0x1F, man = h & 0x3FF, bits;
    if (exp == 0) {
        if (man == 0) bits = sign;
        else {
            exp = 127 - 15 + 1;
            while (!(man & 0x400)) { man <<= 1; --exp; }
            bits = sign | (exp << 23) | ((man & 0x3FF) << 13);
        }
    } else if (exp == 31) bits = sign | 0x7F800000u | (man << 13);
    else bits = sign | ((exp + 127 - 15) << 23) | (man << 13);
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

void make_alphas(e2v_ctx* c) {
    const int T = c->cfg.num_train_timesteps;
    c->alphas.resize(T);
    const float start = (float)std::sqrt(c->cfg.beta_start), end = (float)std::sqrt(c->cfg.beta_end);
    const float step = (end - start) / (float)(T - 1);
    float prod = 1.0f;
    for (int i = 0; i < T; ++i) {
        const float b = (i < T / 2) ? start + step * (float)i : end - step * (float)(T - i - 1);
        prod *= 1.0f - b * b;
        c->alphas[i] = prod;
    }
}

// Every entry point that enqueues work names its stream through here: the ctx's workspace cache hands a freed block to
// the next launch on the assumption that launches of one ctx are stream-ordered, so when a call arrives on a DIFFERENT
// stream than the previous one, the new stream is first made to wait for everything the old one was given.
hipStream_t S(e2v_ctx* c, e2v_stream s) {
    hipStream_t hs = static_cast<hipStream_t>(s);
    c->enter_stream(hs);
    return hs;
}

// Test aid (E2V_OP_RECORD, e2v_op_last_dispatch): for the length of one kernel-level entry point the launchers' dry_tag() texts are kept
// for the real launches too, in the calling thread's string, cleared here.  Switch off: one test of it, nothing else.
struct OpRecord {
    OpRecord() {
        static const int* const on = knob("E2V_OP_RECORD", 0);
        if (*on) { op_dispatch().clear(); op_recording() = true; }
    }
    ~OpRecord() { op_recording() = false; }
};
// An entry point that may refuse a call BEFORE its OpRecord exists (argument checks, a host-only context) starts the record afresh
// here: e2v_op_last_dispatch then says "" for the refused call, never the launches of an earlier one.
void op_record_reset() {
    static const int* const on = knob("E2V_OP_RECORD", 0);
    if (*on) op_dispatch().clear();
}

// Test aid (E2V_OP_IO16): e2v_op_linear / e2v_op_conv3x3 of a 16-bit context build the launch of Runner::linear / Runner::conv3
// (model.cpp) -- a 16-bit pool tensor of exactly M x N for the output, the residual converted to the type, out_f32 = 0, resid_bf16 = 1
// -- and widen the result into the caller's fp32 tensor afterwards.  Ignored in the fp32 and f32x3 modes.
bool op_io16(const e2v_ctx* c) {
    static const int* const on = knob("E2V_OP_IO16", 0);
    return c->bf16_compute && *on != 0;
}

}  // namespace

extern "C" {

void e2v_default_config(e2v_config* c) {
    std::memset(c, 0, sizeof(*c));
    c->in_channels = 4; c->out_channels = 4;
    const int boc[4] = {320, 640, 1280, 1280};
    std::memcpy(c->block_out_channels, boc, sizeof(boc));
    c->layers_per_block = 2; c->cross_attention_dim = 768; c->attention_heads = 8;
    c->norm_num_groups = 32; c->norm_eps = 1e-5f; c->flip_sin_to_cos = 1; c->freq_shift = 0.f;
    c->vae_in_channels = 3; c->vae_latent_channels = 4;
    const int vb[4] = {128, 256, 512, 512};
    std::memcpy(c->vae_block_out_channels, vb, sizeof(vb));
    c->vae_layers_per_block = 2; c->vae_norm_num_groups = 32; c->vae_norm_eps = 1e-6f; c->vae_scaling_factor = 0.18215;
    c->num_train_timesteps = 1000; c->beta_start = 0.00085; c->beta_end = 0.012; c->steps_offset = 1;
    c->sem_in_features = 310; c->sem_hidden = 10000; c->sem_tokens = 77;
}

}  // extern "C"

namespace {
// what e2v_create_clip_vision refuses (clipv_layers != 0), as the vit_* fields are checked
void check_clipv_config(const e2v_clipv_config* v) {
    E2V_REQUIRE(v->clipv_layers > 0 && v->clipv_heads > 0 && v->clipv_intermediate > 0 && v->clipv_intermediate % 4 == 0 &&
                    v->clipv_image_size > 0 && v->clipv_patch_size > 0 && v->clipv_projection_dim > 0 &&
                    v->clipv_projection_dim % 4 == 0 && (v->clipv_act == 0 || v->clipv_act == 1) && v->clipv_norm_eps > 0.f,
                E2V_EINVAL, "bad CLIP vision tower config (sizes must be positive, clipv_intermediate and clipv_projection_dim multiples of 4, "
                            "clipv_act 0 = quick_gelu or 1 = gelu)");
    E2V_REQUIRE(v->clipv_hidden == 64 * v->clipv_heads, E2V_EINVAL,
                "clipv_hidden must be 64 * clipv_heads: 64 is the head dim of the image attention kernel's only instance");
    E2V_REQUIRE(v->clipv_hidden % 4 == 0 && v->clipv_hidden <= 1280, E2V_EINVAL, "clipv_hidden must be a multiple of 4, at most 1280 (the LayerNorm kernel's limit)");
    E2V_REQUIRE(v->clipv_image_size % v->clipv_patch_size == 0 && (3 * v->clipv_patch_size * v->clipv_patch_size) % 4 == 0, E2V_EINVAL,
                "clipv_image_size must be a multiple of clipv_patch_size, and 3 * clipv_patch_size^2 a multiple of 4");
    const long long grid = v->clipv_image_size / v->clipv_patch_size;
    E2V_REQUIRE(grid * grid + 1 <= kImageAttnMaxT, E2V_EINVAL,
                "(clipv_image_size / clipv_patch_size)^2 + 1 tokens must be at most " + std::to_string(kImageAttnMaxT) +
                    ": the image attention kernel keeps K and V of an image's head in LDS");
    E2V_REQUIRE(v->clipv_resize_edge >= v->clipv_image_size && v->clipv_resize_edge <= 4096, E2V_EINVAL,
                "clipv_resize_edge must be at least clipv_image_size (the centre crop is taken from the resized frame) and at most 4096");
    E2V_REQUIRE(v->clipv_resample == kResizeBilinear || v->clipv_resample == kResizeBicubic, E2V_EINVAL,
                "clipv_resample must be 2 (BILINEAR) or 3 (BICUBIC), Pillow's codes");
    for (int ch = 0; ch < 3; ++ch) E2V_REQUIRE(v->clipv_std[ch] != 0.f, E2V_EINVAL, "clipv_std must be non-zero");
}
// what e2v_create_ex refuses of a Seq2Seq config (s2s_d_model != 0): each message names the limit it enforces
void check_s2s_config(const e2v_s2s_config* v) {
    E2V_REQUIRE(v->s2s_electrodes > 0 && v->s2s_samples > 0 && v->s2s_windows > 0 && v->s2s_f1 > 0 && v->s2s_d > 0 && v->s2s_f2 > 0 &&
                    v->s2s_d_model > 0 && v->s2s_heads > 0 && v->s2s_ffn > 0 && v->s2s_encoder_layers > 0 && v->s2s_decoder_layers > 0 &&
                    v->s2s_steps > 0 && v->s2s_latent_channels > 0 && v->s2s_latent_h > 0 && v->s2s_latent_w > 0 && v->s2s_txt_classes > 0 &&
                    v->s2s_norm_eps > 0.f && v->s2s_bn_eps > 0.f,
                E2V_EINVAL, "bad Seq2Seq config: every size and both eps must be positive");
    E2V_REQUIRE(v->s2s_d_model % v->s2s_heads == 0, E2V_EINVAL, "s2s_d_model must be a multiple of s2s_heads");
    const int hd = v->s2s_d_model / v->s2s_heads;
    E2V_REQUIRE(hd % 4 == 0 && hd <= 128, E2V_EINVAL,
                "s2s_d_model / s2s_heads must be a multiple of 4, at most 128: the head dims of the sequence attention kernel");
    E2V_REQUIRE(v->s2s_d_model % 4 == 0 && v->s2s_d_model <= 1280, E2V_EINVAL, "s2s_d_model must be a multiple of 4, at most 1280 (the LayerNorm kernel's limit)");
    E2V_REQUIRE(v->s2s_windows <= kSeqAttnMaxKeys && v->s2s_steps + 1 <= kSeqAttnMaxKeys, E2V_EINVAL,
                "s2s_windows and s2s_steps + 1 must be at most " + std::to_string(kSeqAttnMaxKeys) + ": the sequence attention kernel holds one key per lane of half a wave");
    E2V_REQUIRE(v->s2s_ffn % 4 == 0, E2V_EINVAL, "s2s_ffn must be a multiple of 4 (the linear kernels read and store quads)");
    E2V_REQUIRE(v->s2s_samples >= 32 && v->s2s_samples <= 65536 && v->s2s_electrodes <= 4096 && v->s2s_f1 <= 1024 && v->s2s_d <= 1024 && v->s2s_f2 <= 1024,
                E2V_EINVAL, "s2s_samples must be at least 32 (the two pools leave samples / 32 columns); sizes of the EEGNet embedding are bounded");
    const long long feat = (long long)v->s2s_f2 * ((v->s2s_samples / 4) / 8);
    E2V_REQUIRE(feat % 4 == 0, E2V_EINVAL, "s2s_f2 * ((s2s_samples / 4) / 8), the width of the EEGNet features, must be a multiple of 4");
    const EegnetLayout L = eegnet_layout(v->s2s_electrodes, v->s2s_samples, v->s2s_f1, v->s2s_d, v->s2s_f2);
    E2V_REQUIRE(L.total_floats * sizeof(float) <= (size_t)kEegnetMaxLdsBytes, E2V_EINVAL,
                "one EEG window with its intermediates must fit the embedding kernel's " + std::to_string(kEegnetMaxLdsBytes) + " bytes of LDS (this config: " +
                    std::to_string(L.total_floats * sizeof(float)) + ")");
    const long long lat = (long long)v->s2s_latent_channels * v->s2s_latent_h * v->s2s_latent_w;
    E2V_REQUIRE(lat % 4 == 0 && (v->s2s_latent_h * (long long)v->s2s_latent_w) % 4 == 0 && lat <= (1 << 24), E2V_EINVAL,
                "s2s_latent_h * s2s_latent_w must be a multiple of 4 (the linear and layout kernels store quads), a latent at most 2^24 values");
}
// what e2v_create_ex2 refuses of a GLMNet config (glm_raw_out or glm_mlp_out != 0): each message names the limit it enforces
void check_glm_config(const e2v_glm_config* v) {
    E2V_REQUIRE(v->glm_raw_out >= 0 && v->glm_mlp_out >= 0 && (v->glm_raw_out > 0 || v->glm_mlp_out > 0), E2V_EINVAL,
                "bad GLMNet config: glm_raw_out and glm_mlp_out are the widths of the two heads, 0 for an absent model, not both 0");
    E2V_REQUIRE(v->glm_electrodes > 0 && v->glm_samples > 0 && v->glm_occ_first >= 0 && v->glm_occ_count > 0 && v->glm_filters > 0 && v->glm_taps > 0 &&
                    v->glm_pool > 0 && v->glm_pool_stride > 0 && v->glm_bands > 0 && v->glm_hidden1 > 0 && v->glm_hidden2 > 0 && v->glm_emb > 0 &&
                    v->glm_bn_eps > 0.f,
                E2V_EINVAL, "bad GLMNet config: every size and the eps must be positive");
    E2V_REQUIRE(v->glm_electrodes <= 4096 && v->glm_samples <= 65536 && v->glm_filters <= 1024 && v->glm_taps <= 1024 && v->glm_pool <= 65536 &&
                    v->glm_bands <= 64 && v->glm_hidden1 <= 65536 && v->glm_hidden2 <= 65536 && v->glm_emb <= 65536 && v->glm_raw_out <= 65536 &&
                    v->glm_mlp_out <= 65536,
                E2V_EINVAL, "bad GLMNet config: sizes are bounded (electrodes 4096, filters and taps 1024, the rest 65536, bands 64)");
    E2V_REQUIRE((long long)v->glm_occ_first + v->glm_occ_count <= v->glm_electrodes, E2V_EINVAL,
                "the occipital electrodes glm_occ_first .. glm_occ_first + glm_occ_count - 1 must lie inside glm_electrodes");
    E2V_REQUIRE(v->glm_emb % 4 == 0 && v->glm_hidden1 % 4 == 0 && v->glm_hidden2 % 4 == 0, E2V_EINVAL,
                "glm_emb, glm_hidden1 and glm_hidden2 must be multiples of 4 (the linear kernels read and store quads)");
    if (v->glm_raw_out > 0) {
        const int cols = shallownet_columns(v->glm_samples, v->glm_taps, v->glm_pool, v->glm_pool_stride);
        E2V_REQUIRE(cols >= 1, E2V_EINVAL, "glm_samples must be at least glm_taps + glm_pool - 1: the pool has to leave one column");
        const long long width = (long long)v->glm_filters * cols;
        // the reference sizes its linear 1040 * (T // 200) whatever the pool leaves: only T = 200 .. 204 agree (T = 205 and T = 400 fail inside it)
        if (v->glm_filters == 40 && v->glm_taps == 25 && v->glm_pool == 51 && v->glm_pool_stride == 5)
            E2V_REQUIRE(width == 1040LL * (v->glm_samples / 200), E2V_EINVAL,
                        "at the reference's sizes glm_filters * pooled columns (" + std::to_string(width) + " at glm_samples = " + std::to_string(v->glm_samples) +
                            ") must equal the `out` linear's width 1040 * (glm_samples / 200) = " + std::to_string(1040LL * (v->glm_samples / 200)) +
                            ": samples 200 .. 204");
        E2V_REQUIRE(width % 4 == 0 && width <= (1 << 24), E2V_EINVAL,
                    "glm_filters * pooled columns, the `out` linear's width, must be a multiple of 4 (the linear kernels read quads), at most 2^24");
        E2V_REQUIRE(shallownet_lds_bytes(v->glm_electrodes, v->glm_samples, v->glm_taps) <= (size_t)kShallowMaxLdsBytes, E2V_EINVAL,
                    "one clip glm_electrodes x glm_samples with a filter group's columns must fit the ShallowNet kernel's " + std::to_string(kShallowMaxLdsBytes) +
                        " bytes of LDS (this config: " + std::to_string(shallownet_lds_bytes(v->glm_electrodes, v->glm_samples, v->glm_taps)) + ")");
    }
}
}  // namespace

extern "C" {

int64_t e2v_config_size(void) { return (int64_t)sizeof(e2v_config); }

const char* e2v_version(void) { return "eeg2video_hip 0.1 (gfx950, fp32 MFMA)"; }

e2v_status e2v_create(const e2v_config* cfg, int device, e2v_ctx** out) { return e2v_create_clip_vision(cfg, nullptr, device, out); }

int64_t e2v_clipv_config_size(void) { return (int64_t)sizeof(e2v_clipv_config); }

e2v_status e2v_create_clip_vision(const e2v_config* cfg, const e2v_clipv_config* clipv, int device, e2v_ctx** out) {
    return e2v_create_ex(cfg, clipv, nullptr, device, out);
}

int64_t e2v_s2s_config_size(void) { return (int64_t)sizeof(e2v_s2s_config); }

void e2v_default_s2s_config(e2v_s2s_config* s) {      // myTransformer() as the reference constructs it (my_autoregressive_transformer.py:125-149)
    std::memset(s, 0, sizeof(*s));
    s->s2s_electrodes = 62; s->s2s_samples = 100; s->s2s_windows = 7;
    s->s2s_f1 = 16; s->s2s_d = 4; s->s2s_f2 = 16;
    s->s2s_d_model = 512; s->s2s_heads = 4; s->s2s_ffn = 2048; s->s2s_encoder_layers = 2; s->s2s_decoder_layers = 4;
    s->s2s_steps = 6;
    s->s2s_latent_channels = 4; s->s2s_latent_h = 36; s->s2s_latent_w = 64;
    s->s2s_txt_classes = 13;
    s->s2s_norm_eps = 1e-5f; s->s2s_bn_eps = 1e-5f;
}

e2v_status e2v_create_ex(const e2v_config* cfg, const e2v_clipv_config* clipv, const e2v_s2s_config* s2s, int device, e2v_ctx** out) {
    return e2v_create_ex2(cfg, clipv, s2s, nullptr, device, out);
}

int64_t e2v_glm_config_size(void) { return (int64_t)sizeof(e2v_glm_config); }

void e2v_default_glm_config(e2v_glm_config* g) {      // glfnet(2, 64, 62, 200) and glfnet_mlp(40, 64, 310) as the reference's scripts construct them
    std::memset(g, 0, sizeof(*g));
    g->glm_electrodes = 62; g->glm_samples = 200; g->glm_occ_first = 50; g->glm_occ_count = 12;
    g->glm_filters = 40; g->glm_taps = 25; g->glm_pool = 51; g->glm_pool_stride = 5;
    g->glm_bands = 5; g->glm_hidden1 = 512; g->glm_hidden2 = 256; g->glm_emb = 64;
    g->glm_raw_out = 2; g->glm_mlp_out = 40;
    g->glm_bn_eps = 1e-5f;
}

e2v_status e2v_create_ex2(const e2v_config* cfg, const e2v_clipv_config* clipv, const e2v_s2s_config* s2s, const e2v_glm_config* glm, int device,
                          e2v_ctx** out) {
    if (glm) {                                                   // (all zero: no GLMNet)
        static const e2v_glm_config none = {};
        if (std::memcmp(glm, &none, sizeof(none)) == 0) glm = nullptr;
    }
    if (clipv && clipv->clipv_layers == 0) clipv = nullptr;      // (all zero: no tower)
    if (s2s) {                                                   // (all zero: no Seq2Seq model)
        static const e2v_s2s_config none = {};
        if (std::memcmp(s2s, &none, sizeof(none)) == 0) s2s = nullptr;
    }
    if (!cfg || !out) { g_create_error = "null argument"; return E2V_EINVAL; }
    *out = nullptr;
    e2v_ctx* c = nullptr;
    e2v_status st = guarded(nullptr, [&] {
        if (device != -1) {      // device = -1: host-only context (key scheme + DDIM schedule), no HIP call at all
            int ndev = 0;
            E2V_HIP(hipGetDeviceCount(&ndev));
            E2V_REQUIRE(device >= 0 && device < ndev, E2V_EINVAL, "no such HIP device");
            E2V_HIP(hipSetDevice(device));
        }
        E2V_REQUIRE(cfg->attention_heads > 0 && cfg->norm_num_groups > 0 && cfg->layers_per_block > 0, E2V_EINVAL, "bad config");
        for (int i = 0; i < 4; ++i) {
            const int heads = cfg->attention_heads_per_block[i] > 0 ? cfg->attention_heads_per_block[i] : cfg->attention_heads;
            E2V_REQUIRE(cfg->attention_heads_per_block[i] >= 0 && cfg->block_out_channels[i] % cfg->norm_num_groups == 0 &&
                            cfg->block_out_channels[i] % 32 == 0 && cfg->block_out_channels[i] % heads == 0 &&
                            (cfg->block_out_channels[i] / heads) % 8 == 0,
                        E2V_EINVAL, "block_out_channels must be multiples of 32, of norm_num_groups and of 8*heads");
            E2V_REQUIRE(flash_attention_supports(cfg->block_out_channels[i] / heads), E2V_EINVAL,
                        "block_out_channels / attention heads must be a head dim with a kernel instance (8, 16, 32, 40, 64, 80, 160)");
            E2V_REQUIRE(cfg->vae_block_out_channels[i] % cfg->vae_norm_num_groups == 0 && cfg->vae_block_out_channels[i] % 4 == 0,
                        E2V_EINVAL, "vae_block_out_channels must be multiples of 4 and of vae_norm_num_groups");
        }
        E2V_REQUIRE(cfg->cross_attention_dim % 4 == 0 && cfg->in_channels % 4 == 0, E2V_EINVAL,
                    "cross_attention_dim and in_channels must be multiples of 4");
        if (cfg->text_layers != 0) {                     // (all zero: no text encoder)
            E2V_REQUIRE(cfg->text_layers > 0 && cfg->text_vocab_size > 0 && cfg->text_heads > 0 && cfg->text_intermediate > 0 &&
                            cfg->text_intermediate % 4 == 0 && (cfg->text_act == 0 || cfg->text_act == 1) && cfg->text_norm_eps > 0.f,
                        E2V_EINVAL, "bad text encoder config (sizes must be positive, text_intermediate a multiple of 4, text_act 0 = quick_gelu or 1 = gelu)");
            E2V_REQUIRE(cfg->text_hidden == 64 * cfg->text_heads, E2V_EINVAL,
                        "text_hidden must be 64 * text_heads: 64 is the head dim of the text attention kernel's only instance");
            E2V_REQUIRE(cfg->text_hidden % 4 == 0 && cfg->text_hidden <= 1280, E2V_EINVAL, "text_hidden must be a multiple of 4, at most 1280 (the LayerNorm kernel's limit)");
            E2V_REQUIRE(cfg->text_max_positions >= 1 && cfg->text_max_positions <= kTextAttnMaxT, E2V_EINVAL,
                        "text_max_positions must be in 1 .. " + std::to_string(kTextAttnMaxT) + ": the text attention kernel keeps K and V of a prompt in LDS");
        }
        if (cfg->vit_layers != 0) {                      // (all zero: no image classifier)
            E2V_REQUIRE(cfg->vit_layers > 0 && cfg->vit_heads > 0 && cfg->vit_intermediate > 0 && cfg->vit_intermediate % 4 == 0 &&
                            cfg->vit_image_size > 0 && cfg->vit_patch_size > 0 && cfg->vit_num_labels >= 3 && cfg->vit_norm_eps > 0.f,
                        E2V_EINVAL, "bad image classifier config (sizes must be positive, vit_intermediate a multiple of 4, vit_num_labels at least 3)");
            E2V_REQUIRE(cfg->vit_hidden == 64 * cfg->vit_heads, E2V_EINVAL,
                        "vit_hidden must be 64 * vit_heads: 64 is the head dim of the image attention kernel's only instance");
            E2V_REQUIRE(cfg->vit_hidden % 4 == 0 && cfg->vit_hidden <= 1280, E2V_EINVAL, "vit_hidden must be a multiple of 4, at most 1280 (the LayerNorm kernel's limit)");
            E2V_REQUIRE(cfg->vit_image_size % cfg->vit_patch_size == 0 && (3 * cfg->vit_patch_size * cfg->vit_patch_size) % 4 == 0, E2V_EINVAL,
                        "vit_image_size must be a multiple of vit_patch_size, and 3 * vit_patch_size^2 a multiple of 4");
            const long long grid = cfg->vit_image_size / cfg->vit_patch_size;
            E2V_REQUIRE(grid * grid + 1 <= kImageAttnMaxT, E2V_EINVAL,
                        "(vit_image_size / vit_patch_size)^2 + 1 tokens must be at most " + std::to_string(kImageAttnMaxT) +
                            ": the image attention kernel keeps K and V of an image's head in LDS");
            for (int ch = 0; ch < 3; ++ch) E2V_REQUIRE(cfg->vit_std[ch] != 0.f, E2V_EINVAL, "vit_std must be non-zero");
        }
        if (cfg->vmae_layers != 0) {                     // (all zero: no video classifier)
            E2V_REQUIRE(cfg->vmae_layers > 0 && cfg->vmae_heads > 0 && cfg->vmae_intermediate > 0 && cfg->vmae_intermediate % 4 == 0 &&
                            cfg->vmae_image_size > 0 && cfg->vmae_patch_size > 0 && cfg->vmae_tubelet_size > 0 && cfg->vmae_num_frames > 0 &&
                            cfg->vmae_norm_eps > 0.f,
                        E2V_EINVAL, "bad video classifier config (sizes must be positive, vmae_intermediate a multiple of 4)");
            E2V_REQUIRE(cfg->vmae_num_labels >= 3, E2V_EINVAL, "vmae_num_labels must be at least 3 (the top-3 head)");
            E2V_REQUIRE(cfg->vmae_hidden == 64 * cfg->vmae_heads, E2V_EINVAL,
                        "vmae_hidden must be 64 * vmae_heads: 64 is the head dim of the token attention kernel's only instance");
            E2V_REQUIRE(cfg->vmae_hidden % 4 == 0 && cfg->vmae_hidden <= 1280, E2V_EINVAL, "vmae_hidden must be a multiple of 4, at most 1280 (the LayerNorm kernel's limit)");
            E2V_REQUIRE(cfg->vmae_num_frames % cfg->vmae_tubelet_size == 0, E2V_EINVAL, "vmae_num_frames must be a multiple of vmae_tubelet_size");
            E2V_REQUIRE(cfg->vmae_image_size % cfg->vmae_patch_size == 0 &&
                            (3 * cfg->vmae_tubelet_size * cfg->vmae_patch_size * cfg->vmae_patch_size) % 4 == 0, E2V_EINVAL,
                        "vmae_image_size must be a multiple of vmae_patch_size, and 3 * vmae_tubelet_size * vmae_patch_size^2 a multiple of 4");
            E2V_REQUIRE(cfg->vmae_resize_edge >= cfg->vmae_image_size && cfg->vmae_resize_edge <= 4096, E2V_EINVAL,
                        "vmae_resize_edge must be at least vmae_image_size (the centre crop is taken from the resized frame) and at most 4096");
            const long long tokens = (long long)(cfg->vmae_num_frames / cfg->vmae_tubelet_size) * (cfg->vmae_image_size / cfg->vmae_patch_size) *
                                     (cfg->vmae_image_size / cfg->vmae_patch_size);
            E2V_REQUIRE(tokens <= (1 << 20), E2V_EINVAL, "the video classifier's token count must be at most 2^20");
            for (int ch = 0; ch < 3; ++ch) E2V_REQUIRE(cfg->vmae_std[ch] != 0.f, E2V_EINVAL, "vmae_std must be non-zero");
        }
        if (clipv) check_clipv_config(clipv);
        if (s2s) check_s2s_config(s2s);
        if (glm) check_glm_config(glm);
        c = new e2v_ctx();
        c->cfg = *cfg;
        c->device = device;
        if (clipv) c->vcfg = *clipv;
        if (s2s) c->scfg = *s2s;
        if (glm) c->gcfg = *glm;
        for (int ch = 0; ch < 3 && c->vcfg.clipv_layers > 0; ++ch) // CLIPImageProcessor: as the image processor's table
            for (int b = 0; b < 256; ++b) {
                const float x = (float)((double)b * c->vcfg.clipv_rescale);
                c->clipv_lut[ch * 256 + b] = (x - c->vcfg.clipv_mean[ch]) / c->vcfg.clipv_std[ch];
            }
        for (int ch = 0; ch < 3 && cfg->vmae_layers > 0; ++ch)     // VideoMAEImageProcessor: as the image processor's table
            for (int b = 0; b < 256; ++b) {
                const float x = (float)((double)b * cfg->vmae_rescale);
                c->video_lut[ch * 256 + b] = (x - cfg->vmae_mean[ch]) / cfg->vmae_std[ch];
            }
        for (int ch = 0; ch < 3 && cfg->vit_layers > 0; ++ch)      // ViTImageProcessor: rescale in double, rounded to fp32; normalise in fp32
            for (int b = 0; b < 256; ++b) {
                const float x = (float)((double)b * cfg->vit_rescale);
                c->image_lut[ch * 256 + b] = (x - cfg->vit_mean[ch]) / cfg->vit_std[ch];
            }
        c->expected_keys();
        make_alphas(c);
        if (const char* e = std::getenv("E2V_CONV_ALGO")) c->conv_algo = std::atoi(e);
        if (const char* e = std::getenv("E2V_F32X3")) c->x3_compute = std::atoi(e) != 0;
        if (const char* e = std::getenv("E2V_WINO_MIN_C")) c->wino_min_c = std::atoi(e);
        if (const char* e = std::getenv("E2V_WINO_F4")) c->wino_f4 = std::atoi(e) != 0;
        if (const char* e = std::getenv("E2V_WINO_F4_PAD")) c->wino_f4_pad = std::atof(e);
        if (const char* e = std::getenv("E2V_WINO_F4_MIN_C")) c->wino4_min_c = std::atoi(e);
        if (const char* e = std::getenv("E2V_WINO_WS_MB")) c->wino_ws_floats = (size_t)std::atol(e) * (1u << 18);
    });
    if (st != E2V_OK) { delete c; return st; }
    *out = c;
    return E2V_OK;
}

void e2v_destroy(e2v_ctx* c) {
    if (!c) return;
    if (c->device < 0) { delete c; return; }                 // (host-only, dry runs included: nothing is owned, no HIP call)
    c->pool.closing();                                       // (E2V_POOL_GUARD: the step caches released by `delete` are not compared any more)
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    (void)e2v_comm_destroy(c);
    if (c->stream_ev) (void)hipEventDestroy(c->stream_ev);
    delete c;                                                // every device block frees itself (the step caches before the pool: member order)
}

const char* e2v_last_error(const e2v_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int64_t e2v_num_expected_keys(const e2v_ctx* c) { return c ? (int64_t)c->keys.size() : 0; }

const char* e2v_expected_key(const e2v_ctx* c, int64_t i, int64_t* shape4, int* ndim) {
    if (!c || i < 0 || i >= (int64_t)c->keys.size()) return nullptr;
    const std::string& k = c->keys[(size_t)i];
    const WTensor& t = c->raw.at(k);
    if (ndim) *ndim = (int)t.shape.size();
    if (shape4) for (size_t d = 0; d < 4; ++d) shape4[d] = d < t.shape.size() ? t.shape[d] : 1;
    return k.c_str();
}

e2v_status e2v_load_tensor(e2v_ctx* c, const char* key, const void* host, e2v_dtype dtype, const int64_t* shape, int ndim) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(key && host && shape, E2V_EINVAL, "null argument");
        auto it = c->raw.find(key);
        E2V_REQUIRE(it != c->raw.end(), E2V_ENOWEIGHT, std::string("unexpected state-dict key: ") + key);
        WTensor& t = it->second;
        bool same = (int)t.shape.size() == ndim;
        for (int d = 0; same && d < ndim; ++d) same = t.shape[d] == shape[d];
        E2V_REQUIRE(same, E2V_ENOWEIGHT, std::string("shape mismatch for ") + key);
        if (!t.mem) t.mem = dev_block(t.numel * sizeof(float), 0, nullptr, false);
        if (dtype == E2V_F32) {
            E2V_HIP(hipMemcpy(t.d(), host, t.numel * sizeof(float), hipMemcpyHostToDevice));
        } else if (dtype == E2V_F16) {
            std::vector<float> tmp(t.numel);
            const uint16_t* h = static_cast<const uint16_t*>(host);
            for (size_t i = 0; i < t.numel; ++i) tmp[i] = half_to_float(h[i]);
            E2V_HIP(hipMemcpy(t.d(), tmp.data(), t.numel * sizeof(float), hipMemcpyHostToDevice));
        } else if (dtype == E2V_BF16) {                           // bf16 is the high half of the fp32 pattern
            std::vector<uint32_t> tmp(t.numel);
            const uint16_t* h = static_cast<const uint16_t*>(host);
            for (size_t i = 0; i < t.numel; ++i) tmp[i] = (uint32_t)h[i] << 16;
            E2V_HIP(hipMemcpy(t.d(), tmp.data(), t.numel * sizeof(float), hipMemcpyHostToDevice));
        } else {
            throw Error(E2V_EINVAL, "unsupported dtype");
        }
        t.loaded = true;
    });
}

}  // extern "C"

namespace {
// the tensor behind `key`, once the part that owns it is finalized
const WTensor& updatable(e2v_ctx* c, const char* key) {
    auto it = c->raw.find(key);
    E2V_REQUIRE(it != c->raw.end(), E2V_ENOWEIGHT, std::string("unexpected state-dict key: ") + key);
    const std::string k(key);
    E2V_REQUIRE(c->ready[e2v_ctx::key_part(k)], E2V_ESTATE, "the part that owns " + k + " is not finalized: upload it with e2v_load_tensor, then e2v_finalize_weights");
    return it->second;
}
}  // namespace

extern "C" {

e2v_status e2v_update_tensor(e2v_ctx* c, const char* key, const void* data, e2v_dtype dtype, int on_device, const int64_t* shape,
                             int ndim, e2v_stream stream) {
    return entry(c, [&] {
        E2V_REQUIRE(key && data && shape, E2V_EINVAL, "null argument");
        E2V_REQUIRE(dtype == E2V_F32 || dtype == E2V_F16 || dtype == E2V_BF16, E2V_EINVAL, "e2v_update_tensor: the source is fp32, fp16 or bf16");
        const char* frozen = e2v_ctx::kParts[e2v_ctx::key_part(key)].frozen;
        E2V_REQUIRE(!frozen, E2V_EINVAL, std::string("e2v_update_tensor: ") + frozen);
    }, [&] {
        E2V_REQUIRE(!dry_run(), E2V_ESTATE, "no weights in a dry run");
        const WTensor& t = updatable(c, key);
        bool same = (int)t.shape.size() == ndim;
        for (int d = 0; same && d < ndim; ++d) same = t.shape[d] == shape[d];
        E2V_REQUIRE(same, E2V_ENOWEIGHT, std::string("shape mismatch for ") + key);
        c->update_tensor(key, data, dtype, on_device != 0, S(c, stream));
    });
}

e2v_status e2v_read_tensor(e2v_ctx* c, const char* key, int form, void* out, e2v_dtype dtype, int on_device, const int64_t* shape,
                           int ndim, e2v_stream stream) {
    return entry(c, [&] {
        E2V_REQUIRE(key && out && shape, E2V_EINVAL, "null argument");
        auto it = c->raw.find(key);
        E2V_REQUIRE(it != c->raw.end(), E2V_ENOWEIGHT, std::string("unexpected state-dict key: ") + key);
        const WTensor& t = it->second;
        bool same = (int)t.shape.size() == ndim;
        for (int d = 0; same && d < ndim; ++d) same = t.shape[d] == shape[d];
        E2V_REQUIRE(same, E2V_ENOWEIGHT, std::string("shape mismatch for ") + key);
        E2V_REQUIRE(dtype == E2V_F32 || dtype == E2V_F16 || dtype == E2V_BF16, E2V_EINVAL, "e2v_read_tensor: the destination is fp32, fp16 or bf16");
        if (form == 0) form = E2V_FORM_F32;
        E2V_REQUIRE((form & (form - 1)) == 0, E2V_EINVAL, "e2v_read_tensor: `form` names one stored form (one E2V_FORM_* bit)");
        E2V_REQUIRE(form > 0 && form <= E2V_FORM_WINO4_X3, E2V_EINVAL, "e2v_read_tensor: unknown form bit");
        E2V_REQUIRE(form == E2V_FORM_F32 || form == E2V_FORM_BF16 || form == E2V_FORM_F16 || form == E2V_FORM_X3, E2V_EINVAL,
                    "e2v_read_tensor: the conv kernel layouts, the Winograd domains and the UP2 forms have no index-map inverse; read E2V_FORM_F32");
        updatable(c, key);
        c->read_source(key, form);
    }, [&] {
        E2V_REQUIRE(!dry_run(), E2V_ESTATE, "no weights in a dry run");
        c->read_tensor(key, form, out, dtype, on_device != 0, S(c, stream));
    });
}

e2v_status e2v_op_weight_forms(e2v_ctx* c, const char* key, int* mask) {
    return entry(c, [&] { E2V_REQUIRE(key && mask, E2V_EINVAL, "null argument"); }, [&] {
        updatable(c, key);
        *mask = c->weight_forms(key);
    });
}

e2v_status e2v_finalize_weights(e2v_ctx* c, int which) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        // (bits 7 and 8 belong to the mask of a context that was made with a Seq2Seq / a GLMNet config; on any other they are out of range,
        // as they always were)
        const int mask = 127 | (c->has_part(e2v_ctx::S2S) ? 128 : 0) | (c->has_part(e2v_ctx::GLM) ? 256 : 0);
        E2V_REQUIRE(which >= 1 && (which & ~mask) == 0, E2V_EINVAL,
                    "which is a bit mask: 1 UNet, 2 VAE, 4 semantic predictor, 8 text encoder, 16 image classifier, 32 video classifier, 64 CLIP vision tower, "
                    "128 Seq2Seq latent model (a context made by e2v_create_ex with an e2v_s2s_config only), 256 GLMNet (a context made by "
                    "e2v_create_ex2 with an e2v_glm_config only)");
        c->finalize(which);
    });
}

e2v_status e2v_ddim_timesteps(const e2v_ctx* c, int n, int64_t* out) {
    if (!c || !out || n <= 0 || n > c->cfg.num_train_timesteps) return E2V_EINVAL;
    const int64_t ratio = c->cfg.num_train_timesteps / n;            // step_ratio = T // n
    for (int i = 0; i < n; ++i) out[i] = (int64_t)(n - 1 - i) * ratio + c->cfg.steps_offset;
    return E2V_OK;
}

e2v_status e2v_ddim_alphas_cumprod(const e2v_ctx* c, float* out) {
    if (!c || !out) return E2V_EINVAL;
    std::memcpy(out, c->alphas.data(), c->alphas.size() * sizeof(float));
    return E2V_OK;
}

e2v_status e2v_set_alphas_cumprod(e2v_ctx* c, const float* t, int n) {
    if (!c || !t || n != c->cfg.num_train_timesteps) return E2V_EINVAL;
    c->alphas.assign(t, t + n);
    return E2V_OK;
}

e2v_status e2v_set_ddim_schedule(e2v_ctx* c, const float* t, int n, int steps_offset) {
    if (!c || !t || n <= 0 || steps_offset < 0 || steps_offset >= n) return E2V_EINVAL;
    c->cfg.num_train_timesteps = n;
    c->cfg.steps_offset = steps_offset;
    c->alphas.assign(t, t + n);
    return E2V_OK;
}

// ---- SURVEY 8(f) rows ---------------------------------------------------------------------------------------
e2v_status e2v_semantic_predict(e2v_ctx* c, const float* eeg, int B, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        c->require_ready(e2v_ctx::SEM);
        E2V_REQUIRE(eeg && out && B > 0, E2V_EINVAL, "bad arguments");
        hipStream_t s = S(c, stream);
        const bool b16 = c->bf16_compute;                        // bf16-activation mode: bf16 rows between the layers, fp32 result
        static const bool gemv_on = [] { const char* e = std::getenv("E2V_SEM_GEMV"); return !e || std::atoi(e) != 0; }();
        if (gemv_on && gemv_rows_supported(B, c->cfg.sem_hidden, b16) && gemv_rows_supported(B, c->sem_in_pad, b16)) {
            // the reference's batch sizes (1 .. a few EEG segments): every layer is a stream over its weight matrix
            Act x(c->pool, B, c->sem_in_pad);
            pad_cols(eeg, c->cfg.sem_in_features, x.p, c->sem_in_pad, B, s);
            for (size_t i = 0; i < c->sem.size(); ++i) {
                const LinW& w = c->sem[i];
                const bool last = i + 1 == c->sem.size();
                Act y;
                if (!last) y = Act(c->pool, B, w.out);
                const void* w16 = c->h16_mode == H16_FP16 ? c->lin_f16(w, s) : w.w16;
                gemv_rows(x.p, x.C, b16 ? w16 : (const void*)w.w, b16 ? w.in16 : w.in, b16 ? c->h16_mode : 0, w.b, last ? out : y.p, w.out, B, w.out,
                          b16 ? w.in16 : w.in, last ? 0 : 1, s);
                if (!last) x = std::move(y);
            }
            E2V_HIP(hipGetLastError());
            return;
        }
        Act x(c->pool, B, c->sem_in_pad, b16);
        pad_cols(eeg, c->cfg.sem_in_features, x.p, c->sem_in_pad, B, s, b16 ? c->h16_mode : 0);
        for (size_t i = 0; i < c->sem.size(); ++i) {              // Linear -> ReLU ... -> Linear (train_semantic_predictor.py:14-28)
            const LinW& w = c->sem[i];
            const bool last = i + 1 == c->sem.size();
            Act y;
            if (!last) y = Act(c->pool, B, w.out, b16);
            IgemmArgs g;
            g.a0 = x.p; g.c0 = b16 ? w.in16 : w.in; g.lda0 = g.c0; g.w = w.w; g.ldw = w.in; g.bias = w.b;
            g.out = last ? out : y.p; g.ldc = w.out; g.M = B; g.N = w.out; g.taps = 1; g.relu = last ? 0 : 1; g.ldw16 = w.in16;
            if (b16) { g.w16 = c->h16_mode == H16_FP16 ? c->lin_f16(w, s) : w.w16; g.a_bf16 = c->h16_mode; g.out_f32 = last ? 1 : 0; }
            igemm(g, s);
            if (!last) x = std::move(y);
        }
        E2V_HIP(hipGetLastError());
    });
}

// CLIPTextModel.forward(input_ids)[0]: the ids are checked and narrowed on the host, everything else is enqueued on the stream
e2v_status e2v_text_encode(e2v_ctx* c, const int64_t* host_ids, int B, int T, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        c->require_part(e2v_ctx::TEXT);
        c->require_ready(e2v_ctx::TEXT);
        E2V_REQUIRE(host_ids && out && (reinterpret_cast<uintptr_t>(out) & 15) == 0, E2V_EINVAL, "null or misaligned argument (out: 16 bytes)");
        E2V_REQUIRE(B > 0 && T >= 1 && T <= c->cfg.text_max_positions, E2V_ESHAPE,
                    "input_ids must be [B >= 1][1 <= T <= text_max_positions = " + std::to_string(c->cfg.text_max_positions) + "]");
        const size_t n = (size_t)B * T;
        std::vector<int> ids(n);
        for (size_t i = 0; i < n; ++i) {
            E2V_REQUIRE(host_ids[i] >= 0 && host_ids[i] < c->cfg.text_vocab_size, E2V_EINVAL,
                        "input id " + std::to_string((long long)host_ids[i]) + " is outside [0, text_vocab_size = " + std::to_string(c->cfg.text_vocab_size) + ")");
            ids[i] = (int)host_ids[i];
        }
        hipStream_t s = S(c, stream);
        Act d(c->pool, (int64_t)n, 1);
        E2V_HIP(hipMemcpyAsync(d.p, ids.data(), n * sizeof(int), hipMemcpyHostToDevice, s));
        c->text_encode(reinterpret_cast<const int*>(d.p), B, T, out, s);
    });
}

// myTransformer.forward + the [:, :-1] of its inference.  What is wrong with the call itself is answered first and without a HIP call
// (E2V_EINVAL, a host-only context included); then the state of the context (E2V_ESTATE); nothing is enqueued before both passed.
e2v_status e2v_seq2seq_latents(e2v_ctx* c, const float* eeg, int64_t clip_stride, int64_t window_stride, int64_t channel_stride,
                               const float* mean, const float* scale, int B, int first, int count, int layout, float* latents,
                               float* txt_logits, float* tokens, e2v_stream stream) {
    return entry(c, [&] {
        auto off = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
        E2V_REQUIRE(eeg, E2V_EINVAL, "e2v_seq2seq_latents: eeg is NULL");
        E2V_REQUIRE(latents || txt_logits || tokens, E2V_EINVAL, "e2v_seq2seq_latents: no output asked for (latents, txt_logits and tokens are all NULL)");
        E2V_REQUIRE((mean == nullptr) == (scale == nullptr), E2V_EINVAL, "e2v_seq2seq_latents: the input scaler is a mean AND a scale, or neither");
        E2V_REQUIRE(!off(eeg, 3) && !off(mean, 3) && !off(scale, 3) && !off(txt_logits, 3), E2V_EINVAL,
                    "e2v_seq2seq_latents: eeg, mean, scale and txt_logits must be 4-byte aligned");
        E2V_REQUIRE(!off(latents, 15) && !off(tokens, 15), E2V_EINVAL, "e2v_seq2seq_latents: latents and tokens must be 16-byte aligned");
        E2V_REQUIRE(clip_stride >= 0 && window_stride >= 0 && channel_stride >= 0, E2V_EINVAL, "e2v_seq2seq_latents: strides are non-negative element counts");
        if (latents || tokens) {
            E2V_REQUIRE(layout == 0 || layout == 1, E2V_EINVAL, "e2v_seq2seq_latents: layout is 0 ([B][count][C][h][w]) or 1 ([B][C][count][h][w])");
            const int T1 = c->scfg.s2s_d_model > 0 ? c->scfg.s2s_steps + 1 : 0x7FFFFFF;      // (without a config the range has no upper end to miss)
            E2V_REQUIRE(first >= 0 && count >= 1 && (long long)first + count <= T1, E2V_EINVAL,
                        "e2v_seq2seq_latents: tokens [first, first + count) must lie in [0, s2s_steps + 1) with count >= 1");
        }
        E2V_REQUIRE(B >= 1, E2V_EINVAL, "e2v_seq2seq_latents: B must be at least 1");
        c->require_part(e2v_ctx::S2S);
        c->require_ready(e2v_ctx::S2S);
        E2V_REQUIRE((long long)B * std::max(c->scfg.s2s_windows, c->scfg.s2s_steps + 1) * std::max(c->scfg.s2s_ffn, 3 * c->scfg.s2s_d_model) <= 0x7FFFFFFFLL &&
                        (long long)B * (c->scfg.s2s_steps + 1) <= (1 << 20), E2V_ESHAPE, "e2v_seq2seq_latents: B is too large for one call");
    }, [&] {
        EegnetArgs e;
        e.eeg = eeg; e.clip_stride = clip_stride; e.window_stride = window_stride; e.channel_stride = channel_stride; e.mean = mean; e.scale = scale;
        c->seq2seq_latents(e, B, first, count, layout, latents, txt_logits, tokens, S(c, stream));
    });
}

// DE_PSD of every (clip, window, electrode) row.  No weights: any context with a device serves it.  What is wrong with the call itself
// is answered first and without a HIP call (E2V_EINVAL, a host-only context included); nothing is enqueued before that passed.
e2v_status e2v_eeg_de_psd(e2v_ctx* c, const float* eeg, int64_t clip_stride, int64_t window_stride, int64_t channel_stride, int B,
                          int windows, int electrodes, int samples, int fs, const float* de_mean, const float* de_scale, float* de,
                          float* psd, e2v_stream stream) {
    DePsdArgs a;
    return entry(c, [&] {
        auto off = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
        E2V_REQUIRE(eeg, E2V_EINVAL, "e2v_eeg_de_psd: eeg is NULL");
        E2V_REQUIRE(de || psd, E2V_EINVAL, "e2v_eeg_de_psd: no output asked for (de and psd are both NULL)");
        E2V_REQUIRE((de_mean == nullptr) == (de_scale == nullptr), E2V_EINVAL, "e2v_eeg_de_psd: the DE scaler is a mean AND a scale, or neither");
        E2V_REQUIRE(!off(eeg) && !off(de_mean) && !off(de_scale) && !off(de) && !off(psd), E2V_EINVAL,
                    "e2v_eeg_de_psd: eeg, de_mean, de_scale, de and psd must be 4-byte aligned");
        E2V_REQUIRE(clip_stride >= 0 && window_stride >= 0 && channel_stride >= 0, E2V_EINVAL, "e2v_eeg_de_psd: strides are non-negative element counts");
        E2V_REQUIRE(B >= 1, E2V_EINVAL, "e2v_eeg_de_psd: B must be at least 1");
        E2V_REQUIRE(windows >= 1 && electrodes >= 1 && samples >= 1 && samples <= 65536, E2V_EINVAL,
                    "e2v_eeg_de_psd: windows, electrodes and samples must be at least 1, samples at most 65536");
        E2V_REQUIRE(de_psd_bands(fs, a.first, a.last), E2V_EINVAL,
                    "e2v_eeg_de_psd: at sampling rate " + std::to_string(fs) + " a band's first bin int(fStart / fs * 200) is below 1 or its last "
                    "int(fEnd / fs * 200) above 100: the reference would index from the end of the spectrum or past its half (fs = 200 is its rate)");
        E2V_REQUIRE((long long)B * windows * electrodes <= 0x7FFFFFFFLL, E2V_ESHAPE, "e2v_eeg_de_psd: B * windows * electrodes must stay below 2^31");
    }, [&] {
        hipStream_t s = S(c, stream);
        const std::vector<float>& plan = c->de_psd_plan(samples);      // (lives in the context)
        Act dp(c->pool, (int64_t)plan.size(), 1);
        E2V_HIP(hipMemcpyAsync(dp.p, plan.data(), plan.size() * sizeof(float), hipMemcpyHostToDevice, s));
        a.eeg = eeg; a.clip_stride = clip_stride; a.window_stride = window_stride; a.channel_stride = channel_stride;
        a.plan = dp.p; a.de_mean = de_mean; a.de_scale = de_scale; a.de = de; a.psd = psd;
        a.B = B; a.W = windows; a.C = electrodes; a.n = std::min(samples, kDePsdN);
        a.bins = *std::max_element(a.last, a.last + kDePsdBands) + 1;
        eeg_de_psd(a, s);
        E2V_HIP(hipGetLastError());
    });
}

// glfnet.forward + what its callers take from it.  Argument checks first and without a HIP call, then the state of the context.
e2v_status e2v_glmnet_raw(e2v_ctx* c, const float* eeg, int64_t clip_stride, int64_t channel_stride, int B, const float* in_mean,
                          const float* in_scale, float* logits, float* features, int32_t* labels, e2v_stream stream) {
    return entry(c, [&] {
        auto off = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
        E2V_REQUIRE(eeg, E2V_EINVAL, "e2v_glmnet_raw: eeg is NULL");
        E2V_REQUIRE(logits || features || labels, E2V_EINVAL, "e2v_glmnet_raw: no output asked for (logits, features and labels are all NULL)");
        E2V_REQUIRE((in_mean == nullptr) == (in_scale == nullptr), E2V_EINVAL, "e2v_glmnet_raw: the input scaler is a mean AND a scale, or neither");
        E2V_REQUIRE(!off(eeg) && !off(in_mean) && !off(in_scale) && !off(logits) && !off(features) && !off(labels), E2V_EINVAL,
                    "e2v_glmnet_raw: every pointer must be 4-byte aligned");
        E2V_REQUIRE(clip_stride >= 0 && channel_stride >= 0, E2V_EINVAL, "e2v_glmnet_raw: strides are non-negative element counts");
        E2V_REQUIRE(B >= 1, E2V_EINVAL, "e2v_glmnet_raw: B must be at least 1");
        c->require_part(e2v_ctx::GLM);
        E2V_REQUIRE(c->gcfg.glm_raw_out > 0, E2V_ESTATE, "the context's GLMNet config has no raw model (glm_raw_out = 0)");
        c->require_ready(e2v_ctx::GLM);
        E2V_REQUIRE((long long)B * std::max(c->glm_raw_features(), c->gcfg.glm_filters) <= 0x7FFFFFFFLL, E2V_ESHAPE, "e2v_glmnet_raw: B is too large for one call");
    }, [&] {
        ShallowArgs a;
        a.eeg = eeg; a.clip_stride = clip_stride; a.channel_stride = channel_stride; a.mean = in_mean; a.scale = in_scale;
        c->glmnet_raw(a, B, logits, features, labels, S(c, stream));
    });
}

// glfnet_mlp.forward over DE features on the device
e2v_status e2v_glmnet_mlp(e2v_ctx* c, const float* de, int B, float* logits, float* features, int32_t* labels, e2v_stream stream) {
    return entry(c, [&] {
        auto off = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) != 0; };
        E2V_REQUIRE(de, E2V_EINVAL, "e2v_glmnet_mlp: de is NULL");
        E2V_REQUIRE(logits || features || labels, E2V_EINVAL, "e2v_glmnet_mlp: no output asked for (logits, features and labels are all NULL)");
        E2V_REQUIRE(!off(de) && !off(logits) && !off(features) && !off(labels), E2V_EINVAL, "e2v_glmnet_mlp: every pointer must be 4-byte aligned");
        E2V_REQUIRE(B >= 1, E2V_EINVAL, "e2v_glmnet_mlp: B must be at least 1");
        c->require_part(e2v_ctx::GLM);
        E2V_REQUIRE(c->gcfg.glm_mlp_out > 0, E2V_ESTATE, "the context's GLMNet config has no feature model (glm_mlp_out = 0)");
        c->require_ready(e2v_ctx::GLM);
        E2V_REQUIRE((long long)B * std::max(c->gcfg.glm_hidden1, c->gcfg.glm_electrodes * c->gcfg.glm_bands + 4) <= 0x7FFFFFFFLL, E2V_ESHAPE,
                    "e2v_glmnet_mlp: B is too large for one call");
    }, [&] { c->glmnet_mlp(de, B, logits, features, labels, S(c, stream)); });
}

e2v_status e2v_dana_noise(e2v_ctx* c, const float* x0, const float* ed, const float* es, const int64_t* host_t, int steps,
                          float dyn_beta, int B, int F, int C, int H, int W, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(x0 && ed && es && host_t && out, E2V_EINVAL, "null argument");
        E2V_REQUIRE(B > 0 && F > 0 && C > 0 && H > 0 && W > 0 && steps > 1, E2V_ESHAPE, "non-positive dimension");
        E2V_REQUIRE(dyn_beta >= 0.f && dyn_beta <= 1.f, E2V_EINVAL, "dynamic_beta must be in [0, 1]");
        // linear betas 1e-4 .. 0.02 (DANA_module.py:42-52), alphas_cumprod in fp32 as torch.cumprod does
        std::vector<float> ac(steps);
        {
            const float b0 = 0.0001f, b1 = 0.02f, step = (b1 - b0) / (float)(steps - 1);
            float prod = 1.f;
            for (int i = 0; i < steps; ++i) {
                const float beta = (i < steps / 2) ? b0 + step * (float)i : b1 - step * (float)(steps - 1 - i);
                prod *= 1.f - beta;
                ac[i] = prod;
            }
        }
        std::vector<float> coef(2 * (size_t)B);
        for (int b = 0; b < B; ++b) {
            E2V_REQUIRE(host_t[b] >= 0 && host_t[b] < steps, E2V_EINVAL, "timestep out of range");
            coef[2 * b] = std::sqrt(ac[(size_t)host_t[b]]);
            coef[2 * b + 1] = std::sqrt(1.f - ac[(size_t)host_t[b]]);
        }
        hipStream_t s = S(c, stream);
        Act dc(c->pool, B, 2);
        E2V_HIP(hipMemcpyAsync(dc.p, coef.data(), coef.size() * sizeof(float), hipMemcpyHostToDevice, s));
        dana_noise(x0, ed, es, dc.p, std::sqrt(1.f - dyn_beta), std::sqrt(dyn_beta), out, B, F, C, H * W, s);
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_frames_to_uint8(e2v_ctx* c, const float* videos, uint8_t* out, int64_t count, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(videos && out && count >= 0, E2V_EINVAL, "bad arguments");
        frames_to_u8(videos, out, count, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_frame_metrics(e2v_ctx* c, const void* a, int a_kind, const void* b, int b_kind, int n, int F, int C, int H, int W,
                             float* ssim, float* mse, e2v_stream stream) {
    return entry(c, [&] {
        const int known = E2V_FRAMES_U8 | E2V_FRAMES_CHANNELS_LAST;
        E2V_REQUIRE(a && b, E2V_EINVAL, "e2v_frame_metrics: null argument");
        E2V_REQUIRE(ssim || mse, E2V_EINVAL, "e2v_frame_metrics: ssim and mse are both NULL");
        E2V_REQUIRE((a_kind & ~known) == 0 && (b_kind & ~known) == 0, E2V_EINVAL, "e2v_frame_metrics: unknown bits in a kind");
        E2V_REQUIRE(n > 0 && F > 0, E2V_ESHAPE, "e2v_frame_metrics: non-positive clip or frame count");
        E2V_REQUIRE(C >= 1 && C <= 4, E2V_ESHAPE, "e2v_frame_metrics: 1 to 4 channels");
        E2V_REQUIRE(H >= 7 && W >= 7, E2V_ESHAPE, "e2v_frame_metrics: the 7x7 window exceeds the image");
        E2V_REQUIRE((double)n * F * (double)frame_metrics_tiles(H, W) < 2147483648.0, E2V_ESHAPE, "e2v_frame_metrics: too many tiles for one call");
    }, [&] {
        hipStream_t s = S(c, stream);
        Act partials(c->pool, (int64_t)(frame_metrics_partials_bytes(n, F, H, W) / 4), 1);
        const FrameSrc sa = frame_src(a, a_kind);
        const FrameSrc sb = frame_src(b, b_kind);
        frame_metrics(sa, sb, n, F, C, H, W, partials.p, ssim, mse, s);
        E2V_HIP(hipGetLastError());
    });
}

}  // extern "C"

namespace {
// the argument checks e2v_image_classify and e2v_op_image_preprocess share (no HIP call)
void check_frames(const char* who, const void* frames, int kind, int n, int F, int H, int W) {
    const int known = E2V_FRAMES_U8 | E2V_FRAMES_CHANNELS_LAST;
    const std::string w(who);
    E2V_REQUIRE(frames, E2V_EINVAL, w + ": null frames");
    E2V_REQUIRE((kind & ~known) == 0, E2V_EINVAL, w + ": unknown bits in kind");
    E2V_REQUIRE((kind & E2V_FRAMES_U8) || (reinterpret_cast<uintptr_t>(frames) & 3) == 0, E2V_EINVAL, w + ": fp32 frames must be 4-byte aligned");
    E2V_REQUIRE(n >= 1, E2V_EINVAL, w + ": n < 1");
    E2V_REQUIRE(F >= 1 && H >= 1 && W >= 1, E2V_ESHAPE, w + ": F, H and W must be at least 1");
    E2V_REQUIRE((double)n * F < 2147483648.0, E2V_ESHAPE, w + ": too many images for one call");
}

// What the preprocess ops do once their arguments are checked and their plan is made: the plan's tables onto the device, then launches of
// `step` frames (whole tubelets of ts) under the profile class `name`.  mode != 0 (H16_BF16 / H16_FP16): into 16-bit patch rows of that
// type, widened exactly into `rows`.
void run_preprocess(e2v_ctx* c, const char* name, const PrepPlan& plan, const void* frames, int kind, int n, int F, int ts, long long step,
                    int patch, int mode, float* rows, hipStream_t s) {
    Act tables = upload_plan(c->pool, plan, s);
    E2V_HIP(hipStreamSynchronize(s));                        // (`plan` is the caller's local: a test aid may wait)
    const int* tab = reinterpret_cast<const int*>(tables.p);
    const FrameSrc src = frame_src(frames, kind);
    const int K = 3 * ts * patch * patch;
    const long long per_img = (long long)(plan.S / patch) * (plan.S / patch) * 3 * patch * patch;      // row elements one frame contributes
    const long long total = (long long)n * F;
    for (long long i0 = 0; i0 < total; i0 += step) {
        const int ni = (int)std::min<long long>(step, total - i0);
        if (!mode) { frame_preprocess(src, n, F, ts, i0, ni, plan, tab, patch, rows + i0 * per_img, name, s); continue; }
        const long long nrows = (long long)ni * per_img / K;
        Act r16(c->pool, nrows, K, true);
        frame_preprocess(src, n, F, ts, i0, ni, plan, tab, patch, r16.p, name, s, mode);
        cvt_rows(r16.p, K, mode, rows + i0 * per_img, K, 0, nrows, K, K, s);
    }
    E2V_HIP(hipGetLastError());
}
}  // namespace

extern "C" {

// ViTImageProcessor + ViTForImageClassification + softmax + top 3 of every frame (img_classify_metric's classifier half)
e2v_status e2v_image_classify(e2v_ctx* c, const void* frames, int kind, int n, int F, int H, int W, float* logits, float* probs,
                              int32_t* top3, e2v_stream stream) {
    return entry(c, [&] {
        check_frames("e2v_image_classify", frames, kind, n, F, H, W);
        E2V_REQUIRE(logits || probs || top3, E2V_EINVAL, "e2v_image_classify: logits, probs and top3 are all NULL");
        E2V_REQUIRE(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(top3)) & 3) == 0,
                    E2V_EINVAL, "e2v_image_classify: misaligned output (4 bytes)");
        c->require_part(e2v_ctx::IMAGE);
        E2V_REQUIRE(c->prep_plan(e2v_ctx::IMAGE, H, W).band >= 1, E2V_ESHAPE,
                    "e2v_image_classify: the source rows of one output row do not fit the preprocess kernel's LDS band (downscale too strong)");
        c->require_ready(e2v_ctx::IMAGE);
    }, [&] {
        const FrameSrc src = frame_src(frames, kind);
        c->image_classify(src, n, F, H, W, logits, probs, top3, S(c, stream));
    });
}

e2v_status e2v_image_resize_table(int in_size, int out_size, int* first, int* count, int32_t* coeff, int* ksize) {
    if (!ksize || in_size < 1 || out_size < 1) return E2V_EINVAL;
    const ResizeAxis t = resize_axis(in_size, out_size);
    *ksize = t.ksize;
    if (first) std::memcpy(first, t.first.data(), t.first.size() * sizeof(int));
    if (count) std::memcpy(count, t.count.data(), t.count.size() * sizeof(int));
    if (coeff) std::memcpy(coeff, t.coeff.data(), t.coeff.size() * sizeof(int32_t));
    return E2V_OK;
}

e2v_status e2v_image_resize_table_filter(int in_size, int out_size, int filter, int* first, int* count, int32_t* coeff, int* ksize) {
    if (!ksize || in_size < 1 || out_size < 1 || (filter != kResizeBilinear && filter != kResizeBicubic)) return E2V_EINVAL;
    try {
        const ResizeAxis t = resize_axis(in_size, out_size, filter);
        *ksize = t.ksize;
        if (first) std::memcpy(first, t.first.data(), t.first.size() * sizeof(int));
        if (count) std::memcpy(count, t.count.data(), t.count.size() * sizeof(int));
        if (coeff) std::memcpy(coeff, t.coeff.data(), t.coeff.size() * sizeof(int32_t));
    } catch (const Error& e) {
        return e.code;
    }
    return E2V_OK;
}

// the preprocess of e2v_image_classify on its own, at any (S, P) and with the caller's pixel table
e2v_status e2v_op_image_preprocess(e2v_ctx* c, const void* frames, int kind, int n, int F, int H, int W, int size, int patch,
                                   const float* host_lut, float* rows, e2v_stream stream) {
    PrepPlan plan;
    return entry(c, [&] {
        check_frames("e2v_op_image_preprocess", frames, kind, n, F, H, W);
        E2V_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 3) == 0, E2V_EINVAL, "e2v_op_image_preprocess: null or misaligned rows");
        E2V_REQUIRE(size >= 1 && size <= 4096 && patch >= 1 && size % patch == 0, E2V_ESHAPE, "e2v_op_image_preprocess: 1 <= S <= 4096, a multiple of P >= 1");
        E2V_REQUIRE(host_lut || c->cfg.vit_layers > 0, E2V_ESTATE, "e2v_op_image_preprocess: no pixel table given and the config has no image classifier");
        plan = prep_plan(H, W, PrepWindow{size, size, 0, 0}, size, patch, host_lut ? host_lut : c->image_lut, kResizeBilinear);
        E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, "e2v_op_image_preprocess: the source rows of one output row do not fit the kernel's LDS band");
    }, [&] {
        run_preprocess(c, "image_preprocess", plan, frames, kind, n, F, 1, 4096, patch, 0, rows, S(c, stream));
    });
}

// fp32 in every compute mode, as e2v_image_classify runs it
e2v_status e2v_op_image_attention(e2v_ctx* c, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, e2v_stream stream) {
    return entry(c, [&] {
        E2V_REQUIRE(qkv && out, E2V_EINVAL, "null argument");
        E2V_REQUIRE(B > 0 && heads > 0 && T >= 1 && T <= kImageAttnMaxT, E2V_ESHAPE, "image attention: B, heads >= 1 and 1 <= T <= " + std::to_string(kImageAttnMaxT));
        E2V_REQUIRE(ldqkv >= 3 * heads * 64 && ldqkv % 4 == 0 && ldo >= heads * 64 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                    E2V_EINVAL, "image attention: qkv rows of q | k | v (16-byte aligned, ldqkv a multiple of 4), out rows of heads * 64 columns");
    }, [&] {
        OpRecord rec;
        image_attention(qkv, ldqkv, out, ldo, B, T, heads, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

// VideoMAEImageProcessor + VideoMAEForVideoClassification + softmax + top 3 of every clip (video_classify_metric's classifier half)
e2v_status e2v_video_classify(e2v_ctx* c, const void* frames, int kind, int n, int F, int H, int W, float* logits, float* probs,
                              int32_t* top3, e2v_stream stream) {
    return entry(c, [&] {
        check_frames("e2v_video_classify", frames, kind, n, F, H, W);
        E2V_REQUIRE(logits || probs || top3, E2V_EINVAL, "e2v_video_classify: logits, probs and top3 are all NULL");
        E2V_REQUIRE(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(probs) | reinterpret_cast<uintptr_t>(top3)) & 3) == 0,
                    E2V_EINVAL, "e2v_video_classify: misaligned output (4 bytes)");
        if (c->cfg.vmae_layers > 0) {
            E2V_REQUIRE(F == c->cfg.vmae_num_frames, E2V_ESHAPE,
                        "e2v_video_classify: F = " + std::to_string(F) + " frames per clip, the model takes vmae_num_frames = " +
                            std::to_string(c->cfg.vmae_num_frames) + " (the position table and the token count are sized by it)");
            E2V_REQUIRE(c->prep_plan(e2v_ctx::VIDEO, H, W).band >= 1, E2V_ESHAPE,
                        "e2v_video_classify: the source rows of one output row do not fit the preprocess kernel's LDS band (downscale too strong)");
        }
        c->require_part(e2v_ctx::VIDEO);
        c->require_ready(e2v_ctx::VIDEO);
    }, [&] {
        const FrameSrc src = frame_src(frames, kind);
        c->video_classify(src, n, F, H, W, logits, probs, top3, S(c, stream));
    });
}

// the preprocess of e2v_video_classify on its own, at any (S, P, ts, edge) and with the caller's pixel table
e2v_status e2v_op_video_preprocess(e2v_ctx* c, const void* frames, int kind, int n, int F, int H, int W, int size, int patch, int ts, int edge,
                                   const float* host_lut, float* rows, e2v_stream stream) {
    PrepPlan plan;
    return entry(c, [&] {
        check_frames("e2v_op_video_preprocess", frames, kind, n, F, H, W);
        E2V_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 3) == 0, E2V_EINVAL, "e2v_op_video_preprocess: null or misaligned rows");
        E2V_REQUIRE(size >= 1 && size <= 4096 && patch >= 1 && size % patch == 0 && edge >= size && edge <= 4096, E2V_ESHAPE,
                    "e2v_op_video_preprocess: 1 <= S <= edge <= 4096, S a multiple of P >= 1");
        E2V_REQUIRE(ts >= 1 && F % ts == 0 && F <= 4096, E2V_ESHAPE, "e2v_op_video_preprocess: F must be a multiple of ts >= 1, at most 4096");
        E2V_REQUIRE(host_lut || c->cfg.vmae_layers > 0, E2V_ESTATE, "e2v_op_video_preprocess: no pixel table given and the config has no video classifier");
        plan = prep_plan(H, W, video_crop(H, W, edge, size), size, patch, host_lut ? host_lut : c->video_lut, kResizeBilinear);
        E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, "e2v_op_video_preprocess: the source rows of one output row do not fit the kernel's LDS band");
    }, [&] {
        run_preprocess(c, "video_preprocess", plan, frames, kind, n, F, ts, (long long)std::max(1, 4096 / F) * F, patch, 0, rows, S(c, stream));      // (whole clips)
    });
}

// CLIPImageProcessor + CLIPVisionModelWithProjection.image_embeds of every frame (the model half of clip_score)
e2v_status e2v_clip_embed(e2v_ctx* c, const void* frames, int kind, int n, int F, int H, int W, float* embeds, e2v_stream stream) {
    return entry(c, [&] {
        check_frames("e2v_clip_embed", frames, kind, n, F, H, W);
        E2V_REQUIRE(embeds && (reinterpret_cast<uintptr_t>(embeds) & 3) == 0, E2V_EINVAL, "e2v_clip_embed: null or misaligned embeds (4 bytes)");
        c->require_part(e2v_ctx::CLIPV);
        E2V_REQUIRE(c->prep_plan(e2v_ctx::CLIPV, H, W).band >= 1, E2V_ESHAPE,
                    "e2v_clip_embed: the source rows of one output row do not fit the preprocess kernel's LDS band (downscale too strong)");
        c->require_ready(e2v_ctx::CLIPV);
    }, [&] {
        const FrameSrc src = frame_src(frames, kind);
        c->clip_embed(src, n, F, H, W, embeds, S(c, stream));
    });
}

// torch.nn.functional.cosine_similarity(a, b, dim=-1, eps=1e-8) of rows, pairwise or as a matrix
e2v_status e2v_clip_similarity(e2v_ctx* c, const float* a, int na, const float* b, int nb, int D, int matrix, float* out, e2v_stream stream) {
    return entry(c, [&] {
        E2V_REQUIRE(a && b && out, E2V_EINVAL, "e2v_clip_similarity: null argument");
        E2V_REQUIRE(matrix == 0 || matrix == 1, E2V_EINVAL, "e2v_clip_similarity: matrix is 0 (pairs) or 1");
        E2V_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0,
                    E2V_EINVAL, "e2v_clip_similarity: a and b must be 16-byte aligned, out 4-byte aligned");
        E2V_REQUIRE(na >= 1 && nb >= 1 && D >= 4 && D % 4 == 0, E2V_ESHAPE, "e2v_clip_similarity: na, nb >= 1 and D a positive multiple of 4");
        E2V_REQUIRE(matrix || na == nb, E2V_ESHAPE, "e2v_clip_similarity: the pair form takes as many rows of a as of b");
        E2V_REQUIRE(!matrix || (na + 15) / 16 <= 65535, E2V_ESHAPE, "e2v_clip_similarity: at most 65535 * 16 rows of a in the matrix form");
        E2V_REQUIRE(c->device >= 0, E2V_ESTATE, "e2v_clip_similarity: a host-only context has no device");
    }, [&] {
        clip_similarity(a, na, b, nb, D, matrix != 0, 1e-8f, out, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

// the preprocess of e2v_clip_embed on its own, at any (S, P, edge, filter) and with the caller's pixel table
e2v_status e2v_op_clip_preprocess(e2v_ctx* c, const void* frames, int kind, int n, int F, int H, int W, int size, int patch, int edge,
                                  int filter, const float* host_lut, float* rows, e2v_stream stream) {
    PrepPlan plan;
    return entry(c, [&] {
        check_frames("e2v_op_clip_preprocess", frames, kind, n, F, H, W);
        E2V_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 3) == 0, E2V_EINVAL, "e2v_op_clip_preprocess: null or misaligned rows");
        E2V_REQUIRE(filter == kResizeBilinear || filter == kResizeBicubic, E2V_EINVAL, "e2v_op_clip_preprocess: filter 2 (BILINEAR) or 3 (BICUBIC)");
        E2V_REQUIRE(size >= 1 && size <= 4096 && patch >= 1 && size % patch == 0 && edge >= size && edge <= 4096, E2V_ESHAPE,
                    "e2v_op_clip_preprocess: 1 <= S <= edge <= 4096, S a multiple of P >= 1");
        E2V_REQUIRE(host_lut || c->vcfg.clipv_layers > 0, E2V_ESTATE, "e2v_op_clip_preprocess: no pixel table given and the context has no CLIP vision tower");
        plan = prep_plan(H, W, video_crop(H, W, edge, size), size, patch, host_lut ? host_lut : c->clipv_lut, filter);
        E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, "e2v_op_clip_preprocess: the source rows of one output row do not fit the kernel's LDS band");
    }, [&] {
        run_preprocess(c, "video_preprocess", plan, frames, kind, n, F, 1, 4096, patch, 0, rows, S(c, stream));
    });
}

// fp32 in every compute mode, as e2v_video_classify runs it
e2v_status e2v_op_token_attention(e2v_ctx* c, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, e2v_stream stream) {
    return entry(c, [&] {
        E2V_REQUIRE(qkv && out, E2V_EINVAL, "null argument");
        E2V_REQUIRE(B > 0 && heads > 0 && T >= 1, E2V_ESHAPE, "token attention: B, heads, T >= 1");
        E2V_REQUIRE(ldqkv >= 3 * heads * 64 && ldqkv % 4 == 0 && ldo >= heads * 64 && ldo % 4 == 0 && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0 &&
                        (reinterpret_cast<uintptr_t>(out) & 15) == 0,
                    E2V_EINVAL, "token attention: qkv rows of q | k | v, out rows of heads * 64 columns, both 16-byte aligned with strides that are multiples of 4");
    }, [&] {
        OpRecord rec;
        token_attention(qkv, ldqkv, out, ldo, B, T, heads, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

// ---- the metric towers in a 16-bit mode (e2v_set_tower_dtype) and the pieces of that path on their own ----------------------------
namespace {
int tower_mode_of(int dtype) { return dtype == E2V_BF16 ? H16_BF16 : dtype == E2V_F16 ? H16_FP16 : dtype == E2V_F32 ? H16_NONE : -1; }
void require_h16(const char* who, int dtype) {
    E2V_REQUIRE(dtype == E2V_BF16 || dtype == E2V_F16, E2V_EINVAL, std::string(who) + ": dtype is E2V_BF16 or E2V_F16");
}
}  // namespace

e2v_status e2v_set_tower_dtype(e2v_ctx* c, int part, int dtype) {
    if (!c) return E2V_EINVAL;
    const int slot = e2v_ctx::tower_part(part), mode = tower_mode_of(dtype);
    if (slot < 0 || mode < 0) {
        c->err = "e2v_set_tower_dtype: part is 16 (image classifier), 32 (video classifier) or 64 (CLIP vision tower); dtype is E2V_F32, E2V_BF16 or E2V_F16";
        return E2V_EINVAL;
    }
    if (!c->has_part((e2v_ctx::Part)slot)) {
        c->err = "e2v_set_tower_dtype: the context has no such tower (part " + std::to_string(part) + ")";
        return E2V_ESTATE;
    }
    c->tower_h16[slot] = mode;
    return E2V_OK;
}

int e2v_tower_dtype(const e2v_ctx* c, int part) {
    const int slot = e2v_ctx::tower_part(part);
    if (!c || slot < 0) return -1;
    const int m = c->tower_h16[slot];
    return m == H16_BF16 ? E2V_BF16 : m == H16_FP16 ? E2V_F16 : E2V_F32;
}

// The preprocess storing 16-bit patch rows (what a tower in that mode feeds its patch linear), widened exactly into the caller's
// fp32 `rows`: tower = 16 (the image classifier's: the whole frame), 32 (the video classifier's: ts, edge) or 64 (CLIP's: edge, filter).
e2v_status e2v_op_tower_preprocess(e2v_ctx* c, int tower, int dtype, const void* frames, int kind, int n, int F, int H, int W, int size,
                                   int patch, int ts, int edge, int filter, const float* host_lut, float* rows, e2v_stream stream) {
    PrepPlan plan;
    return entry(c, [&] {
        check_frames("e2v_op_tower_preprocess", frames, kind, n, F, H, W);
        require_h16("e2v_op_tower_preprocess", dtype);
        E2V_REQUIRE(tower == 16 || tower == 32 || tower == 64, E2V_EINVAL, "e2v_op_tower_preprocess: tower is 16, 32 or 64");
        E2V_REQUIRE(rows && (reinterpret_cast<uintptr_t>(rows) & 3) == 0 && host_lut, E2V_EINVAL, "e2v_op_tower_preprocess: null or misaligned rows, or no pixel table");
        E2V_REQUIRE(size >= 1 && size <= 4096 && patch >= 1 && size % patch == 0, E2V_ESHAPE, "e2v_op_tower_preprocess: 1 <= S <= 4096, a multiple of P >= 1");
        if (tower == 32) E2V_REQUIRE(ts >= 1 && F % ts == 0 && F <= 4096, E2V_ESHAPE, "e2v_op_tower_preprocess: F must be a multiple of ts >= 1, at most 4096");
        if (tower != 16) E2V_REQUIRE(edge >= size && edge <= 4096, E2V_ESHAPE, "e2v_op_tower_preprocess: S <= edge <= 4096");
        if (tower == 64) E2V_REQUIRE(filter == kResizeBilinear || filter == kResizeBicubic, E2V_EINVAL, "e2v_op_tower_preprocess: filter 2 (BILINEAR) or 3 (BICUBIC)");
        plan = prep_plan(H, W, tower == 16 ? PrepWindow{size, size, 0, 0} : video_crop(H, W, edge, size), size, patch, host_lut,
                         tower == 64 ? filter : kResizeBilinear);
        E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, "e2v_op_tower_preprocess: the source rows of one output row do not fit the kernel's LDS band");
    }, [&] {
        const long long step = tower == 32 ? (long long)std::max(1, 4096 / F) * F : 4096;     // frames per launch (whole clips for the tubelets)
        run_preprocess(c, tower == 16 ? "image_preprocess" : "video_preprocess", plan, frames, kind, n, F, tower == 32 ? ts : 1, step, patch,
                       tower_mode_of(dtype), rows, S(c, stream));
    });
}

// Attention as a tower in 16-bit mode runs it: qkv [B*T][ldqkv] (q | k | v of heads * 64 columns) rounded once to `dtype`, then
// flash_attention on the 16-bit rows (mode 1, F = 1, Nq = Nk = T, head dim 64, scale 1/8), the 16-bit output widened exactly.
e2v_status e2v_op_tower_attention(e2v_ctx* c, int dtype, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads,
                                  e2v_stream stream) {
    return entry(c, [&] {
        require_h16("e2v_op_tower_attention", dtype);
        E2V_REQUIRE(qkv && out, E2V_EINVAL, "null argument");
        E2V_REQUIRE(B > 0 && heads > 0 && T >= 1 && (double)B * T < 2147483648.0, E2V_ESHAPE, "tower attention: B, heads, T >= 1");
        E2V_REQUIRE(ldqkv >= 3 * heads * 64 && ldo >= heads * 64, E2V_EINVAL, "tower attention: qkv rows of q | k | v, out rows of heads * 64 columns");
    }, [&] {
        hipStream_t s = S(c, stream);
        const int mode = tower_mode_of(dtype), C = heads * 64;
        const int64_t M = (int64_t)B * T;
        OpRecord rec;
        Act b(c->pool, M, 3 * C, true), o(c->pool, M, C, true);
        cvt_rows(qkv, ldqkv, 0, b.p, 3 * C, mode, M, 3 * C, 3 * C, s);
        AttnArgs a;
        a.q = b.at(0); a.ldq = 3 * C; a.k = b.at(C); a.v = b.at(2 * C); a.ldkv = 3 * C; a.o = o.p; a.ldo = C;
        a.n = B; a.F = 1; a.heads = heads; a.D = 64; a.Nq = T; a.Nk = T; a.mode = 1; a.scale = 0.125f; a.io_bf16 = mode;
        flash_attention(a, s);
        cvt_rows(o.p, C, mode, out, ldo, 0, M, C, C, s);
        E2V_HIP(hipGetLastError());
    });
}

// token_mean over 16-bit rows: x [B*T][C] fp32 rounded once to `dtype`, out [B][C] fp32 (the sum in index order, fp32)
e2v_status e2v_op_tower_token_mean(e2v_ctx* c, int dtype, const float* x, int B, int T, int C, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        require_h16("e2v_op_tower_token_mean", dtype);
        E2V_REQUIRE(x && out && B >= 1 && B <= 65535 && T >= 1 && C >= 1, E2V_EINVAL, "tower token mean: null argument or bad sizes");
        hipStream_t s = S(c, stream);
        const int mode = tower_mode_of(dtype);
        Act b(c->pool, (int64_t)B * T, C, true);
        cvt_rows(x, C, 0, b.p, C, mode, (int64_t)B * T, C, C, s);
        token_mean(b.p, out, B, T, C, s, mode);
        E2V_HIP(hipGetLastError());
    });
}

// The LayerNorm in front of a tower's head in 16-bit mode: x [total_rows][C] fp32 rounded once to `dtype`; rows 0, stride, 2 stride, ...
// (`rows` of them, stride in ROWS: a tower's class rows are T apart) are normalised into out [rows][C] fp32, not rounded.
e2v_status e2v_op_tower_layernorm(e2v_ctx* c, int dtype, const float* x, int64_t rows, int stride, int C, const float* gamma,
                                  const float* beta, float eps, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        require_h16("e2v_op_tower_layernorm", dtype);
        E2V_REQUIRE(x && gamma && beta && out && rows >= 1 && stride >= 1 && C % 4 == 0 && C >= 4 && C <= 1280 && (double)stride * C < 2147483648.0 &&
                        (double)rows * stride < 2147483648.0,
                    E2V_EINVAL, "tower layernorm: null argument or bad sizes (C a multiple of 4 up to 1280)");
        hipStream_t s = S(c, stream);
        const int mode = tower_mode_of(dtype);
        const int64_t total = (rows - 1) * stride + 1;
        OpRecord rec;
        Act b(c->pool, total, C, true);
        cvt_rows(x, C, 0, b.p, C, mode, total, C, C, s);
        layernorm_f32_out(b.p, stride * C, gamma, beta, out, C, (int)rows, C, eps, s, mode);
        E2V_HIP(hipGetLastError());
    });
}

// The MLP activation on 16-bit storage: x [count] fp32 rounded once to `dtype`, act (0 quick-GELU, 1 erf GELU) in fp32, rounded
// once more at the store; out [count] fp32 = the stored values widened.  count a multiple of 8.
e2v_status e2v_op_tower_activation(e2v_ctx* c, int dtype, const float* x, int64_t count, int act, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        require_h16("e2v_op_tower_activation", dtype);
        E2V_REQUIRE(x && out && count >= 8 && count % 8 == 0 && (act == 0 || act == 1), E2V_EINVAL, "tower activation: count a positive multiple of 8, act 0 or 1");
        hipStream_t s = S(c, stream);
        const int mode = tower_mode_of(dtype);
        Act b(c->pool, count / 8, 8, true);
        cvt_rows(x, 8, 0, b.p, 8, mode, count / 8, 8, 8, s);
        text_activation(b.p, count, act, s, mode);
        cvt_rows(b.p, 8, mode, out, 8, 0, count / 8, 8, 8, s);
        E2V_HIP(hipGetLastError());
    });
}

// The token rows of a tower in 16-bit mode (token_embed): patches [nimg*(T-1)][C] (cls != NULL: a class row in front) or [nimg*T][C]
// (cls == NULL) fp32 rounded once to `dtype`; cls [C] and pos [T][C] stay fp32; out [nimg*T][C] fp32 = the stored rows widened.
e2v_status e2v_op_tower_embed(e2v_ctx* c, int dtype, const float* patches, const float* cls, const float* pos, int nimg, int T, int C,
                              float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        require_h16("e2v_op_tower_embed", dtype);
        E2V_REQUIRE(patches && pos && out && nimg >= 1 && T >= (cls ? 2 : 1) && C >= 4 && C % 4 == 0 && (double)nimg * T < 2147483648.0, E2V_EINVAL,
                    "tower embed: null argument or bad sizes (C a multiple of 4)");
        hipStream_t s = S(c, stream);
        const int mode = tower_mode_of(dtype);
        const int64_t prow = (int64_t)nimg * (cls ? T - 1 : T), M = (int64_t)nimg * T;
        Act p16(c->pool, prow, C, true), x16(c->pool, M, C, true);
        cvt_rows(patches, C, 0, p16.p, C, mode, prow, C, C, s);
        token_embed(p16.p, cls, pos, x16.p, nimg, T, C, s, mode);
        cvt_rows(x16.p, C, mode, out, C, 0, M, C, C, s);
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_profile_begin(e2v_ctx* c) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] { E2V_HIP(hipDeviceSynchronize()); profiler().begin(); });
}

int64_t e2v_profile_end(e2v_ctx* c, char* json, int64_t cap) {
    if (!c || !json || cap <= 0) return -1;
    const std::string s = profiler().end_json();
    const int64_t n = (int64_t)s.size() < cap - 1 ? (int64_t)s.size() : cap - 1;
    std::memcpy(json, s.data(), (size_t)n);
    json[n] = 0;
    return (int64_t)s.size();
}

e2v_status e2v_set_compute_dtype(e2v_ctx* c, int dtype) {
    if (!c || (dtype != E2V_F32 && dtype != E2V_BF16 && dtype != E2V_F16 && dtype != E2V_F32X3)) return E2V_EINVAL;
    if (dtype == E2V_F32X3 && (c->ready[e2v_ctx::UNET] || c->ready[e2v_ctx::VAE] || c->ready[e2v_ctx::SEM])) {
        c->err = "E2V_F32X3 needs the split weights: select it before e2v_finalize_weights";
        return E2V_ESTATE;
    }
    c->set_h16_mode(dtype == E2V_BF16 ? H16_BF16 : dtype == E2V_F16 ? H16_FP16 : H16_NONE);
    c->x3_compute = dtype == E2V_F32X3;
    return E2V_OK;
}

e2v_status e2v_set_conv_algo(e2v_ctx* c, int algo) {
    if (!c || algo < E2V_CONV_AUTO || algo > E2V_CONV_WINOGRAD4) return E2V_EINVAL;
    c->conv_algo = algo;
    return E2V_OK;
}

int64_t e2v_device_bytes(const e2v_ctx* c) { return c ? (int64_t)(c->weight_bytes() + c->pool.bytes()) : 0; }

// ---------------------------------------------------------------------------------------------------
// The body of the three UNet entry points: NCFHW in, unet_forward_cl, NCFHW out.  host_tf != null: fractional timesteps;
// sink != null: the taps of e2v_op_unet_forward_taps are collected on the way.
static void unet_forward_ncfhw(e2v_ctx* c, const float* sample, const int64_t* host_t, const float* host_tf, int n_t, const float* cond,
                               int N, int F, int H, int W, int T, float* out, e2v_ctx::TapSink* sink, e2v_stream stream) {
    E2V_REQUIRE(sample && (host_t || host_tf) && cond && out && (!sink || sink->buf), E2V_EINVAL, "null argument");
    E2V_REQUIRE(N > 0 && F > 0 && H > 0 && W > 0 && T > 0 && (!sink || sink->cap > 0), E2V_ESHAPE, "non-positive dimension");
    hipStream_t s = S(c, stream);
    const int Cin = c->cfg.in_channels, Cout = c->cfg.out_channels;
    const int FHW = F * H * W;
    struct Guard { e2v_ctx* c; ~Guard() { c->tap_sink = nullptr; } } guard{c};
    c->tap_sink = sink;
    Act x(c->pool, (int64_t)N * FHW, Cin);
    ncfhw_to_cl(sample, x.p, N, Cin, Cin, FHW, 1.0f, s);
    Act y = c->unet_forward_cl(x.p, host_t, n_t, cond, N, F, H, W, T, s, false, host_tf);
    cl_to_ncfhw(y.p, Cout, out, N, Cout, FHW, 1.0f, 0.0f, 0, 0.f, 0.f, s);
    E2V_HIP(hipGetLastError());
}

e2v_status e2v_unet_forward(e2v_ctx* c, const float* sample, const int64_t* host_t, int n_t, const float* cond, int N,
                            int F, int H, int W, int T, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] { unet_forward_ncfhw(c, sample, host_t, nullptr, n_t, cond, N, F, H, W, T, out, nullptr, stream); });
}

// Test aid (eeg2video_hip_ops.h): the forward above with the block outputs the oracle exposes copied out on the way.
e2v_status e2v_op_unet_forward_taps(e2v_ctx* c, const float* sample, const int64_t* host_t, int n_t, const float* cond, int N,
                                    int F, int H, int W, int T, float* out, float* taps, int64_t taps_cap, int64_t* shapes,
                                    int* n_taps, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(host_t && shapes && n_taps, E2V_EINVAL, "null argument");
        e2v_ctx::TapSink sink;
        sink.buf = taps; sink.cap = taps_cap;
        unet_forward_ncfhw(c, sample, host_t, nullptr, n_t, cond, N, F, H, W, T, out, &sink, stream);
        *n_taps = sink.count;
        for (int i = 0; i < sink.count; ++i)
            for (int k = 0; k < 5; ++k) shapes[5 * i + k] = sink.shapes[i][k];
    });
}

e2v_status e2v_unet_forward_ft(e2v_ctx* c, const float* sample, const float* host_t, int n_t, const float* cond, int N,
                               int F, int H, int W, int T, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] { unet_forward_ncfhw(c, sample, nullptr, host_t, n_t, cond, N, F, H, W, T, out, nullptr, stream); });
}

static void ddim_coeffs(const e2v_ctx* c, int64_t t, int64_t t_prev, float co[4]) {
    E2V_REQUIRE(t >= 0 && t < (int64_t)c->alphas.size() && t_prev < (int64_t)c->alphas.size(), E2V_EINVAL, "timestep out of range");
    const float a_t = c->alphas[(size_t)t];
    const float a_p = t_prev >= 0 ? c->alphas[(size_t)t_prev] : c->alphas[0];   // final_alpha_cumprod (set_alpha_to_one = False)
    co[0] = std::sqrt(a_t);
    co[1] = std::sqrt(1.0f - a_t);
    co[2] = std::sqrt(a_p);
    co[3] = std::sqrt(1.0f - a_p);
}

e2v_status e2v_ddim_cfg_step(e2v_ctx* c, const float* eu, const float* ec, const float* x, float* xo, int64_t count,
                             float g, int64_t t, int64_t t_prev, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(eu && x && xo && count >= 0, E2V_EINVAL, "null argument");
        float co[4];
        ddim_coeffs(c, t, t_prev, co);
        ddim_cfg_step(eu, ec, x, xo, count, g, co[0], co[1], co[2], co[3], S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

static void decode_to_video(e2v_ctx* c, const float* z_cl, int B, int F, int h, int w, int post, float* videos, hipStream_t s) {
    const int HW8 = 64 * h * w;
    const int C3 = c->cfg.vae_in_channels;
    Act frames(c->pool, (int64_t)B * F * HW8, C3);
    // frames are independent samples, so the grouping does not change a bit of the result.  fp32: one clip (F frames) per pass keeps
    // the workspace at ~1 clip.  bf16 mode: four -- the 36x64 levels of ONE clip (M = 13 824 rows) are 432 tiles for 512 slots; 0.6 % of
    // a B = 32 pass (same-box A/B; fp32: +-0), 0.9 GB per 288x512x128 bf16 tensor.  E2V_VAE_CLIPS_PER_PASS overrides both.
    static const int forced = [] { const char* e = std::getenv("E2V_VAE_CLIPS_PER_PASS"); return e ? std::atoi(e) : 0; }();
    const int group = forced > 0 ? forced : (c->bf16_compute ? 4 : 1);
    for (int b = 0; b < B; b += group) {
        const int nb = B - b < group ? B - b : group;
        c->vae_decode_frames(z_cl + (size_t)b * F * h * w * c->cfg.vae_latent_channels, nb * F, h, w,
                             frames.p + (size_t)b * F * HW8 * C3, s, B <= small_family_clips());      // the dispatch family is the CALL's (model.h), not the pass's; clips, not samples (ADVICE.md finding 3)
    }
    nchw_frames_to_ncfhw(frames.p, C3, videos, B, F, C3, HW8, post ? 0.5f : 1.0f, post ? 0.5f : 0.0f, post ? 1 : 0, s);
}

e2v_status e2v_vae_decode(e2v_ctx* c, const float* latents, int B, int F, int h, int w, int post, float* videos,
                          e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(latents && videos, E2V_EINVAL, "null argument");
        E2V_REQUIRE(B > 0 && F > 0 && h > 0 && w > 0, E2V_ESHAPE, "non-positive dimension");
        hipStream_t s = S(c, stream);
        const int lat = c->cfg.vae_latent_channels;
        Act z(c->pool, (int64_t)B * F * h * w, lat);
        ncfhw_to_cl(latents, z.p, B, lat, lat, F * h * w, post ? (float)(1.0 / c->cfg.vae_scaling_factor) : 1.0f, s);   // :177
        decode_to_video(c, z.p, B, F, h, w, post, videos, s);
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_vae_encode(e2v_ctx* c, const float* images, int n, int H, int W, float* mean, float* logvar, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(images && mean && logvar, E2V_EINVAL, "null argument");
        E2V_REQUIRE(n > 0 && H % 8 == 0 && W % 8 == 0 && H > 0 && W > 0, E2V_ESHAPE, "H and W must be positive multiples of 8");
        hipStream_t s = S(c, stream);
        const int Cimg = c->cfg.vae_in_channels, Cp = c->vae.enc_in.cin_pad, lat = c->cfg.vae_latent_channels;
        Act x(c->pool, (int64_t)n * H * W, Cp);
        ncfhw_to_cl(images, x.p, n, Cimg, Cp, H * W, 1.0f, s);
        const int hw = (H / 8) * (W / 8);
        Act m(c->pool, (int64_t)n * hw, 2 * lat);
        c->vae_encode_frames(x.p, n, H, W, m.p, s);
        cl_to_ncfhw(m.p, 2 * lat, mean, n, lat, hw, 1.f, 0.f, 0, 0.f, 0.f, s);
        cl_to_ncfhw(m.p + lat, 2 * lat, logvar, n, lat, hw, 1.f, 0.f, 1, -30.f, 20.f, s);
        E2V_HIP(hipGetLastError());
    });
}

// ---- the denoising loop (pipeline_tuneeeg2video.py:311-334), shared by e2v_generate and e2v_generate_plan -------------------------
// Everything both loops do lives here: the [uncond ; cond] assembly, the per-run caches, the guidance-pair decision, one
// unet_forward_cl per evaluation, latents_out and the decode.  What differs comes in as three callables:
//   input(i)               -> the channel-last latents [B * P][Cl] evaluation i reads
//   update(i, eps_u, eps_c) : consume the evaluation's eps (eps_c null: guidance off), B * per floats each
//   result()               -> the channel-last latents the loop ends with
struct LoopArgs {
    const float *cond, *uncond;
    int Bu, B, F, h, w, T;
    float guidance;
    float *videos, *latents_out;
};

static void check_loop_args(const LoopArgs& a, const float* latents) {
    E2V_REQUIRE(latents && a.cond, E2V_EINVAL, "null argument");
    E2V_REQUIRE(a.B > 0 && a.F > 0 && a.h > 0 && a.w > 0 && a.T > 0, E2V_ESHAPE, "non-positive dimension");
}
static void check_loop_uncond(const LoopArgs& a) {
    E2V_REQUIRE(a.guidance <= 1.0f || (a.uncond && (a.Bu == 1 || a.Bu == a.B)), E2V_EINVAL, "uncond must have batch 1 or B");
}

extern "C++" {
template <class Input, class Update, class Result>
static void denoise_loop(e2v_ctx* c, const LoopArgs& a, const std::vector<e2v_ctx::EvalTime>& ev, hipStream_t s, Input&& input,
                         Update&& update, Result&& result) {
    const int B = a.B, F = a.F, h = a.h, w = a.w, T = a.T, Bu = a.Bu;
    const bool cfg_on = a.guidance > 1.0f;                                   // pipeline_tuneeeg2video.py:281
    const int Cl = c->cfg.in_channels, D = c->cfg.cross_attention_dim;
    const int P = F * h * w;
    const size_t per = (size_t)P * Cl;
    const int N = cfg_on ? 2 * B : B;
    const int steps = (int)ev.size();

    Act emb;                                                                 // [uncond ; cond] (:162-172)
    const float* embp = a.cond;
    if (cfg_on) {
        emb = Act(c->pool, (int64_t)N * T, D);
        const size_t one = (size_t)T * D;
        if (Bu == B) E2V_HIP(hipMemcpyAsync(emb.p, a.uncond, one * B * sizeof(float), hipMemcpyDeviceToDevice, s));
        else for (int b = 0; b < B; ++b)
            E2V_HIP(hipMemcpyAsync(emb.p + b * one, a.uncond, one * sizeof(float), hipMemcpyDeviceToDevice, s));
        E2V_HIP(hipMemcpyAsync(emb.p + B * one, a.cond, one * B * sizeof(float), hipMemcpyDeviceToDevice, s));
        embp = emb.p;
    }
    // everything that depends only on (t_i, conditioning) is computed once for the whole loop
    struct CacheGuard {
        e2v_ctx* c;
        ~CacheGuard() { c->step_cache_on = false; c->temb_cache.clear(); c->kv_cache.clear(); }
    } guard{c};
    // (the family of the UNet passes this call makes, so that the caches do not depend on what an earlier call ran.  No launch in
    // there is eligible for split-K at the shipped thresholds -- cross-attention K = cross_attention_dim < 2 x 2048, the
    // time-embedding linears are fp32 rows -- so the caches are the same bits in both families)
    c->build_step_caches(ev.data(), steps, embp, N, T, unet_small_family(N), s);
    c->step_cache_on = true;
    // latent_model_input = cat([latents] * 2) (:313) is not materialised: the UNet is told that its input stands for the
    // pair, and computes what the two copies share (up to the first cross-attention) once
    const bool pair = cfg_on && !c->unet.down[0].attn.empty();
    Act xin;
    if (cfg_on && !pair) xin = Act(c->pool, (int64_t)N * P, Cl);
    for (int i = 0; i < steps; ++i) {                                        // :311
        const float* x = input(i);
        const float* in = x;
        if (cfg_on && !pair) {
            E2V_HIP(hipMemcpyAsync(xin.p, x, per * B * sizeof(float), hipMemcpyDeviceToDevice, s));
            E2V_HIP(hipMemcpyAsync(xin.p + per * B, x, per * B * sizeof(float), hipMemcpyDeviceToDevice, s));
            in = xin.p;
        }
        c->step_cache_step = i;
        Act eps = c->unet_forward_cl(in, ev[i].frac ? nullptr : &ev[i].t, 1, embp, N, F, h, w, T, s, pair,
                                     ev[i].frac ? &ev[i].tf : nullptr);      // :317
        update(i, eps.p, cfg_on ? eps.p + per * B : nullptr);               // :320-325
        // profiling aid: under rocprofv3 --pmc (ROCm 7.2) rocprofiler-sdk's queue-intercept callback faulted with a whole pass
        // (~34 000 launches, ~680 per DDIM step) queued behind the GPU (profiles/r02_pmc_async_abort_README.md names the frames);
        // E2V_SYNC_EACH_STEP=1 drains the stream after every step.  Read once per process; never set in a timed run
        static const bool sync_each = [] { const char* e = std::getenv("E2V_SYNC_EACH_STEP"); return e && std::atoi(e) != 0; }();
        if (sync_each) E2V_HIP(hipStreamSynchronize(s));
    }
    const float* x = result();
    if (a.latents_out) cl_to_ncfhw(x, Cl, a.latents_out, B, Cl, P, 1.f, 0.f, 0, 0.f, 0.f, s);
    if (a.videos) {                                                          // decode_latents (:175-184)
        Act z(c->pool, (int64_t)B * P, Cl);
        const float inv = (float)(1.0 / c->cfg.vae_scaling_factor);
        ncfhw_to_cl(x, z.p, 1, 1, 1, (int)(per * B), inv, s);            // z = 1 / 0.18215 * latents (:177), flat scale
        decode_to_video(c, z.p, B, F, h, w, 1, a.videos, s);
    }
    E2V_HIP(hipGetLastError());
}
}  // extern "C++"

e2v_status e2v_generate(e2v_ctx* c, const float* latents, const float* cond, const float* uncond, int Bu, int B, int F,
                        int h, int w, int T, int steps, float guidance, float eta, float* videos, float* latents_out,
                        e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        const LoopArgs a{cond, uncond, Bu, B, F, h, w, T, guidance, videos, latents_out};
        check_loop_args(a, latents);
        E2V_REQUIRE(steps > 0 && steps <= c->cfg.num_train_timesteps, E2V_EINVAL, "num_inference_steps out of range");
        E2V_REQUIRE(eta == 0.0f, E2V_EINVAL, "only the deterministic DDIM update (eta = 0) is implemented");
        check_loop_uncond(a);
        hipStream_t s = S(c, stream);
        const int Cl = c->cfg.in_channels, P = F * h * w;
        const long long count = (long long)P * Cl * B;
        Act x(c->pool, (int64_t)B * P, Cl);
        ncfhw_to_cl(latents, x.p, B, Cl, Cl, P, 1.0f, s);                        // init_noise_sigma = 1 (:244)
        std::vector<int64_t> ts(steps);
        e2v_ddim_timesteps(c, steps, ts.data());                                 // :287-288
        const int64_t ratio = c->cfg.num_train_timesteps / steps;
        std::vector<e2v_ctx::EvalTime> ev(steps);
        for (int i = 0; i < steps; ++i) ev[i] = e2v_ctx::EvalTime{ts[i], (float)ts[i], false};
        denoise_loop(c, a, ev, s,
                     [&](int) { return (const float*)x.p; },
                     [&](int i, const float* eu, const float* ec) {
                         float co[4];
                         ddim_coeffs(c, ts[i], ts[i] - ratio, co);
                         ddim_cfg_step(eu, ec, x.p, x.p, count, guidance, co[0], co[1], co[2], co[3], s);
                     },
                     [&] { return (const float*)x.p; });
    });
}

// ---- sampler plans (eeg2video_hip.h: e2v_plan_op) ------------------------------------------------------------------------------------
// Host-only validation: everything e2v_generate_plan / e2v_op_run_plan index memory by.  Throws E2V_EINVAL naming the op.
static int plan_check(const e2v_ctx* c, const e2v_plan_op* ops, int n_ops, int n_slots, int final_slot, int n_noise) {
    E2V_REQUIRE(ops && n_ops > 0, E2V_EINVAL, "plan: no ops");
    E2V_REQUIRE(n_slots >= 1 && n_slots <= E2V_PLAN_MAX_SLOTS, E2V_EINVAL,
                "plan: n_slots = " + std::to_string(n_slots) + " is outside 1.." + std::to_string(E2V_PLAN_MAX_SLOTS));
    E2V_REQUIRE(n_noise >= 0, E2V_EINVAL, "plan: negative n_noise");
    bool written[E2V_PLAN_MAX_SLOTS] = {true};                                   // slot 0 holds the latents on entry
    int n_unet = 0;
    for (int i = 0; i < n_ops; ++i) {
        const e2v_plan_op& op = ops[i];
        const std::string at = "plan op " + std::to_string(i) + ": ";
        E2V_REQUIRE(op.kind == E2V_PLAN_UNET || op.kind == E2V_PLAN_LINCOMB, E2V_EINVAL, at + "unknown kind " + std::to_string(op.kind));
        const int lo = 1, hi = op.kind == E2V_PLAN_UNET ? 1 : E2V_PLAN_MAX_TERMS;
        E2V_REQUIRE(op.n_src >= lo && op.n_src <= hi, E2V_EINVAL,
                    at + std::to_string(op.n_src) + " terms (" + (hi == 1 ? "a UNET op reads one slot" : "a LINCOMB op takes 1..5") + ")");
        E2V_REQUIRE(op.dst >= 0 && op.dst < n_slots, E2V_EINVAL, at + "destination slot " + std::to_string(op.dst) + " out of range");
        for (int k = 0; k < op.n_src; ++k) {
            const int src = op.src[k];
            if (src < 0) {
                E2V_REQUIRE(op.kind == E2V_PLAN_LINCOMB && -1 - (int64_t)src < n_noise, E2V_EINVAL,
                            at + "noise tensor " + std::to_string(-1 - (int64_t)src) + " out of range");
            } else {
                E2V_REQUIRE(src < n_slots, E2V_EINVAL, at + "source slot " + std::to_string(src) + " out of range");
                E2V_REQUIRE(written[src], E2V_EINVAL, at + "slot " + std::to_string(src) + " is read before any op wrote it");
                E2V_REQUIRE(src != op.dst, E2V_EINVAL, at + "writes slot " + std::to_string(src) + ", which it reads");
            }
            if (op.kind == E2V_PLAN_LINCOMB)
                E2V_REQUIRE(std::isfinite(op.coef[k]) && std::isfinite((float)op.coef[k]), E2V_EINVAL, at + "non-finite coefficient");
        }
        if (op.kind == E2V_PLAN_UNET) {
            E2V_REQUIRE(std::isfinite(op.timestep) && std::isfinite((float)op.timestep), E2V_EINVAL, at + "non-finite timestep");
            if (!op.fractional)
                E2V_REQUIRE(op.timestep == std::floor(op.timestep) && op.timestep >= 0 && op.timestep < c->cfg.num_train_timesteps,
                            E2V_EINVAL, at + "integral timestep outside [0, num_train_timesteps)");
            ++n_unet;
        }
        written[op.dst] = true;
    }
    E2V_REQUIRE(n_unet > 0, E2V_EINVAL, "plan: no UNET op");
    E2V_REQUIRE(final_slot >= 0 && final_slot < n_slots && written[final_slot], E2V_EINVAL,
                "plan: final_slot " + std::to_string(final_slot) + " is out of range or never written");
    return n_unet;
}

static e2v_status plan_checked(e2v_ctx* c, const e2v_plan_op* ops, int n_ops, int n_slots, int final_slot, const float* noise,
                               int n_noise, int* n_unet) {
    try {
        *n_unet = plan_check(c, ops, n_ops, n_slots, final_slot, n_noise);
        E2V_REQUIRE(n_noise == 0 || noise, E2V_EINVAL, "plan: n_noise > 0 needs the noise array");
        return E2V_OK;
    } catch (const Error& e) {
        c->err = e.what();
        return e.code;
    }
}

// The executor: walks the ops in order with the launchers of the stepped loop (misc.hip: lincomb, cfg_combine), the coefficients cast
// to float as e2v_lincomb's callers cast them.  Every slot is `count` floats; the layout is whatever the caller's is (the ops are
// elementwise).
struct PlanRun {
    const e2v_plan_op* ops;
    int n_ops;
    long long count;
    float guidance;
    const float* noise;                                      // [n_noise][count], in the slots' layout
    hipStream_t s;
    std::vector<Act> slot;
    int pc = 0;
    // run the LINCOMB ops up to the next UNET op (or the end); returns that op, or null
    const e2v_plan_op* advance() {
        for (; pc < n_ops && ops[pc].kind == E2V_PLAN_LINCOMB; ++pc) {
            const e2v_plan_op& op = ops[pc];
            const float* xs[E2V_PLAN_MAX_TERMS];
            float cf[E2V_PLAN_MAX_TERMS];
            for (int k = 0; k < op.n_src; ++k) {
                xs[k] = op.src[k] >= 0 ? slot[op.src[k]].p : noise + (size_t)(-1 - op.src[k]) * (size_t)count;
                cf[k] = (float)op.coef[k];
            }
            lincomb(op.n_src, xs, cf, slot[op.dst].p, count, s);
        }
        return pc < n_ops ? &ops[pc] : nullptr;
    }
    // the UNET op at pc: its dst slot receives the guided eps (:320-322), or eps itself
    void unet_result(const float* eu, const float* ec) {
        const e2v_plan_op& op = ops[pc++];
        if (ec) cfg_combine(eu, ec, guidance, slot[op.dst].p, count, s);
        else E2V_HIP(hipMemcpyAsync(slot[op.dst].p, eu, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
};

e2v_status e2v_generate_plan(e2v_ctx* c, const float* latents, const float* cond, const float* uncond, int Bu, int B, int F, int h,
                             int w, int T, const e2v_plan_op* ops, int n_ops, int n_slots, int final_slot, const float* noise,
                             int n_noise, float guidance, float* videos, float* latents_out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    int n_unet = 0;
    const e2v_status st = plan_checked(c, ops, n_ops, n_slots, final_slot, noise, n_noise, &n_unet);
    if (st != E2V_OK) return st;
    return guarded(c, [&] {
        const LoopArgs a{cond, uncond, Bu, B, F, h, w, T, guidance, videos, latents_out};
        check_loop_args(a, latents);
        check_loop_uncond(a);
        hipStream_t s = S(c, stream);
        const int Cl = c->cfg.in_channels, P = F * h * w;
        E2V_REQUIRE((int64_t)(n_noise > 0 ? n_noise : 1) * B <= INT32_MAX, E2V_ESHAPE, "n_noise * B does not fit an int");
        PlanRun run{ops, n_ops, (long long)P * Cl * B, guidance, nullptr, s, {}};
        for (int k = 0; k < n_slots; ++k) run.slot.emplace_back(c->pool, (int64_t)B * P, Cl);
        ncfhw_to_cl(latents, run.slot[0].p, B, Cl, Cl, P, 1.0f, s);
        Act noise_cl;                                        // the noise tensors in the loop's layout (exact: a permutation)
        if (n_noise > 0) {
            noise_cl = Act(c->pool, (int64_t)n_noise * B * P, Cl);
            ncfhw_to_cl(noise, noise_cl.p, n_noise * B, Cl, Cl, P, 1.0f, s);
            run.noise = noise_cl.p;
        }
        std::vector<e2v_ctx::EvalTime> ev;
        ev.reserve(n_unet);
        for (int i = 0; i < n_ops; ++i)
            if (ops[i].kind == E2V_PLAN_UNET)
                ev.push_back(e2v_ctx::EvalTime{(int64_t)ops[i].timestep, (float)ops[i].timestep, ops[i].fractional != 0});
        denoise_loop(c, a, ev, s,
                     [&](int) { return (const float*)run.slot[run.advance()->src[0]].p; },
                     [&](int, const float* eu, const float* ec) { run.unet_result(eu, ec); },
                     [&] { run.advance(); return (const float*)run.slot[final_slot].p; });
    });
}

// Test aid (eeg2video_hip_ops.h): the executor above with the UNet's results handed in.
e2v_status e2v_op_run_plan(e2v_ctx* c, const e2v_plan_op* ops, int n_ops, int n_slots, int final_slot, const float* x0,
                           const float* eps_u, const float* eps_c, int n_unet, const float* noise, int n_noise, float guidance,
                           float* out, int64_t count, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    int plan_unet = 0;
    const e2v_status st = plan_checked(c, ops, n_ops, n_slots, final_slot, noise, n_noise, &plan_unet);
    if (st != E2V_OK) return st;
    if (plan_unet != n_unet) { c->err = "plan: " + std::to_string(plan_unet) + " UNET ops, eps arrays of " + std::to_string(n_unet); return E2V_EINVAL; }
    return guarded(c, [&] {
        const bool cfg_on = guidance > 1.0f;
        E2V_REQUIRE(x0 && eps_u && out && count > 0 && (!cfg_on || eps_c), E2V_EINVAL, "null argument");
        hipStream_t s = S(c, stream);
        PlanRun run{ops, n_ops, (long long)count, guidance, noise, s, {}};
        for (int k = 0; k < n_slots; ++k) run.slot.emplace_back(c->pool, count, 1);
        E2V_HIP(hipMemcpyAsync(run.slot[0].p, x0, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, s));
        for (int k = 0; run.advance(); ++k)
            run.unet_result(eps_u + (size_t)k * count, cfg_on ? eps_c + (size_t)k * count : nullptr);
        E2V_HIP(hipMemcpyAsync(out, run.slot[final_slot].p, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, s));
        E2V_HIP(hipGetLastError());
    });
}

int64_t e2v_plan_op_size(void) { return (int64_t)sizeof(e2v_plan_op); }

// ---- which kernel and tile every launch of a configuration takes, without a GPU -----------------------------------------------------
// Runs e2v_generate (one DDIM step with guidance + decode) of B clips of [4, F, h, w] latents as a DRY RUN on a host-only ctx: the
// graph walker, the launch rules of every launcher and the per-layer decisions execute exactly as in a real call, no HIP call is
// made, and every launch leaves one record "class shape -> kernel tile".  Output: one line per distinct record in first-occurrence
// order, "<count>x <record>\n".  A rule change shows up as a diff of this text (tests/golden/dispatch_sd_v1_4.json).
e2v_status e2v_op_describe_dispatch(e2v_ctx* c, int dtype, int B, int F, int h, int w, int T, char* buf, int64_t cap, int64_t* needed) {
    if (!c || !needed || (dtype != E2V_F32 && dtype != E2V_BF16 && dtype != E2V_F16) || B <= 0 || F <= 0 || h <= 0 || w <= 0 || T <= 0 || (cap > 0 && !buf)) return E2V_EINVAL;
    if (c->device >= 0) { c->err = "e2v_op_describe_dispatch runs on a host-only context (e2v_create(..., device = -1, ...))"; return E2V_ESTATE; }
    struct Dry {
        Dry() { dry_run() = true; dry_log().clear(); }
        ~Dry() { dry_run() = false; dry_log().clear(); }
    } dry;
    e2v_status st = guarded(c, [&] {
        if (!c->ready[e2v_ctx::UNET] || !c->ready[e2v_ctx::VAE]) c->finalize(3);
    });
    if (st != E2V_OK) return st;
    const int was_mode = c->h16_mode;
    c->set_h16_mode(dtype == E2V_BF16 ? H16_BF16 : dtype == E2V_F16 ? H16_FP16 : H16_NONE);
    dry_log().clear();
    const float* fake = dry_fake_ptr(1 << 20);
    st = e2v_generate(c, fake, fake, fake, 1, B, F, h, w, T, 1, 12.5f, 0.0f, dry_fake_ptr(1 << 20), nullptr, nullptr);
    c->set_h16_mode(was_mode);
    if (st != E2V_OK) return st;
    std::vector<std::pair<std::string, long>> agg;
    std::unordered_map<std::string, size_t> at;
    for (const std::string& r : dry_log()) {
        auto it = at.find(r);
        if (it == at.end()) { at.emplace(r, agg.size()); agg.emplace_back(r, 1); }
        else agg[it->second].second += 1;
    }
    std::string out;
    for (const auto& kv : agg) out += std::to_string(kv.second) + "x " + kv.first + "\n";
    *needed = (int64_t)out.size() + 1;
    if (cap >= *needed) std::memcpy(buf, out.c_str(), out.size() + 1);
    return E2V_OK;
}

// ---- building blocks of the schedulers other than DDIM (pipeline_tuneeeg2video.py:48-55) -----------
e2v_status e2v_cfg_combine(e2v_ctx* c, const float* eu, const float* ec, float g, float* out, int64_t count, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(eu && ec && out && count >= 0, E2V_EINVAL, "null argument");
        cfg_combine(eu, ec, g, out, count, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_lincomb(e2v_ctx* c, int n, const float* const* xs, const float* coefs, float* out, int64_t count, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(n >= 1 && n <= 5 && xs && coefs && out && count >= 0, E2V_EINVAL, "lincomb takes 1..5 terms");
        for (int k = 0; k < n; ++k) E2V_REQUIRE(xs[k] != nullptr, E2V_EINVAL, "null term");
        lincomb(n, xs, coefs, out, count, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

// ---- DDIM inversion (EEG2Video_New/Generation/tuneavideo/util.py:56-101) --------------------------
// next_step: "timestep" = t - T/n (alpha of the step being left; < 0 -> final_alpha_cumprod), "next_timestep" = t.
static void ddim_next_coeffs(const e2v_ctx* c, int64_t t, int steps, float co[4]) {
    const int64_t T = c->cfg.num_train_timesteps;
    E2V_REQUIRE(steps > 0 && steps <= T, E2V_EINVAL, "num_inference_steps out of range");
    E2V_REQUIRE(t >= 0 && t < (int64_t)c->alphas.size(), E2V_EINVAL, "timestep out of range");
    const int64_t cur = std::min<int64_t>(t - T / steps, 999);                     // util.py:58-59
    const float a_t = cur >= 0 ? c->alphas[(size_t)cur] : c->alphas[0];           // :60 (set_alpha_to_one = False)
    const float a_n = c->alphas[(size_t)t];                                        // :61
    co[0] = std::sqrt(a_t);
    co[1] = std::sqrt(1.0f - a_t);
    co[2] = std::sqrt(a_n);
    co[3] = std::sqrt(1.0f - a_n);
}

e2v_status e2v_ddim_next_step(e2v_ctx* c, const float* eps, const float* x, float* xo, int64_t count, int64_t t,
                              int num_inference_steps, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(eps && x && xo && count >= 0, E2V_EINVAL, "null argument");
        float co[4];
        ddim_next_coeffs(c, t, num_inference_steps, co);
        ddim_cfg_step(eps, nullptr, x, xo, count, 1.0f, co[0], co[1], co[2], co[3], S(c, stream));   // :63-65, same form as step()
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_ddim_invert(e2v_ctx* c, const float* latents, const float* cond, int B, int F, int h, int w, int T,
                           int num_inv_steps, float* all_latents, float* final_latent, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(latents && cond && (all_latents || final_latent), E2V_EINVAL, "null argument");
        E2V_REQUIRE(B > 0 && F > 0 && h > 0 && w > 0 && T > 0, E2V_ESHAPE, "non-positive dimension");
        E2V_REQUIRE(num_inv_steps > 0 && num_inv_steps <= c->cfg.num_train_timesteps, E2V_EINVAL, "num_inv_steps out of range");
        hipStream_t s = S(c, stream);
        const int Cl = c->cfg.in_channels;
        const int P = F * h * w;
        const size_t per = (size_t)B * P * Cl;
        Act x(c->pool, (int64_t)B * P, Cl);
        ncfhw_to_cl(latents, x.p, B, Cl, Cl, P, 1.0f, s);
        if (all_latents) E2V_HIP(hipMemcpyAsync(all_latents, latents, per * sizeof(float), hipMemcpyDeviceToDevice, s));   // all_latent = [latent] (:86)
        std::vector<int64_t> ts(num_inv_steps);
        e2v_ddim_timesteps(c, num_inv_steps, ts.data());
        for (int i = 0; i < num_inv_steps; ++i) {                                 // :88
            const int64_t t = ts[num_inv_steps - 1 - i];                          // timesteps[len - i - 1] (:89): ascending
            Act eps = c->unet_forward_cl(x.p, &t, 1, cond, B, F, h, w, T, s);     // get_noise_pred_single (:68-70), no guidance
            float co[4];
            ddim_next_coeffs(c, t, num_inv_steps, co);
            ddim_cfg_step(eps.p, nullptr, x.p, x.p, (long long)per, 1.0f, co[0], co[1], co[2], co[3], s);   // next_step (:91)
            if (all_latents) cl_to_ncfhw(x.p, Cl, all_latents + (size_t)(i + 1) * per, B, Cl, P, 1.f, 0.f, 0, 0.f, 0.f, s);
        }
        if (final_latent) cl_to_ncfhw(x.p, Cl, final_latent, B, Cl, P, 1.f, 0.f, 0, 0.f, 0.f, s);
        E2V_HIP(hipGetLastError());
    });
}

// ---------------------------------------------------------------------------------------------------
// kernel-level entry points (eeg2video_hip_ops.h)
// ---------------------------------------------------------------------------------------------------
e2v_status e2v_op_conv3x3(e2v_ctx* c, const float* x0, int c0, const float* x1, int c1, int n_img, int Hs, int Ws, int Hi,
                          int Wi, int Ho, int Wo, int stride, int pad_lo, const float* w_oihw, const float* bias, int cout,
                          const float* rowbias, int rows_per_sample, const float* resid, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(x0 && w_oihw && out && c0 % 4 == 0 && c1 % 4 == 0 && c0 > 0, E2V_EINVAL, "bad conv arguments");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        const int cin = c0 + c1;
        E2V_REQUIRE(c1 == 0 || c0 % 32 == 0, E2V_ESHAPE, "conv: the concat seam must be a multiple of 32 channels");
        Conv3 d;                     // the launch as the graph runner describes it (model.h); the weight forms are pool temporaries here
        d.x0 = x0; d.c0 = c0; d.x1 = x1; d.c1 = c1; d.nimg = n_img; d.Hs = Hs; d.Ws = Ws;
        d.Hi = Hi; d.Wi = Wi; d.Ho = Ho; d.Wo = Wo; d.stride = stride; d.pad = pad_lo;
        d.cout = cout; d.out = out; d.bias = bias;
        d.rowbias = rowbias; d.rb_ld = cout; d.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; d.resid = resid;
        if (c->bf16_compute) {       // bf16-activation mode: operands rounded to bf16 once (channels zero-padded to 8), fp32 result
            E2V_REQUIRE(c1 == 0 || c0 % 64 == 0, E2V_ESHAPE, "bf16 conv: the concat seam must be a multiple of 64 channels");
            const int c0p = c1 > 0 ? c0 : (c0 + 7) / 8 * 8, c1p = (c1 + 7) / 8 * 8;
            const int64_t rows_in = (int64_t)n_img * Hs * Ws;
            Act a0(c->pool, rows_in, c0p, true), a1;
            cvt_rows(x0, c0, 0, a0.p, c0p, c->h16_mode, rows_in, c0, c0p, s);
            if (c1 > 0) { a1 = Act(c->pool, rows_in, c1p, true); cvt_rows(x1, c1, 0, a1.p, c1p, c->h16_mode, rows_in, c1, c1p, s); }
            const int ld64 = conv3x3_packed_ld(cin, 64);
            Act w64(c->pool, cout, ld64), w16(c->pool, cout, (ld64 + 1) / 2);
            pack_conv3x3(w_oihw, w64.p, cout, cin, 64, s);
            to_h16(w64.p, w16.p, (size_t)cout * ld64, c->h16_mode, s);
            d.x0 = a0.p; d.c0 = c0p; d.x1 = a1.p; d.c1 = c1p;
            const bool io16 = op_io16(c);                  // the graph's launch: 16-bit output tensor, 16-bit residual
            const int64_t rows_out = (int64_t)n_img * Ho * Wo;
            Act o16, r16;
            if (io16) {
                o16 = Act(c->pool, rows_out, cout, true);
                d.out = o16.p;
                if (resid) { r16 = Act(c->pool, rows_out, cout, true); cvt_rows(resid, cout, 0, r16.p, cout, c->h16_mode, rows_out, cout, cout, s); d.resid = r16.p; }
            }
            IgemmArgs g = conv3_igemm(d);
            g.w16 = w16.p; g.ldw16 = ld64; g.ldw = ld64;
            g.a_bf16 = c->h16_mode; g.out_f32 = io16 ? 0 : 1; g.resid_bf16 = io16 && resid ? 1 : 0;
            // test aid: E2V_SPLITK_FORCE = S runs the launch as split-K with S runs where it is eligible (the graph asks for it by itself
            // in the small-batch family, model.cpp Runner::sk_setup)
            static const int* const sk_force = knob("E2V_SPLITK_FORCE", 0);
            Act skws;
            if (*sk_force >= 2 && !g.upsample) skws = splitk_attach(c->pool, g, *sk_force);
            if (c1 == 0 && c0p == c0 && bgemm_up2x_applies(g)) {   // exact 2x resize: the sub-pixel form the graph runner takes
                const size_t n = 4 * (size_t)cout * conv_up2x_packed_ld(cin);
                Act u32(c->pool, (int64_t)((n + 1023) / 1024), 1024), u16(c->pool, (int64_t)((n + 2047) / 2048), 1024);
                pack_conv_up2x(w_oihw, u32.p, cout, cin, s);
                to_h16(u32.p, u16.p, n, c->h16_mode, s);
                bgemm_up2x_launch(g, u16.p, s);
            } else {
                igemm(g, s);
            }
            if (io16) cvt_rows(o16.p, cout, c->h16_mode, out, cout, 0, rows_out, cout, cout, s);      // exact
        } else if (const int wm = c->conv_wino_tile(cin, cout, stride, pad_lo, Hi, Wi, Ho, Wo)) {      // the graph runner's policy
            Act u(c->pool, (int64_t)(wm + 2) * (wm + 2) * cout, cin);
            wino_pack_weights(w_oihw, u.p, cout, cin, wm, s);
            Act u3;
            if (c->x3_compute) {
                const size_t n = (size_t)(wm + 2) * (wm + 2) * cout * cin;
                u3 = Act(c->pool, (int64_t)((3 * n + 1) / 2 + 1023) / 1024, 1024);
                split_bf16x3(u.p, u3.p, n, n, s);
            }
            conv3_wino(c, d, wm, u.p, u3.p, nullptr, 0, s);
        } else {
            const int ld32 = conv3x3_packed_ld(cin, 32);
            Act wp(c->pool, cout, ld32);
            pack_conv3x3(w_oihw, wp.p, cout, cin, 32, s);
            IgemmArgs g = conv3_igemm(d);
            g.w = wp.p; g.ldw = ld32;
            igemm(g, s);
        }
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_conv3x3_gn(e2v_ctx* c, const float* x0, int c0, const float* x1, int c1, int n_img, int Hs, int Ws, int Hi, int Wi,
                             int Ho, int Wo, int stride, int pad_lo, int gn_P, int groups, float eps, const float* gamma,
                             const float* beta, const float* w_oihw, const float* bias, int cout, const float* rowbias,
                             int rows_per_sample, const float* resid, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    // the argument and shape checks make no HIP call, so they come before guarded(): a host-only context answers them too
    const int cin = c0 + c1;
    const int64_t rows = (int64_t)n_img * Hs * Ws;
    if (!(x0 && gamma && beta && w_oihw && out && c0 > 0 && c0 % 4 == 0 && c1 >= 0 && c1 % 4 == 0 && (c1 == 0 || x1) && cout > 0 && n_img > 0 &&
          Hs > 0 && Ws > 0 && groups > 0 && cin % groups == 0 && gn_P > 0 && rows % gn_P == 0)) {
        c->err = "bad conv3x3_gn arguments";
        return E2V_EINVAL;
    }
    const int wm = c->conv_wino_tile(cin, cout, stride, pad_lo, Hi, Wi, Ho, Wo);      // the graph runner's policy
    if (wm == 0) {
        c->err = "conv: fused GroupNorm needs the Winograd path";
        return E2V_ESHAPE;
    }
    return guarded(c, [&] {
        hipStream_t s = S(c, stream);
        OpRecord rec;
        const int samples = (int)(rows / gn_P);
        Act part(c->pool, (int64_t)samples * groupnorm_chunks(gn_P), cin * 2);
        Act sc(c->pool, samples, cin * 2);
        GroupNormArgs a;                     // statistics only: (scale, shift) per (slab, channel) for the conv's input transform
        a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.ld0 = c0; a.ld1 = c1; a.gamma = gamma; a.beta = beta;
        a.samples = samples; a.P = gn_P; a.groups = groups; a.eps = eps;
        a.ws_part = part.p; a.ws_scale = sc.p;
        groupnorm_stats(a, s);
        Conv3 d;
        d.x0 = x0; d.c0 = c0; d.x1 = x1; d.c1 = c1; d.nimg = n_img; d.Hs = Hs; d.Ws = Ws;
        d.Hi = Hi; d.Wi = Wi; d.Ho = Ho; d.Wo = Wo; d.stride = stride; d.pad = pad_lo;
        d.cout = cout; d.out = out; d.bias = bias;
        d.rowbias = rowbias; d.rb_ld = cout; d.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1; d.resid = resid;
        Act u(c->pool, (int64_t)(wm + 2) * (wm + 2) * cout, cin);
        wino_pack_weights(w_oihw, u.p, cout, cin, wm, s);
        Act u3;
        if (c->x3_compute) {
            const size_t n = (size_t)(wm + 2) * (wm + 2) * cout * cin;
            u3 = Act(c->pool, (int64_t)((3 * n + 1) / 2 + 1023) / 1024, 1024);
            split_bf16x3(u.p, u3.p, n, n, s);
        }
        conv3_wino(c, d, wm, u.p, u3.p, sc.p, gn_P, s);
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_linear(e2v_ctx* c, const float* x, int ldx, int64_t M, int K, const float* w, const float* bias, int N,
                         const float* resid, int geglu, float* out, e2v_stream stream) {
    return e2v_op_linear_cat(c, x, K, ldx, nullptr, 0, 0, M, w, bias, N, resid, geglu, out, stream);
}

e2v_status e2v_op_linear_cat(e2v_ctx* c, const float* x0, int c0, int ld0, const float* x1, int c1, int ld1, int64_t M, const float* w,
                             const float* bias, int N, const float* resid, int geglu, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    op_record_reset();
    // the argument checks make no HIP call, so they come before guarded(): a host-only context answers them too
    // one source: fp32 arithmetic reads 16-byte row pieces of the caller's tensor; the bf16-activation mode re-lays its operands out (K padded to 8)
    if (!(x0 && w && out && c0 > 0 && c1 >= 0 && (c1 == 0 || x1) && M >= 0 && N > 0 && (c->bf16_compute || (c0 % 4 == 0 && ld0 % 4 == 0)))) {
        c->err = "bad linear arguments";
        return E2V_EINVAL;
    }
    // two sources: the granularity Runner::linear asks for (the K loop changes source on a whole 16-byte piece)
    const int gran = c->bf16_compute ? 8 : 4;
    if (c1 > 0 && (c0 % gran || c1 % gran || (!c->bf16_compute && ld1 % 4) || ld0 < c0 || ld1 < c1)) {
        c->err = "linear: K must be a multiple of 4 (bf16: 8)";
        return E2V_ESHAPE;
    }
    return guarded(c, [&] {
        hipStream_t s = S(c, stream);
        OpRecord rec;
        const int K = c0 + c1;
        IgemmArgs g;
        g.a0 = x0; g.c0 = c0; g.lda0 = ld0; g.a1 = c1 > 0 ? x1 : nullptr; g.c1 = c1; g.lda1 = c1 > 0 ? ld1 : 0;
        g.ldw = K; g.out = out; g.M = (int)M; g.taps = 1; g.resid = resid;
        Act wp, bp;
        if (geglu) {
            E2V_REQUIRE(N % 32 == 0 && bias, E2V_EINVAL, "GEGLU width must be a multiple of 32 and have a bias");
            wp = Act(c->pool, 2 * N, K);
            bp = Act(c->pool, 1, 2 * N);
            geglu_interleave(w, bias, N, K, wp.p, bp.p, s);
            g.w = wp.p; g.bias = bp.p; g.N = 2 * N; g.ldc = N; g.geglu = 1;
        } else {
            g.w = w; g.bias = bias; g.N = N; g.ldc = N; g.ldr = N;
        }
        Act w16, a16, b16, o16, r16;
        const bool io16 = op_io16(c);      // the graph's launch: 16-bit output tensor, 16-bit residual
        if (c->bf16_compute) {       // bf16-activation mode: A and W rounded to bf16 once (K zero-padded to 8), fp32 result
            const int K8 = (K + 7) / 8 * 8, c0p = c1 > 0 ? c0 : K8;
            a16 = Act(c->pool, M, c0p, true);
            cvt_rows(x0, ld0, 0, a16.p, c0p, c->h16_mode, M, c0, c0p, s);
            if (c1 > 0) { b16 = Act(c->pool, M, c1, true); cvt_rows(x1, ld1, 0, b16.p, c1, c->h16_mode, M, c1, c1, s); }
            w16 = Act(c->pool, g.N, K8, true);
            cvt_rows(g.w, K, 0, w16.p, K8, c->h16_mode, g.N, K, K8, s);
            g.a0 = a16.p; g.c0 = c0p; g.lda0 = c0p; g.a1 = b16.p; g.lda1 = c1;
            g.a_bf16 = c->h16_mode; g.out_f32 = 1; g.w16 = w16.p; g.ldw16 = K8;
            if (io16) {
                o16 = Act(c->pool, M, N, true);
                g.out = o16.p; g.out_f32 = 0;
                if (resid) { r16 = Act(c->pool, M, N, true); cvt_rows(resid, N, 0, r16.p, N, c->h16_mode, M, N, N, s); g.resid = r16.p; g.resid_bf16 = 1; }
            }
        }
        static const int* const sk_force = knob("E2V_SPLITK_FORCE", 0);      // test aid, as in e2v_op_conv3x3
        Act skws;
        if (c->bf16_compute && *sk_force >= 2) skws = splitk_attach(c->pool, g, *sk_force);
        Act w3;
        if (c->x3_compute) {
            const size_t n = (size_t)g.N * K;
            w3 = Act(c->pool, (int64_t)((3 * n + 1) / 2 + 1023) / 1024, 1024);
            split_bf16x3(g.w, w3.p, n, n, s);
            g.x3 = 1; g.w3 = w3.p; g.w3_plane = (long long)n;
        }
        igemm(g, s);
        if (io16) cvt_rows(o16.p, N, c->h16_mode, out, N, 0, M, N, N, s);      // exact
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_groupnorm(e2v_ctx* c, const float* x0, int c0, const float* x1, int c1, int samples, int P, int groups,
                            float eps, const float* gamma, const float* beta, int act, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        const int C = c0 + c1;
        E2V_REQUIRE(x0 && gamma && beta && out && c0 % 4 == 0 && c1 % 4 == 0 && C % groups == 0, E2V_EINVAL, "bad groupnorm arguments");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        Act part(c->pool, (int64_t)samples * groupnorm_chunks(P), C * 2);
        Act sc(c->pool, samples, C * 2);
        GroupNormArgs a;
        a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.ld0 = c0; a.ld1 = c1; a.gamma = gamma; a.beta = beta;
        a.out = out; a.ldo = C; a.samples = samples; a.P = P; a.groups = groups; a.eps = eps; a.silu = act;
        a.ws_part = part.p; a.ws_scale = sc.p;
        if (c->bf16_compute) {       // bf16-activation mode: bf16 rows in and out (fp32 statistics), converted at this boundary
            const int64_t rows = (int64_t)samples * P;
            Act b0(c->pool, rows, c0, true), b1, bo(c->pool, rows, C, true);
            cvt_rows(x0, c0, 0, b0.p, c0, c->h16_mode, rows, c0, c0, s);
            if (c1 > 0) { b1 = Act(c->pool, rows, c1, true); cvt_rows(x1, c1, 0, b1.p, c1, c->h16_mode, rows, c1, c1, s); }
            a.bf16 = c->h16_mode; a.x0 = b0.p; a.x1 = c1 > 0 ? b1.p : nullptr; a.out = bo.p;
            static const int* const fused = knob("E2V_GN_FUSED_SMALL", 1);      // 2 (test aid): the one-kernel form of the small-batch family here too
            a.fused_small = *fused == 2 ? 1 : 0;
            static const int* const coop = E2V_AB_KNOB("E2V_GN_COOP", 0);        // `make ab` builds: 2 = the cooperative one-launch form here too
            a.small_chunks = *coop == 2 ? 1 : 0;
            groupnorm(a, s);
            cvt_rows(bo.p, C, c->h16_mode, out, C, 0, rows, C, C, s);
        } else {
            groupnorm(a, s);
        }
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_layernorm(e2v_ctx* c, const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps,
                            float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(x && gamma && beta && out && C % 4 == 0 && C <= 1280, E2V_EINVAL, "bad layernorm arguments");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        if (c->bf16_compute) {
            Act bi(c->pool, rows, C, true), bo(c->pool, rows, C, true);
            cvt_rows(x, C, 0, bi.p, C, c->h16_mode, rows, C, C, s);
            layernorm(bi.p, C, gamma, beta, bo.p, C, (int)rows, C, eps, s, c->h16_mode);
            cvt_rows(bo.p, C, c->h16_mode, out, C, 0, rows, C, C, s);
        } else {
            layernorm(x, C, gamma, beta, out, C, (int)rows, C, eps, s);
        }
        E2V_HIP(hipGetLastError());
    });
}

// Test aid: the canonical row-block sums a GroupNorm takes instead of its statistics pass (norm.hip rowblock_sums; what the staged
// epilogue of bgemm_t256_kernel leaves with a conv's output): x is rounded to bf16 first, out[rows / 64][C][2] = (sum, sum of squares).
e2v_status e2v_op_rowblock_sums(e2v_ctx* c, const float* x, int64_t rows, int C, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(x && out && rows > 0 && rows % 64 == 0 && C > 0 && C % 8 == 0, E2V_EINVAL, "rowblock_sums: rows must be a multiple of 64, C of 8");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        Act b(c->pool, rows, C, true);
        cvt_rows(x, C, 0, b.p, C, H16_BF16, rows, C, C, s);
        rowblock_sums(b.p, C, C, rows, rbsum_rows_per_pass(C), out, s);
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_attention(e2v_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, float* o, int ldo,
                            int n, int F, int heads, int D, int Nq, int Nk, int mode, float scale, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(q && k && v && o, E2V_EINVAL, "null argument");
        E2V_REQUIRE(D == 8 || D == 16 || D == 32 || D == 40 || D == 64 || D == 80 || D == 160, E2V_EINVAL,
                    "head dim must be one of 8, 16, 32, 40, 64, 80, 160");
        E2V_REQUIRE(ldq % 4 == 0 && ldkv % 4 == 0 && ldo % 4 == 0 && Nq > 0 && Nk > 0, E2V_EINVAL, "bad strides / sizes");
        E2V_REQUIRE(mode == 1 || Nq == Nk, E2V_ESHAPE, "self-attention needs Nq == Nk");
        AttnArgs a;
        a.q = q; a.ldq = ldq; a.k = k; a.v = v; a.ldkv = ldkv; a.o = o; a.ldo = ldo; a.n = n; a.F = F; a.heads = heads; a.D = D;
        a.Nq = Nq; a.Nk = Nk; a.mode = mode; a.scale = scale; a.x3 = c->x3_compute ? 1 : 0;
        hipStream_t s = S(c, stream);
        OpRecord rec;
        if (c->bf16_compute) {       // bf16-activation mode: Q, K, V rounded to bf16 rows once; O comes back as bf16
            const int C = heads * D;
            const int64_t qrows = (int64_t)n * F * Nq, krows = mode == 0 ? (int64_t)n * F * Nk : (int64_t)n * Nk;
            Act bq(c->pool, qrows, C, true), bk(c->pool, krows, C, true), bv(c->pool, krows, C, true), bo(c->pool, qrows, C, true);
            cvt_rows(q, ldq, 0, bq.p, C, c->h16_mode, qrows, C, C, s);
            cvt_rows(k, ldkv, 0, bk.p, C, c->h16_mode, krows, C, C, s);
            cvt_rows(v, ldkv, 0, bv.p, C, c->h16_mode, krows, C, C, s);
            a.q = bq.p; a.ldq = C; a.k = bk.p; a.v = bv.p; a.ldkv = C; a.o = bo.p; a.ldo = C; a.io_bf16 = c->h16_mode;
            flash_attention(a, s);
            cvt_rows(bo.p, C, c->h16_mode, o, ldo, 0, qrows, C, C, s);
        } else {
            flash_attention(a, s);
        }
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_temporal_attention(e2v_ctx* c, const float* qkv, float* out, int n, int F, int HW, int heads, int D,
                                     float scale, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(qkv && out && D % 4 == 0, E2V_EINVAL, "bad temporal attention arguments");
        const int C = heads * D;
        hipStream_t s = S(c, stream);
        OpRecord rec;
        if (c->bf16_compute) {
            const int64_t rows = (int64_t)n * F * HW;
            Act bi(c->pool, rows, 3 * C, true), bo(c->pool, rows, C, true);
            cvt_rows(qkv, 3 * C, 0, bi.p, 3 * C, c->h16_mode, rows, 3 * C, 3 * C, s);
            temporal_attention(bi.p, 3 * C, bo.p, C, n, F, HW, heads, D, scale, s, c->h16_mode);
            cvt_rows(bo.p, C, c->h16_mode, out, C, 0, rows, C, C, s);
        } else {
            temporal_attention(qkv, 3 * C, out, C, n, F, HW, heads, D, scale, s);
        }
        E2V_HIP(hipGetLastError());
    });
}

// the graph's own member (Runner::vae_attention_core through e2v_ctx::vae_attention_core): conversions at the boundary happen there
e2v_status e2v_op_vae_attention_core(e2v_ctx* c, const float* qkv, float* out, int nimg, int HW, int C, float* scores, float* probs,
                                     e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(qkv && out && nimg > 0 && nimg <= 65535 && HW > 0 && C > 0, E2V_EINVAL, "bad VAE attention arguments");
        E2V_REQUIRE(C % (c->bf16_compute ? 8 : 4) == 0, E2V_EINVAL, "VAE attention needs C to be a multiple of 4 (16-bit modes: 8)");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        c->vae_attention_core(qkv, nimg, HW, C, out, scores, probs, s);
    });
}

e2v_status e2v_op_softmax_rows(e2v_ctx* c, float* x, int ld, int rows, int cols, void* out16, int out_mode, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(x && rows > 0 && cols > 0 && ld >= cols, E2V_EINVAL, "bad softmax arguments");
        E2V_REQUIRE(out_mode == 0 ? out16 == nullptr : (out16 != nullptr && (out_mode == H16_BF16 || out_mode == H16_FP16)), E2V_EINVAL,
                    "softmax: out_mode 0 takes no 16-bit copy, 1 (bf16) and 2 (fp16) need one");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        softmax_rows(x, ld, rows, cols, s, out16, out_mode ? out_mode : H16_BF16);
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_transpose2d(e2v_ctx* c, const void* in, int ld_in, void* out, int ld_out, int rows, int cols, int batch,
                              int64_t sb_in, int64_t sb_out, int two_byte, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(in && out && rows > 0 && cols > 0 && ld_in >= cols && ld_out >= rows, E2V_EINVAL, "bad transpose arguments");
        E2V_REQUIRE(batch > 0 && batch <= 65535 && (rows + 31) / 32 <= 65535 && (batch == 1 || (sb_in >= 0 && sb_out >= 0)), E2V_EINVAL,
                    "transpose: 1 <= batch <= 65535, at most 65535 row tiles, batch strides not negative");
        hipStream_t s = S(c, stream);
        OpRecord rec;
        transpose2d(static_cast<const float*>(in), ld_in, static_cast<float*>(out), ld_out, rows, cols, batch, sb_in, sb_out, s, two_byte ? 1 : 0);
        E2V_HIP(hipGetLastError());
    });
}

// fp32 in every compute mode, as e2v_text_encode runs it
e2v_status e2v_op_causal_attention(e2v_ctx* c, const float* qkv, int ldqkv, float* out, int ldo, int B, int T, int heads, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(qkv && out && (reinterpret_cast<uintptr_t>(qkv) & 15) == 0, E2V_EINVAL, "null or misaligned argument (qkv: 16 bytes)");
        E2V_REQUIRE(B > 0 && heads > 0 && T >= 1 && T <= kTextAttnMaxT, E2V_ESHAPE, "causal attention: B, heads >= 1 and 1 <= T <= " + std::to_string(kTextAttnMaxT));
        E2V_REQUIRE(ldqkv % 4 == 0 && ldqkv >= 3 * 64 * heads && ldo >= 64 * heads, E2V_EINVAL, "bad strides: ldqkv >= 3 * 64 * heads (a multiple of 4), ldo >= 64 * heads");
        text_causal_attention(qkv, ldqkv, out, ldo, B, T, heads, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

// the EEGNet embedding kernel of e2v_seq2seq_latents from torch-layout device tensors (folded on the host, as finalize does)
e2v_status e2v_op_eegnet_embed(e2v_ctx* c, const float* eeg, int64_t clip_stride, int64_t window_stride, int64_t channel_stride,
                               const float* mean, const float* scale, int B, int W, int C, int T, int F1, int D, int F2, const float* w1,
                               const float* bn1, const float* w2, const float* bn2, const float* w3, const float* w4, const float* bn3,
                               float bn_eps, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(eeg && out && w1 && bn1 && w2 && bn2 && w3 && w4 && bn3, E2V_EINVAL, "null argument");
        E2V_REQUIRE((mean == nullptr) == (scale == nullptr), E2V_EINVAL, "the scaler is a mean AND a scale, or neither");
        E2V_REQUIRE(clip_stride >= 0 && window_stride >= 0 && channel_stride >= 0 && bn_eps > 0.f, E2V_EINVAL, "negative stride or eps");
        E2V_REQUIRE(B >= 1 && W >= 1 && C >= 1 && C <= 4096 && T >= 32 && T <= 65536 && F1 >= 1 && F1 <= 1024 && D >= 1 && D <= 1024 && F2 >= 1 && F2 <= 1024,
                    E2V_ESHAPE, "EEGNet embedding: positive, bounded sizes and at least 32 samples a window");
        hipStream_t s = S(c, stream);
        const int FD = F1 * D;
        auto host = [&](const float* d, size_t n) {
            std::vector<float> h(n);
            E2V_HIP(hipMemcpyAsync(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost, s));
            return h;
        };
        const std::vector<float> h1 = host(w1, (size_t)F1 * 64), hb1 = host(bn1, 4 * (size_t)F1), h2 = host(w2, (size_t)FD * C), hb2 = host(bn2, 4 * (size_t)FD),
                                 h3 = host(w3, (size_t)FD * 16), h4 = host(w4, (size_t)F2 * FD), hb3 = host(bn3, 4 * (size_t)F2);
        E2V_HIP(hipStreamSynchronize(s));
        const std::vector<float> pk = eegnet_pack(EegnetHostW{h1.data(), hb1.data(), h2.data(), hb2.data(), h3.data(), h4.data(), hb3.data()}, C, F1, D, F2, bn_eps);
        Act dp(c->pool, (int64_t)pk.size(), 1);
        E2V_HIP(hipMemcpyAsync(dp.p, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice, s));
        EegnetArgs a;
        a.eeg = eeg; a.clip_stride = clip_stride; a.window_stride = window_stride; a.channel_stride = channel_stride; a.mean = mean; a.scale = scale;
        a.pack = dp.p; a.out = out; a.B = B; a.W = W; a.C = C; a.T = T; a.F1 = F1; a.D = D; a.F2 = F2;
        eegnet_embed(a, s);
        E2V_HIP(hipStreamSynchronize(s));                        // (pk is pageable host memory: the copy has to have left it)
        E2V_HIP(hipGetLastError());
    });
}

// the ShallowNet kernel of e2v_glmnet_raw from torch-layout device tensors (folded on the host, as finalize does)
e2v_status e2v_op_shallownet(e2v_ctx* c, const float* eeg, int64_t clip_stride, int64_t channel_stride, const float* mean, const float* scale,
                             int B, int C, int T, int F, int K, int P, int S_, const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* bn, float bn_eps, float* out, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(B >= 1 && C >= 1 && C <= 4096 && T >= 1 && T <= 65536 && F >= 1 && F <= 1024 && K >= 1 && K <= 1024 && P >= 1 && P <= 65536 && S_ >= 1 &&
                        shallownet_columns(T, K, P, S_) >= 1,
                    E2V_ESHAPE, "ShallowNet: positive, bounded sizes and at least taps + pool - 1 samples");
        E2V_REQUIRE(eeg && out && w1 && b1 && w2 && b2 && bn, E2V_EINVAL, "null argument");
        E2V_REQUIRE((mean == nullptr) == (scale == nullptr), E2V_EINVAL, "the scaler is a mean AND a scale, or neither");
        E2V_REQUIRE(clip_stride >= 0 && channel_stride >= 0 && bn_eps > 0.f, E2V_EINVAL, "negative stride or eps");
        hipStream_t s = S(c, stream);
        auto host = [&](const float* d, size_t n) {
            std::vector<float> h(n);
            E2V_HIP(hipMemcpyAsync(h.data(), d, n * sizeof(float), hipMemcpyDeviceToHost, s));
            return h;
        };
        const std::vector<float> h1 = host(w1, (size_t)F * K), hb1 = host(b1, F), h2 = host(w2, (size_t)F * F * C), hb2 = host(b2, F), hbn = host(bn, 4 * (size_t)F);
        E2V_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < F; ++i) E2V_REQUIRE(hbn[3 * F + i] + bn_eps > 0.f, E2V_EINVAL, "running_var + eps must be positive");
        const std::vector<float> pk = shallownet_fold(ShallowHostW{h1.data(), hb1.data(), h2.data(), hb2.data(), hbn.data()}, C, F, K, bn_eps);
        Act dp(c->pool, (int64_t)pk.size(), 1);
        E2V_HIP(hipMemcpyAsync(dp.p, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice, s));
        ShallowArgs a;
        a.eeg = eeg; a.clip_stride = clip_stride; a.channel_stride = channel_stride; a.mean = mean; a.scale = scale;
        a.w = dp.p; a.c = dp.p + pk.size() - shallownet_fold_floats(0, F, 0);
        a.out = out; a.ldo = F * shallownet_columns(T, K, P, S_);
        a.B = B; a.C = C; a.T = T; a.F = F; a.K = K; a.P = P; a.S = S_;
        shallownet(a, s);
        E2V_HIP(hipStreamSynchronize(s));                        // (pk is pageable host memory: the copy has to have left it)
        E2V_HIP(hipGetLastError());
    });
}

// the attention kernel of e2v_seq2seq_latents on caller tensors
e2v_status e2v_op_seq_attention(e2v_ctx* c, const float* q, int ldq, const float* k, const float* v, int ldkv, float* out, int ldo, int B,
                                int heads, int D, int Nq, int Nk, int q_pos0, int causal, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        E2V_REQUIRE(q && k && v && out && ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0, E2V_EINVAL,
                    "null or misaligned argument (q, k: 16 bytes)");
        E2V_REQUIRE(B >= 1 && heads >= 1 && Nq >= 1 && Nq <= (1 << 16) && Nk >= 1 && Nk <= kSeqAttnMaxKeys && q_pos0 >= 0 && D >= 4 && D % 4 == 0 && D <= 128 && heads <= 4096,
                    E2V_ESHAPE, "sequence attention: B, heads, Nq >= 1, 1 <= Nk <= " + std::to_string(kSeqAttnMaxKeys) + ", D a multiple of 4 up to 128");
        E2V_REQUIRE(ldq % 4 == 0 && ldkv % 4 == 0 && ldq >= heads * D && ldkv >= heads * D && ldo >= heads * D, E2V_EINVAL,
                    "bad strides: ldq, ldkv (multiples of 4) and ldo are at least heads * D");
        SeqAttnArgs a;
        a.q = q; a.sq = (long long)Nq * ldq; a.ldq = ldq; a.k = k; a.v = v; a.skv = (long long)Nk * ldkv; a.ldkv = ldkv;
        a.o = out; a.so = (long long)Nq * ldo; a.ldo = ldo;
        a.B = B; a.heads = heads; a.D = D; a.Nq = Nq; a.Nk = Nk; a.q_pos0 = q_pos0; a.causal = causal ? 1 : 0; a.scale = 1.0f / std::sqrt((float)D);
        seq_attention(a, S(c, stream));
        E2V_HIP(hipGetLastError());
    });
}

e2v_status e2v_op_to_channels_last(e2v_ctx* c, const float* in, float* out, int n, int C, int Cpad, int FHW, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] { ncfhw_to_cl(in, out, n, C, Cpad, FHW, 1.0f, S(c, stream)); E2V_HIP(hipGetLastError()); });
}

e2v_status e2v_op_from_channels_last(e2v_ctx* c, const float* in, int ld, float* out, int n, int C, int FHW, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] { cl_to_ncfhw(in, ld, out, n, C, FHW, 1.f, 0.f, 0, 0.f, 0.f, S(c, stream)); E2V_HIP(hipGetLastError()); });
}

// Test aid (E2V_POOL_GUARD, runtime.h): drain the stream, compare the guard zones of the blocks that are still live -- pool blocks,
// dev_alloc blocks, the GroupNorm workspaces -- and hand out the totals since the previous report.
e2v_status e2v_op_pool_guard_report(e2v_ctx* c, int64_t* blocks_checked, int64_t* violations, char* buf, int64_t cap) {
    if (!c) return E2V_EINVAL;
    if (!blocks_checked || !violations || cap < 0 || (cap > 0 && !buf)) { c->err = "null argument"; return E2V_EINVAL; }
    return guarded(c, [&] {
        E2V_REQUIRE(!dry_run(), E2V_ESTATE, "no guarded blocks in a dry run");
        const hipStream_t s = c->last_stream;
        c->pool.check_live(s);
        for (const auto& part : c->owned_part)
            for (const DevBlock& b : part)
                if (b.guard) c->guard_tally.check(b, "dev_alloc", s);
        for (const GrowBuf* ws : {&c->gn_part, &c->gn_scale})
            if (ws->blk.guard) c->guard_tally.check(ws->blk, "GroupNorm workspace", s);
        E2V_HIP(hipStreamSynchronize(s));
        E2V_HIP(hipGetLastError());
        c->guard_tally.collect();
        std::string text;
        c->guard_tally.take(*blocks_checked, *violations, text);
        if (cap > 0) {
            const size_t n = std::min(text.size(), (size_t)cap - 1);
            std::memcpy(buf, text.data(), n);
            buf[n] = 0;
        }
    });
}

int64_t e2v_op_pool_gets(const e2v_ctx* c) { return c ? c->pool.gets() : 0; }

// Test aid: the detector's own test.  Takes one block of payload_bytes through the pool, sets the word `offset` bytes into its trailing
// guard zone to zero from the host side (hipMemsetAsync: an address inside the block the pool allocated) and releases the block.
e2v_status e2v_op_pool_guard_selftest(e2v_ctx* c, int64_t payload_bytes, int64_t offset, e2v_stream stream) {
    if (!c) return E2V_EINVAL;
    return guarded(c, [&] {
        const int kib = pool_guard_kib();
        E2V_REQUIRE(kib > 0, E2V_ESTATE, "E2V_POOL_GUARD is off");
        E2V_REQUIRE(payload_bytes > 0 && payload_bytes % 4 == 0 && offset >= 0 && offset % 4 == 0 && offset + 4 <= (int64_t)kib * 1024, E2V_EINVAL,
                    "the payload is whole words and the offset a word inside the guard zone");
        hipStream_t s = S(c, stream);
        float* p = c->pool.get_bytes((size_t)payload_bytes);
        hipError_t e = hipMemsetAsync(reinterpret_cast<char*>(p) + payload_bytes + offset, 0, 4, s);
        c->pool.put(p);
        E2V_HIP(e);
    });
}

// Test aid: the dry_tag() texts of the launches the calling thread's latest kernel-level entry point made (E2V_OP_RECORD on), else "".
// No HIP call: a host-only context answers it too.
e2v_status e2v_op_last_dispatch(char* buf, int64_t cap) {
    if (cap < 0 || (cap > 0 && !buf)) return E2V_EINVAL;
    static const int* const on = knob("E2V_OP_RECORD", 0);
    if (cap == 0) return E2V_OK;
    if (!*on) { buf[0] = 0; return E2V_OK; }
    const std::string& t = op_dispatch();
    const size_t n = std::min(t.size(), (size_t)cap - 1);
    std::memcpy(buf, t.data(), n);
    buf[n] = 0;
    return E2V_OK;
}

e2v_status e2v_op_set_knob(const char* name, int value) {
    if (!name) return E2V_EINVAL;
    return set_knob(name, value) ? E2V_OK : E2V_EINVAL;
}

}  // extern "C"
