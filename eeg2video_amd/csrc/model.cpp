// Model graphs of the EEG2Video generation hot path on one HIP stream (see model.h).
#include "model.h"
#include "h16.h"
#include "../../include/eeg2video_hip_ops.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace e2v;

// =====================================================================================================
// expected state-dict keys (SURVEY App. D for the UNet, App. C.5 for the VAE) -- mirrors
// eeg2video_amd/weights.py; the test-suite checks both against the reference's own state dict.
// =====================================================================================================
namespace {

struct KeySink {
    e2v_ctx* c;
    void add(const std::string& k, std::vector<int64_t> shape) {
        WTensor t;
        t.shape = std::move(shape);
        t.numel = 1;
        for (auto d : t.shape) t.numel *= (size_t)d;
        c->keys.push_back(k);
        c->raw.emplace(k, std::move(t));
    }
    void conv(const std::string& n, int co, int ci, int k) { add(n + ".weight", {co, ci, k, k}); add(n + ".bias", {co}); }
    void lin(const std::string& n, int co, int ci, bool bias = true) {
        add(n + ".weight", {co, ci});
        if (bias) add(n + ".bias", {co});
    }
    void norm(const std::string& n, int ch) { add(n + ".weight", {ch}); add(n + ".bias", {ch}); }
    void resnet3d(const std::string& p, int cin, int cout, int temb) {      // resnet.py:141-172
        norm(p + ".norm1", cin); conv(p + ".conv1", cout, cin, 3);
        if (temb > 0) lin(p + ".time_emb_proj", cout, temb);
        norm(p + ".norm2", cout); conv(p + ".conv2", cout, cout, 3);
        if (cin != cout) conv(p + ".conv_shortcut", cout, cin, 1);
    }
    void transformer3d(const std::string& p, int ch, int cross) {            // attention.py:58-87,158-202
        norm(p + ".norm", ch); conv(p + ".proj_in", ch, ch, 1);
        const std::string b = p + ".transformer_blocks.0";
        const char* names[3] = {"attn1", "attn2", "attn_temp"};
        const int kv[3] = {ch, cross, ch};
        for (int i = 0; i < 3; ++i) {
            const std::string a = b + "." + names[i];
            lin(a + ".to_q", ch, ch, false); lin(a + ".to_k", ch, kv[i], false); lin(a + ".to_v", ch, kv[i], false);
            lin(a + ".to_out.0", ch, ch);
        }
        for (const char* n : {"norm1", "norm2", "norm3", "norm_temp"}) norm(b + "." + n, ch);
        lin(b + ".ff.net.0.proj", 8 * ch, ch); lin(b + ".ff.net.2", ch, 4 * ch);
        conv(p + ".proj_out", ch, ch, 1);
    }
    void vae_mid(const std::string& p, int ch) {
        resnet3d(p + ".resnets.0", ch, ch, 0);
        const std::string a = p + ".attentions.0";
        norm(a + ".group_norm", ch);
        for (const char* n : {"query", "key", "value", "proj_attn"}) lin(a + "." + n, ch, ch);
        resnet3d(p + ".resnets.1", ch, ch, 0);
    }
    // one encoder layer under transformers' ViT / VideoMAE names ("image.", "video.") and one CLIPEncoderLayer ("text.", "clipv."),
    // each in its checkpoint's own order
    void hf_vit_layer(const std::string& l, int C, int I) {
        for (const char* n : {"query", "key", "value"}) lin(l + ".attention.attention." + n, C, C);
        lin(l + ".attention.output.dense", C, C);
        lin(l + ".intermediate.dense", I, C); lin(l + ".output.dense", C, I);
        norm(l + ".layernorm_before", C); norm(l + ".layernorm_after", C);
    }
    void clip_layer(const std::string& l, int C, int I) {
        for (const char* n : {"q_proj", "k_proj", "v_proj", "out_proj"}) lin(l + ".self_attn." + n, C, C);
        norm(l + ".layer_norm1", C); norm(l + ".layer_norm2", C);
        lin(l + ".mlp.fc1", I, C); lin(l + ".mlp.fc2", C, I);
    }
};

std::string idx(const std::string& a, int i, const std::string& b, int j) {
    return a + "." + std::to_string(i) + "." + b + "." + std::to_string(j);
}

}  // namespace

bool e2v_ctx::has_part(Part p) const {
    switch (p) {
        case UNET: case VAE: return true;
        case SEM: return cfg.sem_in_features > 0 && cfg.sem_hidden > 0;
        case TEXT: return cfg.text_layers > 0;
        case IMAGE: return cfg.vit_layers > 0;
        case VIDEO: return cfg.vmae_layers > 0;
        case CLIPV: return vcfg.clipv_layers > 0;
        case S2S: return scfg.s2s_d_model > 0;
        case GLM: return gcfg.glm_raw_out > 0 || gcfg.glm_mlp_out > 0;
        case N_PARTS: break;
    }
    return false;
}

void e2v_ctx::expected_keys() {
    KeySink s{this};
    const int* boc = cfg.block_out_channels;
    const int temb = boc[0] * 4, cross = cfg.cross_attention_dim, L = cfg.layers_per_block;
    s.conv("conv_in", boc[0], cfg.in_channels, 3);
    s.lin("time_embedding.linear_1", temb, boc[0]);
    s.lin("time_embedding.linear_2", temb, temb);
    int out_c = boc[0];
    for (int i = 0; i < 4; ++i) {                      // unet.py:113-139; blocks 0-2 carry attention
        const int in_c = out_c;
        out_c = boc[i];
        for (int j = 0; j < L; ++j) {
            s.resnet3d(idx("down_blocks", i, "resnets", j), j == 0 ? in_c : out_c, out_c, temb);
            if (i < 3) s.transformer3d(idx("down_blocks", i, "attentions", j), out_c, cross);
        }
        if (i != 3) s.conv("down_blocks." + std::to_string(i) + ".downsamplers.0.conv", out_c, out_c, 3);
    }
    s.resnet3d("mid_block.resnets.0", boc[3], boc[3], temb);
    s.transformer3d("mid_block.attentions.0", boc[3], cross);
    s.resnet3d("mid_block.resnets.1", boc[3], boc[3], temb);
    const int rev[4] = {boc[3], boc[2], boc[1], boc[0]};
    out_c = rev[0];
    for (int i = 0; i < 4; ++i) {                      // unet.py:164-202; blocks 1-3 carry attention
        const int prev = out_c;
        out_c = rev[i];
        const int in_c = rev[std::min(i + 1, 3)];
        for (int j = 0; j < L + 1; ++j) {
            const int skip = (j == L) ? in_c : out_c;  // unet_blocks.py:431-432
            const int rin = (j == 0) ? prev : out_c;
            s.resnet3d(idx("up_blocks", i, "resnets", j), rin + skip, out_c, temb);
            if (i > 0) s.transformer3d(idx("up_blocks", i, "attentions", j), out_c, cross);
        }
        if (i != 3) s.conv("up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out_c, out_c, 3);
    }
    s.norm("conv_norm_out", boc[0]);
    s.conv("conv_out", cfg.out_channels, boc[0], 3);

    // ---- VAE ("vae." prefix) ----
    const int* vb = cfg.vae_block_out_channels;
    const int VL = cfg.vae_layers_per_block, lat = cfg.vae_latent_channels;
    s.conv("vae.encoder.conv_in", vb[0], cfg.vae_in_channels, 3);
    out_c = vb[0];
    for (int i = 0; i < 4; ++i) {
        const int in_c = out_c;
        out_c = vb[i];
        for (int j = 0; j < VL; ++j) s.resnet3d(idx("vae.encoder.down_blocks", i, "resnets", j), j == 0 ? in_c : out_c, out_c, 0);
        if (i != 3) s.conv("vae.encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv", out_c, out_c, 3);
    }
    s.vae_mid("vae.encoder.mid_block", vb[3]);
    s.norm("vae.encoder.conv_norm_out", vb[3]);
    s.conv("vae.encoder.conv_out", 2 * lat, vb[3], 3);
    const int vrev[4] = {vb[3], vb[2], vb[1], vb[0]};
    s.conv("vae.decoder.conv_in", vrev[0], lat, 3);
    s.vae_mid("vae.decoder.mid_block", vrev[0]);
    out_c = vrev[0];
    for (int i = 0; i < 4; ++i) {
        const int in_c = out_c;
        out_c = vrev[i];
        for (int j = 0; j < VL + 1; ++j) s.resnet3d(idx("vae.decoder.up_blocks", i, "resnets", j), j == 0 ? in_c : out_c, out_c, 0);
        if (i != 3) s.conv("vae.decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out_c, out_c, 3);
    }
    s.norm("vae.decoder.conv_norm_out", vb[0]);
    s.conv("vae.decoder.conv_out", cfg.vae_in_channels, vb[0], 3);
    s.conv("vae.quant_conv", 2 * lat, 2 * lat, 1);
    s.conv("vae.post_quant_conv", lat, lat, 1);

    // ---- Semantic Predictor ("semantic." prefix; nn.Sequential indices of train_semantic_predictor.py:14-28) ----
    if (has_part(SEM)) {
        const int dims[6] = {cfg.sem_in_features, cfg.sem_hidden, cfg.sem_hidden, cfg.sem_hidden, cfg.sem_hidden,
                             cfg.sem_tokens * cfg.cross_attention_dim};
        for (int i = 0; i < 5; ++i) s.lin("semantic.mlp." + std::to_string(2 * i), dims[i + 1], dims[i]);
    }

    // ---- CLIP text encoder ("text." prefix; the keys of the SD-v1-4 text_encoder checkpoint, transformers CLIPTextModel) ----
    if (has_part(TEXT)) {
        const int C = cfg.text_hidden, I = cfg.text_intermediate;
        const std::string m = "text.text_model.";
        s.add(m + "embeddings.token_embedding.weight", {cfg.text_vocab_size, C});
        s.add(m + "embeddings.position_embedding.weight", {cfg.text_max_positions, C});
        for (int i = 0; i < cfg.text_layers; ++i) s.clip_layer(m + "encoder.layers." + std::to_string(i), C, I);
        s.norm(m + "final_layer_norm", C);
    }

    // ---- ViT image classifier ("image." prefix; the keys of the google/vit-base-patch16-224 checkpoint, ViTForImageClassification) ----
    if (has_part(IMAGE)) {
        const int C = cfg.vit_hidden, I = cfg.vit_intermediate, P = cfg.vit_patch_size;
        const std::string m = "image.vit.";
        s.add(m + "embeddings.cls_token", {1, 1, C});
        s.add(m + "embeddings.position_embeddings", {1, image_tokens(), C});
        s.conv(m + "embeddings.patch_embeddings.projection", C, 3, P);
        for (int i = 0; i < cfg.vit_layers; ++i) s.hf_vit_layer(m + "encoder.layer." + std::to_string(i), C, I);
        s.norm(m + "layernorm", C);
        s.lin("image.classifier", cfg.vit_num_labels, C);
    }

    // ---- VideoMAE video classifier ("video." prefix; the names of transformers' VideoMAEForVideoClassification state dict, and the
    // fixed position table -- a buffer transformers builds at construction -- as a key of our own) ----
    if (has_part(VIDEO)) {
        const int C = cfg.vmae_hidden, I = cfg.vmae_intermediate, P = cfg.vmae_patch_size;
        const std::string m = "video.videomae.";
        s.add(m + "embeddings.position_embeddings", {video_tokens(), C});
        s.conv(m + "embeddings.patch_embeddings.projection", C, 3 * cfg.vmae_tubelet_size, P);      // Conv3d [C][3][ts][P][P], axes 1 and 2 merged
        for (int i = 0; i < cfg.vmae_layers; ++i) s.hf_vit_layer(m + "encoder.layer." + std::to_string(i), C, I);
        s.norm("video.fc_norm", C);
        s.lin("video.classifier", cfg.vmae_num_labels, C);
    }

    // ---- CLIP vision tower ("clipv." prefix; the keys of a CLIPVisionModelWithProjection checkpoint -- "pre_layrnorm" is the
    // checkpoint's own spelling; the position_ids buffer of older checkpoints is not a weight) ----
    if (has_part(CLIPV)) {
        const int C = vcfg.clipv_hidden, I = vcfg.clipv_intermediate, P = vcfg.clipv_patch_size;
        const std::string m = "clipv.vision_model.";
        s.add(m + "embeddings.class_embedding", {C});
        s.add(m + "embeddings.patch_embedding.weight", {C, 3, P, P});
        s.add(m + "embeddings.position_embedding.weight", {clipv_tokens(), C});
        s.norm(m + "pre_layrnorm", C);
        for (int i = 0; i < vcfg.clipv_layers; ++i) s.clip_layer(m + "encoder.layers." + std::to_string(i), C, I);
        s.norm(m + "post_layernorm", C);
        s.lin("clipv.visual_projection", vcfg.clipv_projection_dim, C, false);
    }

    // ---- Seq2Seq latent model ("s2s." prefix; the names of the reference's myTransformer state dict in its order, without what
    // inference never reads -- embedding.weight, img_embedding.*, every num_batches_tracked -- and with the position table as the
    // [windows][d_model] rows that are read, not the [1][5000][d_model] buffer) ----
    if (has_part(S2S)) {
        const int C = scfg.s2s_d_model, I = scfg.s2s_ffn, FD = scfg.s2s_f1 * scfg.s2s_d;
        const std::string e = "s2s.eeg_embedding.";
        auto bn = [&](const std::string& n, int ch) {
            for (const char* t : {".weight", ".bias", ".running_mean", ".running_var"}) s.add(n + t, {ch});
        };
        auto mha = [&](const std::string& n) {
            s.add(n + ".in_proj_weight", {3 * C, C}); s.add(n + ".in_proj_bias", {3 * C});
            s.lin(n + ".out_proj", C, C);
        };
        s.add(e + "block_1.1.weight", {scfg.s2s_f1, 1, 1, 64}); bn(e + "block_1.2", scfg.s2s_f1);
        s.add(e + "block_2.0.weight", {FD, 1, scfg.s2s_electrodes, 1}); bn(e + "block_2.1", FD);
        s.add(e + "block_3.1.weight", {FD, 1, 1, 16});
        s.add(e + "block_3.2.weight", {scfg.s2s_f2, FD, 1, 1}); bn(e + "block_3.3", scfg.s2s_f2);
        s.lin(e + "embedding", C, s2s_features());
        for (int i = 0; i < scfg.s2s_encoder_layers; ++i) {
            const std::string l = "s2s.transformer_encoder.layers." + std::to_string(i);
            mha(l + ".self_attn");
            s.lin(l + ".linear1", I, C); s.lin(l + ".linear2", C, I);
            s.norm(l + ".norm1", C); s.norm(l + ".norm2", C);
        }
        for (int i = 0; i < scfg.s2s_decoder_layers; ++i) {
            const std::string l = "s2s.transformer_decoder.layers." + std::to_string(i);
            mha(l + ".self_attn"); mha(l + ".multihead_attn");
            s.lin(l + ".linear1", I, C); s.lin(l + ".linear2", C, I);
            s.norm(l + ".norm1", C); s.norm(l + ".norm2", C); s.norm(l + ".norm3", C);
        }
        s.add("s2s.positional_encoding.pe", {scfg.s2s_windows, C});
        s.lin("s2s.txtpredictor", scfg.s2s_txt_classes, C);
        s.lin("s2s.predictor", s2s_latent(), C);
    }

    // ---- GLMNet ("glm.raw." + the names of the reference's glfnet state dict, "glm.mlp." + glfnet_mlp's, each in its order and only
    // if the model is configured; num_batches_tracked is not a weight and not expected) ----
    if (has_part(GLM)) {
        const int F = gcfg.glm_filters, E = gcfg.glm_emb;
        if (gcfg.glm_raw_out > 0) {
            for (const auto& net : {std::make_pair(std::string("glm.raw.globalnet"), gcfg.glm_electrodes),
                                    std::make_pair(std::string("glm.raw.occipital_localnet"), gcfg.glm_occ_count)}) {
                s.add(net.first + ".net.0.weight", {F, 1, 1, gcfg.glm_taps}); s.add(net.first + ".net.0.bias", {F});
                s.add(net.first + ".net.1.weight", {F, F, net.second, 1}); s.add(net.first + ".net.1.bias", {F});
                for (const char* t : {".weight", ".bias", ".running_mean", ".running_var"}) s.add(net.first + ".net.2" + t, {F});
                s.lin(net.first + ".out", E, glm_raw_features());
            }
            s.lin("glm.raw.out", gcfg.glm_raw_out, 2 * E);
        }
        if (gcfg.glm_mlp_out > 0) {
            for (const auto& net : {std::make_pair(std::string("glm.mlp.globalnet"), gcfg.glm_electrodes),
                                    std::make_pair(std::string("glm.mlp.occipital_localnet"), gcfg.glm_occ_count)}) {
                s.lin(net.first + ".net.1", gcfg.glm_hidden1, net.second * gcfg.glm_bands);
                s.lin(net.first + ".net.3", gcfg.glm_hidden2, gcfg.glm_hidden1);
                s.lin(net.first + ".net.5", E, gcfg.glm_hidden2);
            }
            s.lin("glm.mlp.out", gcfg.glm_mlp_out, 2 * E);
        }
    }
}

// a block of a weight layout, owned by the part its caller selected (AllocPart); guarded, and its payload poisoned before the first
// write, under E2V_POOL_GUARD.  A dry run hands out an address and owns nothing.
float* e2v_ctx::dev_alloc(size_t floats) {
    E2V_REQUIRE(alloc_part >= 0, E2V_ESTATE, "dev_alloc outside a part");
    DevBlock b = dev_block(std::max<size_t>(floats, 1) * sizeof(float), (size_t)pool_guard_kib() * 1024, nullptr, true);
    float* p = b.f32();
    if (b.total) owned_part[alloc_part].push_back(std::move(b));
    return p;
}

size_t e2v_ctx::weight_bytes() const {
    size_t n = 0;
    for (const auto& kv : raw) n += kv.second.mem.total;
    for (const auto& part : owned_part)
        for (const DevBlock& b : part) n += b.total;
    return n;
}

// fp32 arithmetic only (in a 16-bit mode the transforms would dominate and rounding the transformed inputs costs accuracy), for a
// stride-1, pad-1 conv whose channel counts are multiples of 4.  conv_algo 1 / 2 / 3: direct / F(2x2) / F(4x4) wherever it applies.
int e2v_ctx::conv_wino_tile(int cin, int cout, int stride, int pad, int Hi, int Wi, int Ho, int Wo) const {
    if (bf16_compute || stride != 1 || pad != 1 || Hi != Ho || Wi != Wo || cin % 4 != 0 || cout % 4 != 0) return 0;
    if (conv_algo == 2 || conv_algo == 3) return conv_algo == 3 ? 4 : 2;
    if (conv_algo != 0) return 0;
    const int cmin = std::min(cin, cout);
    const double padded = (double)((Ho + 3) / 4 * 4) * ((Wo + 3) / 4 * 4);
    if (wino_f4 && cmin >= wino4_min_c && padded <= wino_f4_pad * Ho * Wo) return 4;
    return cmin >= wino_min_c ? 2 : 0;
}

int e2v::small_family_clips() {
    static const int* const clips = knob("E2V_SMALL_FAMILY_CLIPS", 4);
    return *clips;
}

IgemmArgs e2v::conv3_igemm(const Conv3& d) {
    IgemmArgs g;
    g.a0 = d.x0; g.c0 = d.c0; g.lda0 = d.c0; g.a1 = d.x1; g.c1 = d.c1; g.lda1 = d.c1;
    g.out = d.out; g.ldc = d.cout; g.bias = d.bias;
    g.rowbias = d.rowbias; g.rb_ld = d.rb_ld; g.rows_per_sample = d.rows_per_sample;
    g.resid = d.resid; g.ldr = d.cout;
    g.M = d.nimg * d.Ho * d.Wo; g.N = d.cout; g.taps = 9;
    g.Ho = d.Ho; g.Wo = d.Wo; g.Hi = d.Hi; g.Wi = d.Wi; g.Hs = d.Hs; g.Ws = d.Ws; g.stride = d.stride; g.pad = d.pad;
    g.upsample = d.resized(); g.ups_h = d.ups_h(); g.ups_w = d.ups_w();
    return g;
}

void e2v::conv3_wino(e2v_ctx* c, const Conv3& d, int m, const float* U, const void* U3, const float* gn_scsh, int gn_P, hipStream_t s) {
    WinoArgs a;
    a.m = m;
    a.x0 = d.x0; a.c0 = d.c0; a.ld0 = d.c0; a.x1 = d.x1; a.c1 = d.c1; a.ld1 = d.c1;
    a.nimg = d.nimg; a.Hs = d.Hs; a.Ws = d.Ws; a.Ho = d.Ho; a.Wo = d.Wo;
    a.upsample = d.resized(); a.ups_h = d.ups_h(); a.ups_w = d.ups_w();
    if (gn_P > 0) { a.gn_scsh = gn_scsh; a.gn_P = gn_P; a.gn_silu = 1; }
    a.U = U; a.U3 = U3; a.N = d.cout; a.out = d.out; a.ldc = d.cout; a.bias = d.bias;
    a.rowbias = d.rowbias; a.rb_ld = d.rb_ld; a.rows_per_sample = d.rows_per_sample; a.resid = d.resid; a.ldr = d.cout;
    const int chunk = wino_chunk_images(a, c->wino_ws_floats);
    const size_t need = wino_workspace_floats(a, chunk);
    Act ws(c->pool, (int64_t)((need + 1023) / 1024), 1024);
    wino_conv3x3(a, ws.p, chunk, s);
}

void e2v::geglu_interleave(const float* w, const float* b, int half, int in, float* dw, float* db, hipStream_t s) {
    for (int q = 0; q < half / 32; ++q) {
        copy_rows(w + (size_t)(q * 32) * in, in, dw + (size_t)(q * 64) * in, in, 32, in, s);
        copy_rows(w + (size_t)(half + q * 32) * in, in, dw + (size_t)(q * 64 + 32) * in, in, 32, in, s);
        copy_rows(b + q * 32, 32, db + q * 64, 32, 1, 32, s);
        copy_rows(b + half + q * 32, 32, db + q * 64 + 32, 32, 1, 32, s);
    }
}

Act e2v::splitk_attach(Pool& pool, IgemmArgs& g, int want) {
    Act ws;
    const int runs = splitk_plan(g, want);
    if (runs < 2) return ws;
    ws = Act(pool, (int64_t)runs * g.M, g.N);
    g.sk = want; g.sk_ws = ws.p;
    return ws;
}

// First use of a layout: allocate it under the owning finalize() group (freed when that part is finalized again) and derive
// it from the torch-layout weight on the calling stream -- ordered before the launch that asked for it.
void e2v_ctx::conv_form(const ConvW& w, ConvForm f, hipStream_t s) {
    AllocPart guard(this, w.part);
    bool fresh = false;
    auto need = [&](auto& dst, size_t floats) {
        if (dst) return;
        dst = dev_alloc(floats);
        fresh = true;
    };
    const size_t n16 = (size_t)w.cout * w.ldw16, n16_up2 = 4 * (size_t)w.cout * conv_up2x_packed_ld(w.cin);
    switch (f) {
        case FORM_DIRECT32: need(w.w, (size_t)w.cout * w.ldw); break;
        case FORM_BF16: need(w.w16, (n16 + 1) / 2); break;
        case FORM_F16: need(w.w16h, (n16 + 1) / 2); break;
        case FORM_BF16_UP2: need(w.w16_up2, (n16_up2 + 1) / 2); break;
        case FORM_F16_UP2: need(w.w16h_up2, (n16_up2 + 1) / 2); break;
        case FORM_WINO2:
        case FORM_WINO4: {
            const int m = f == FORM_WINO4 ? 4 : 2;
            const size_t n = (size_t)(m + 2) * (m + 2) * w.cout * w.cin;
            need(m == 4 ? w.wino4 : w.wino, n);
            if (x3_compute) need(m == 4 ? w.wino4_x3 : w.wino_x3, (3 * n + 1) / 2);
            break;
        }
    }
    if (fresh) conv_fill(w, f, s);
}

// The one place a layout's contents come from: pack from the torch-layout weight, round once.  Runs when conv_form allocates the
// layout and when e2v_update_tensor has overwritten w.raw -- the same launches in the same order, so the bits are the same.
void e2v_ctx::conv_fill(const ConvW& w, ConvForm f, hipStream_t s) {
    // a 16-bit layout of n elements: packed in fp32 staging (the up2x tap sums are formed in fp32), rounded once
    auto fill16 = [&](const void* dst, bool up2, int mode) {
        const size_t n = up2 ? 4 * (size_t)w.cout * conv_up2x_packed_ld(w.cin) : (size_t)w.cout * w.ldw16;
        Act tmp(pool, (int64_t)((n + 1023) / 1024), 1024);
        if (up2) pack_conv_up2x(w.raw, tmp.p, w.cout, w.cin, s);
        else pack_conv3x3(w.raw, tmp.p, w.cout, w.cin, 64, s);                // the 64-channel-chunk layout
        to_h16(tmp.p, const_cast<void*>(dst), n, mode, s);
    };
    switch (f) {
        case FORM_DIRECT32: pack_conv3x3(w.raw, const_cast<float*>(w.w), w.cout, w.cin, 32, s); break;
        case FORM_BF16: fill16(w.w16, false, H16_BF16); break;
        case FORM_F16: fill16(w.w16h, false, H16_FP16); break;
        case FORM_BF16_UP2: fill16(w.w16_up2, true, H16_BF16); break;
        case FORM_F16_UP2: fill16(w.w16h_up2, true, H16_FP16); break;
        case FORM_WINO2:
        case FORM_WINO4: {
            const int m = f == FORM_WINO4 ? 4 : 2;
            const size_t n = (size_t)(m + 2) * (m + 2) * w.cout * w.cin;
            const float* u = m == 4 ? w.wino4 : w.wino;
            const void* u3 = m == 4 ? w.wino4_x3 : w.wino_x3;
            wino_pack_weights(w.raw, const_cast<float*>(u), w.cout, w.cin, m, s);
            if (u3) split_bf16x3(u, const_cast<void*>(u3), n, n, s);
            break;
        }
    }
}

// fp16 mode: the IEEE-half copy of a linear's weight, derived on first use from the fp32 matrix finalize() kept (same layout as the
// bf16 copy: rows zero-padded to in16), filed under the finalize() group that owns the layer.
static const void* lin_h16_form(e2v_ctx* c, const LinW& w, int mode, hipStream_t s) {
    e2v_ctx::AllocPart guard(c, w.part);
    const size_t n = (size_t)w.out * w.in16;
    float* d16 = c->dev_alloc((n + 1) / 2);
    if (w.in16 == w.in) {
        to_h16(w.w, d16, n, mode, s);
    } else {
        Act tmp(c->pool, (int64_t)((n + 1023) / 1024), 1024);
        pad_cols(w.w, w.in, tmp.p, w.in16, w.out, s);
        to_h16(tmp.p, d16, n, mode, s);
    }
    return d16;
}

const void* e2v_ctx::lin_f16(const LinW& w, hipStream_t s) {
    if (!w.w16h) w.w16h = lin_h16_form(this, w, H16_FP16, s);
    return w.w16h;
}

// The bf16 copy of a linear that finalize() left fp32 only (the metric towers; a tower in bf16 mode): the same derivation, on first
// use.  Both 16-bit copies of a tower stay until the part is finalized again -- switching a tower's mode back and forth costs nothing
// after the first call in each mode, and e2v_update_tensor keeps every copy that exists in step.
const void* e2v_ctx::lin_b16(const LinW& w, hipStream_t s) {
    if (!w.w16) w.w16 = lin_h16_form(this, w, H16_BF16, s);
    return w.w16;
}

void e2v_ctx::enter_stream(hipStream_t s) {
    if (has_last_stream && s != last_stream) {
        if (!stream_ev) E2V_HIP(hipEventCreateWithFlags(&stream_ev, hipEventDisableTiming));
        E2V_HIP(hipEventRecord(stream_ev, last_stream));
        E2V_HIP(hipStreamWaitEvent(s, stream_ev, 0));
    }
    last_stream = s;
    has_last_stream = true;
}

// =====================================================================================================
// finalize: torch layouts -> kernel layouts
// =====================================================================================================
namespace {

struct Packer {
    e2v_ctx* c;
    hipStream_t s = nullptr;
    bool f32_only = false;           // the part's PartRow::f32_only: a linear keeps its fp32 matrix and nothing else, in every compute mode
    std::vector<std::string> superseded;     // raw keys whose torch-layout tensor was re-laid out into a block of the part: finalize() releases them
    const WTensor& t(const std::string& k) {
        auto it = c->raw.find(k);
        E2V_REQUIRE(it != c->raw.end(), E2V_ENOWEIGHT, "unknown key " + k);
        if (dry_run()) {                                     // shapes only: the dispatch of a configuration does not depend on values
            if (!it->second.mem) it->second.mem = dev_block(it->second.numel * sizeof(float), 0, nullptr, false);
            return it->second;
        }
        E2V_REQUIRE(it->second.loaded, E2V_ENOWEIGHT, "state-dict key not loaded: " + k);
        return it->second;
    }
    // ---- where each raw key lands (model.h: WBind), for e2v_update_tensor ----
    void bind_raw(const std::string& k, const float* dst, int rows, int in, int half = 0) {
        WBind b;
        b.kind = WBind::RAW; b.dst = const_cast<float*>(dst); b.rows = rows; b.in = in; b.half = half;
        c->bind[k] = b;
    }
    void bind_lin(const std::string& k, const float* anchor, int row_off, int half = 0) {
        const WTensor& w = t(k);
        WBind b;
        b.kind = WBind::LIN; b.anchor = anchor; b.rows = (int)w.shape[0]; b.in = (int)w.shape[1]; b.row_off = row_off;
        b.half = half; b.blk = 32;
        c->bind[k] = b;
    }
    // a conv weight that IS a linear as it stands ([rows][in] over its trailing dims: the towers' patch convolutions): bound as one, so
    // that the 16-bit copies a tower builds on first use follow e2v_update_tensor and can be read back
    void bind_matrix(const std::string& k, const float* anchor, int rows, int in) {
        WBind b;
        b.kind = WBind::LIN; b.anchor = anchor; b.rows = rows; b.in = in; b.blk = 32;
        c->bind[k] = b;
    }
    const void* half(const float* w, size_t n) {             // bf16 copy of a (packed) weight for the bf16-MFMA mode
        float* d = c->dev_alloc((n + 1) / 2);
        to_bf16(w, d, n, s);
        return d;
    }
    // every form of one [out][in] matrix: fp32 as it is, bf16 with rows padded to a multiple of 8 (16-byte pieces), f32x3 planes
    LinW mk_lin(const float* w, const float* b, int in, int out) {
        const int in16 = (in + 7) / 8 * 8;
        if (f32_only) {
            LinW l{w, b, in, out};
            l.in16 = in16;
            l.part = c->alloc_part >= 0 ? c->alloc_part : 0;
            return l;
        }
        const void* w16;
        if (in16 == in) {
            w16 = half(w, (size_t)out * in);
        } else {
            const DevBlock tmp = dev_block((size_t)out * in16 * sizeof(float), 0, s, false);
            pad_cols(w, in, tmp.f32(), in16, out, s);
            w16 = half(tmp.f32(), (size_t)out * in16);
            E2V_HIP(hipStreamSynchronize(s));
        }
        LinW l{w, b, in, out, w16, split3(w, (size_t)out * in)};
        l.in16 = in16;
        l.part = c->alloc_part >= 0 ? c->alloc_part : 0;
        return l;
    }
    const void* split3(const float* w, size_t n) {           // three bf16 planes (f32x3 mode only)
        if (!c->x3_compute) return nullptr;
        float* d = c->dev_alloc((3 * n + 1) / 2);
        split_bf16x3(w, d, n, n, s);
        return d;
    }
    NormW norm(const std::string& n) {
        const NormW w{t(n + ".weight").d(), t(n + ".bias").d(), (int)t(n + ".weight").shape[0]};
        bind_raw(n + ".weight", w.g, 1, w.c); bind_raw(n + ".bias", w.b, 1, w.c);
        return w;
    }
    LinW lin(const std::string& n, bool bias = true) {       // Linear or 1x1 conv: [out][in] as it is
        const WTensor& w = t(n + ".weight");
        bind_lin(n + ".weight", w.d(), 0);
        if (bias) bind_raw(n + ".bias", t(n + ".bias").d(), 1, (int)w.shape[0]);
        return mk_lin(w.d(), bias ? t(n + ".bias").d() : nullptr, (int)w.shape[1], (int)w.shape[0]);
    }
    // 3x3 conv: the torch-layout weight stays; kernel layouts are built on first use (e2v_ctx::conv_form)
    ConvW conv3(const std::string& n) {
        const WTensor& w = t(n + ".weight");
        ConvW cw;
        cw.raw = w.d(); cw.b = t(n + ".bias").d();
        cw.cout = (int)w.shape[0]; cw.cin = (int)w.shape[1];
        cw.cin_pad = (cw.cin + 3) / 4 * 4; cw.cin_pad16 = (cw.cin + 7) / 8 * 8;
        cw.ldw = conv3x3_packed_ld(cw.cin, 32); cw.ldw16 = conv3x3_packed_ld(cw.cin, 64);
        cw.part = c->alloc_part >= 0 ? c->alloc_part : 0;
        WBind b;
        b.kind = WBind::CONV; b.anchor = cw.raw; b.rows = 1; b.in = (int)w.numel;
        c->bind[n + ".weight"] = b;
        bind_raw(n + ".bias", cw.b, 1, cw.cout);
        return cw;
    }
    LinW fuse_rows(const std::vector<std::string>& names, bool bias) {   // stack Linear weights along `out`
        int in = 0, out = 0;
        for (auto& n : names) { const WTensor& w = t(n + ".weight"); in = (int)w.shape[1]; out += (int)w.shape[0]; }
        float* d = c->dev_alloc((size_t)out * in);
        float* b = bias ? c->dev_alloc(out) : nullptr;
        int r = 0;
        for (auto& n : names) {
            const WTensor& w = t(n + ".weight");
            copy_rows(w.d(), in, d + (size_t)r * in, in, (int)w.shape[0], in, s);
            if (bias) copy_rows(t(n + ".bias").d(), (int)w.shape[0], b + r, (int)w.shape[0], 1, (int)w.shape[0], s);
            bind_lin(n + ".weight", d, r);
            superseded.push_back(n + ".weight");
            if (bias) { bind_raw(n + ".bias", b + r, 1, (int)w.shape[0]); superseded.push_back(n + ".bias"); }
            r += (int)w.shape[0];
        }
        return mk_lin(d, b, in, out);
    }
    LinW geglu(const std::string& n) {        // rows [value 0..4C) | gate 0..4C)] -> per 64: [32 value | 32 gate]
        const WTensor& w = t(n + ".weight");
        const WTensor& bsrc = t(n + ".bias");
        const int out = (int)w.shape[0], in = (int)w.shape[1], half = out / 2;
        E2V_REQUIRE(half % 32 == 0, E2V_EINVAL, "GEGLU inner width must be a multiple of 32");
        float* d = c->dev_alloc((size_t)out * in);
        float* b = c->dev_alloc(out);
        geglu_interleave(w.d(), bsrc.d(), half, in, d, b, s);
        bind_lin(n + ".weight", d, 0, half);
        bind_raw(n + ".bias", b, out / 32, 32, half / 32);       // 32-element groups, interleaved one by one
        superseded.push_back(n + ".weight"); superseded.push_back(n + ".bias");
        return mk_lin(d, b, in, out);
    }
    ResW resnet(const std::string& p, bool temb) {
        ResW r;
        r.n1 = norm(p + ".norm1"); r.c1 = conv3(p + ".conv1");
        if (temb) r.temb = lin(p + ".time_emb_proj");
        r.n2 = norm(p + ".norm2"); r.c2 = conv3(p + ".conv2");
        r.cin = r.c1.cin; r.cout = r.c1.cout;
        if (c->raw.count(p + ".conv_shortcut.weight")) r.sc = lin(p + ".conv_shortcut");
        return r;
    }
    TransW transformer(const std::string& p) {
        TransW w;
        const std::string b = p + ".transformer_blocks.0";
        w.norm = norm(p + ".norm"); w.proj_in = lin(p + ".proj_in"); w.proj_out = lin(p + ".proj_out");
        w.ln1 = norm(b + ".norm1"); w.ln2 = norm(b + ".norm2"); w.ln3 = norm(b + ".norm3"); w.lnt = norm(b + ".norm_temp");
        w.a1_qkv = fuse_rows({b + ".attn1.to_q", b + ".attn1.to_k", b + ".attn1.to_v"}, false);
        w.a1_out = lin(b + ".attn1.to_out.0");
        w.a2_q = lin(b + ".attn2.to_q", false);
        w.a2_kv = fuse_rows({b + ".attn2.to_k", b + ".attn2.to_v"}, false);
        w.a2_out = lin(b + ".attn2.to_out.0");
        w.ff1 = geglu(b + ".ff.net.0.proj"); w.ff2 = lin(b + ".ff.net.2");
        w.at_qkv = fuse_rows({b + ".attn_temp.to_q", b + ".attn_temp.to_k", b + ".attn_temp.to_v"}, false);
        w.at_out = lin(b + ".attn_temp.to_out.0");
        w.C = w.norm.c;
        return w;
    }
    VAEAttnW vae_attn(const std::string& a) {
        VAEAttnW w;
        w.norm = norm(a + ".group_norm");
        w.qkv = fuse_rows({a + ".query", a + ".key", a + ".value"}, true);
        w.proj = lin(a + ".proj_attn");
        w.C = w.norm.c;
        return w;
    }
    // ---- pieces the towers share ----
    // a plain table (class token, position rows, token embedding) read where it was loaded
    const float* table(const std::string& k, int rows, int cols) {
        const float* d = t(k).d();
        bind_raw(k, d, rows, cols);
        return d;
    }
    // a patch / tubelet convolution [C][3][(ts)][P][P] is the linear [C][K] over the patch rows as it stands
    LinW patch_linear(const std::string& n, int C, int K, bool bias) {
        const WTensor& w = t(n + ".weight");
        bind_matrix(n + ".weight", w.d(), C, K);
        if (bias) bind_raw(n + ".bias", t(n + ".bias").d(), 1, C);
        return mk_lin(w.d(), bias ? t(n + ".bias").d() : nullptr, K, C);
    }
    // a head [L][C] + [L] in a block of its own with rows of zeros appended up to a multiple of 4: the linear kernels store quads.
    // bound: the raw keys are bound to that block, which supersedes them (the classifiers); else they stay bound where they were
    // loaded (s2s.txtpredictor: the loaded tensors are the ones read back)
    LinW padded_head(const std::string& wk, const std::string& bk, int L, int C, bool bound) {
        const int Lp = (L + 3) / 4 * 4;
        float* d = c->dev_alloc((size_t)Lp * C);
        float* b = c->dev_alloc(Lp);
        E2V_HIP(hipMemsetAsync(d, 0, (size_t)Lp * C * sizeof(float), s));
        E2V_HIP(hipMemsetAsync(b, 0, (size_t)Lp * sizeof(float), s));
        copy_rows(t(wk).d(), C, d, C, L, C, s);
        copy_rows(t(bk).d(), L, b, L, 1, L, s);
        if (bound) {
            bind_lin(wk, d, 0);
            bind_raw(bk, b, 1, L);
            superseded.push_back(wk); superseded.push_back(bk);
        }
        return mk_lin(d, b, C, Lp);
    }
    LinW classifier(const std::string& n, int L, int C) {
        return L % 4 == 0 ? lin(n) : padded_head(n + ".weight", n + ".bias", L, C, true);
    }
    // a CLIPEncoderLayer under its checkpoint names (text., clipv.) and a transformers ViT / VideoMAE layer (image., video.): one packing
    TextLayerW clip_layer(const std::string& l) {
        TextLayerW w;
        w.ln1 = norm(l + ".layer_norm1"); w.ln2 = norm(l + ".layer_norm2");
        w.qkv = fuse_rows({l + ".self_attn.q_proj", l + ".self_attn.k_proj", l + ".self_attn.v_proj"}, true);
        w.out = lin(l + ".self_attn.out_proj");
        w.fc1 = lin(l + ".mlp.fc1"); w.fc2 = lin(l + ".mlp.fc2");
        return w;
    }
    TextLayerW encoder_layer(const std::string& l) {
        TextLayerW w;
        w.ln1 = norm(l + ".layernorm_before"); w.ln2 = norm(l + ".layernorm_after");
        w.qkv = fuse_rows({l + ".attention.attention.query", l + ".attention.attention.key", l + ".attention.attention.value"}, true);
        w.out = lin(l + ".attention.output.dense");
        w.fc1 = lin(l + ".intermediate.dense"); w.fc2 = lin(l + ".output.dense");
        return w;
    }

    // ---- one packing function per part (e2v_ctx::kParts; finalize() dispatches through pack) ----
    void pack_unet() {
        const int L = c->cfg.layers_per_block;
        UNetW u;
        u.conv_in = conv3("conv_in");
        u.te1 = lin("time_embedding.linear_1"); u.te2 = lin("time_embedding.linear_2");
        for (int i = 0; i < 4; ++i) {
            UNetW::Block b;
            for (int j = 0; j < L; ++j) {
                b.res.push_back(resnet(idx("down_blocks", i, "resnets", j), true));
                if (i < 3) b.attn.push_back(transformer(idx("down_blocks", i, "attentions", j)));
            }
            if (i != 3) { b.resample = true; b.rs = conv3("down_blocks." + std::to_string(i) + ".downsamplers.0.conv"); }
            u.down.push_back(std::move(b));
        }
        u.mid_r0 = resnet("mid_block.resnets.0", true);
        u.mid_attn = transformer("mid_block.attentions.0");
        u.mid_r1 = resnet("mid_block.resnets.1", true);
        for (int i = 0; i < 4; ++i) {
            UNetW::Block b;
            for (int j = 0; j < L + 1; ++j) {
                b.res.push_back(resnet(idx("up_blocks", i, "resnets", j), true));
                if (i > 0) b.attn.push_back(transformer(idx("up_blocks", i, "attentions", j)));
            }
            if (i != 3) { b.resample = true; b.rs = conv3("up_blocks." + std::to_string(i) + ".upsamplers.0.conv"); }
            u.up.push_back(std::move(b));
        }
        u.norm_out = norm("conv_norm_out");
        u.conv_out = conv3("conv_out");
        c->unet = std::move(u);
    }
    void pack_vae() {
        VAEW v;
        const int VL = c->cfg.vae_layers_per_block;
        v.post_quant = lin("vae.post_quant_conv");
        v.dec_in = conv3("vae.decoder.conv_in");
        v.dec_mid0 = resnet("vae.decoder.mid_block.resnets.0", false);
        v.dec_attn = vae_attn("vae.decoder.mid_block.attentions.0");
        v.dec_mid1 = resnet("vae.decoder.mid_block.resnets.1", false);
        for (int i = 0; i < 4; ++i) {
            VAEW::Block b;
            for (int j = 0; j < VL + 1; ++j) b.res.push_back(resnet(idx("vae.decoder.up_blocks", i, "resnets", j), false));
            if (i != 3) { b.resample = true; b.rs = conv3("vae.decoder.up_blocks." + std::to_string(i) + ".upsamplers.0.conv"); }
            v.dec_up.push_back(std::move(b));
        }
        v.dec_norm_out = norm("vae.decoder.conv_norm_out");
        v.dec_out = conv3("vae.decoder.conv_out");
        v.quant = lin("vae.quant_conv");
        v.enc_in = conv3("vae.encoder.conv_in");
        for (int i = 0; i < 4; ++i) {
            VAEW::Block b;
            for (int j = 0; j < VL; ++j) b.res.push_back(resnet(idx("vae.encoder.down_blocks", i, "resnets", j), false));
            if (i != 3) { b.resample = true; b.rs = conv3("vae.encoder.down_blocks." + std::to_string(i) + ".downsamplers.0.conv"); }
            v.enc_down.push_back(std::move(b));
        }
        v.enc_mid0 = resnet("vae.encoder.mid_block.resnets.0", false);
        v.enc_attn = vae_attn("vae.encoder.mid_block.attentions.0");
        v.enc_mid1 = resnet("vae.encoder.mid_block.resnets.1", false);
        v.enc_norm_out = norm("vae.encoder.conv_norm_out");
        v.enc_out = conv3("vae.encoder.conv_out");
        c->vae = std::move(v);
    }
    void pack_sem() {
        const e2v_config& cfg = c->cfg;
        c->sem.clear();
        // the first layer's K (310) is padded to a multiple of 8 (320 -> 312 would do for fp32's 16-byte rows, but the bf16
        // tile reads 8-element pieces): pad FIRST, then derive the bf16 / split copies from the padded matrix so that every
        // form of the layer has the same row length.  The loaded matrix stays: nothing of this part is superseded.
        c->sem_in_pad = (cfg.sem_in_features + 7) / 8 * 8;
        for (int i = 0; i < 5; ++i) {
            const std::string n = "semantic.mlp." + std::to_string(2 * i);
            if (i == 0 && c->sem_in_pad != cfg.sem_in_features) {
                const WTensor& w = t(n + ".weight");
                const int out = (int)w.shape[0];
                float* wp = c->dev_alloc((size_t)out * c->sem_in_pad);
                pad_cols(w.d(), cfg.sem_in_features, wp, c->sem_in_pad, out, nullptr);
                bind_lin(n + ".weight", wp, 0);
                bind_raw(n + ".bias", t(n + ".bias").d(), 1, out);
                c->sem.push_back(mk_lin(wp, t(n + ".bias").d(), c->sem_in_pad, out));
            } else {
                c->sem.push_back(lin(n));
            }
        }
    }
    void pack_text() {
        const e2v_config& cfg = c->cfg;
        TextW w;
        const std::string m = "text.text_model.";
        w.tok = table(m + "embeddings.token_embedding.weight", cfg.text_vocab_size, cfg.text_hidden);
        w.pos = table(m + "embeddings.position_embedding.weight", cfg.text_max_positions, cfg.text_hidden);
        for (int i = 0; i < cfg.text_layers; ++i) w.layers.push_back(clip_layer(m + "encoder.layers." + std::to_string(i)));
        w.ln_f = norm(m + "final_layer_norm");
        c->text = std::move(w);
    }
    void pack_image() {
        const e2v_config& cfg = c->cfg;
        VisionTowerW v;
        const std::string m = "image.vit.";
        const int C = cfg.vit_hidden;
        v.cls = table(m + "embeddings.cls_token", 1, C);
        v.pos = table(m + "embeddings.position_embeddings", c->image_tokens(), C);
        v.patch = patch_linear(m + "embeddings.patch_embeddings.projection", C, 3 * cfg.vit_patch_size * cfg.vit_patch_size, true);
        for (int i = 0; i < cfg.vit_layers; ++i) v.layers.push_back(encoder_layer(m + "encoder.layer." + std::to_string(i)));
        v.head_ln = norm(m + "layernorm");
        v.head = classifier("image.classifier", cfg.vit_num_labels, C);
        c->image = std::move(v);
    }
    void pack_video() {
        const e2v_config& cfg = c->cfg;
        VisionTowerW v;
        const std::string m = "video.videomae.";
        const int C = cfg.vmae_hidden;
        v.pos = table(m + "embeddings.position_embeddings", c->video_tokens(), C);
        v.patch = patch_linear(m + "embeddings.patch_embeddings.projection", C,
                               3 * cfg.vmae_tubelet_size * cfg.vmae_patch_size * cfg.vmae_patch_size, true);
        for (int i = 0; i < cfg.vmae_layers; ++i) v.layers.push_back(encoder_layer(m + "encoder.layer." + std::to_string(i)));
        v.head_ln = norm("video.fc_norm");
        v.head = classifier("video.classifier", cfg.vmae_num_labels, C);
        c->video = std::move(v);
    }
    void pack_clipv() {
        const e2v_clipv_config& cfg = c->vcfg;
        VisionTowerW v;
        const std::string m = "clipv.vision_model.";
        const int C = cfg.clipv_hidden;
        v.cls = table(m + "embeddings.class_embedding", 1, C);
        v.pos = table(m + "embeddings.position_embedding.weight", c->clipv_tokens(), C);
        v.patch = patch_linear(m + "embeddings.patch_embedding", C, 3 * cfg.clipv_patch_size * cfg.clipv_patch_size, false);
        v.pre_ln = norm(m + "pre_layrnorm");
        for (int i = 0; i < cfg.clipv_layers; ++i) v.layers.push_back(clip_layer(m + "encoder.layers." + std::to_string(i)));
        v.head_ln = norm(m + "post_layernorm");
        v.head = lin("clipv.visual_projection", false);
        c->clipv = std::move(v);
    }
    void pack_s2s() {
        const e2v_s2s_config& scfg = c->scfg;
        S2sW v;
        const int C = scfg.s2s_d_model, F1 = scfg.s2s_f1, D = scfg.s2s_d, F2 = scfg.s2s_f2, E = scfg.s2s_electrodes;
        // every tensor stays where e2v_load_tensor put it and is read back from there: a matrix is used as it stands, in_proj as views
        auto keep = [&](const std::string& k) -> const WTensor& {
            const WTensor& w = t(k);
            const int rows = w.shape.size() > 1 ? (int)w.shape[0] : 1;
            bind_raw(k, w.d(), rows, (int)(w.numel / (size_t)rows));
            return w;
        };
        auto klin = [&](const std::string& n) {
            const WTensor& w = keep(n + ".weight");
            return mk_lin(w.d(), keep(n + ".bias").d(), (int)w.shape[1], (int)w.shape[0]);
        };
        auto knorm = [&](const std::string& n) { return NormW{keep(n + ".weight").d(), keep(n + ".bias").d(), C}; };
        {   // the EEGNet embedding: the four convs and the three BatchNorms (eval mode: running statistics) folded on the host
            const std::string e = "s2s.eeg_embedding.";
            auto host = [&](const std::string& k) {
                const WTensor& w = keep(k);
                std::vector<float> h(w.numel);
                E2V_HIP(hipMemcpy(h.data(), w.d(), w.numel * sizeof(float), hipMemcpyDeviceToHost));
                return h;
            };
            auto host_bn = [&](const std::string& n) {
                std::vector<float> h;
                for (const char* f : {".weight", ".bias", ".running_mean", ".running_var"}) {
                    const std::vector<float> part = host(n + f);
                    h.insert(h.end(), part.begin(), part.end());
                }
                return h;
            };
            const std::vector<float> w1 = host(e + "block_1.1.weight"), w2 = host(e + "block_2.0.weight"), w3 = host(e + "block_3.1.weight"),
                                     w4 = host(e + "block_3.2.weight");
            const std::vector<float> bn1 = host_bn(e + "block_1.2"), bn2 = host_bn(e + "block_2.1"), bn3 = host_bn(e + "block_3.3");
            for (int i = 0; i < F1 * D; ++i)
                E2V_REQUIRE(bn2[3 * F1 * D + i] + scfg.s2s_bn_eps > 0.f, E2V_EINVAL, "s2s.eeg_embedding.block_2.1.running_var + eps must be positive");
            for (int i = 0; i < F1; ++i)
                E2V_REQUIRE(bn1[3 * F1 + i] + scfg.s2s_bn_eps > 0.f, E2V_EINVAL, "s2s.eeg_embedding.block_1.2.running_var + eps must be positive");
            for (int i = 0; i < F2; ++i)
                E2V_REQUIRE(bn3[3 * F2 + i] + scfg.s2s_bn_eps > 0.f, E2V_EINVAL, "s2s.eeg_embedding.block_3.3.running_var + eps must be positive");
            const std::vector<float> pk = eegnet_pack(EegnetHostW{w1.data(), bn1.data(), w2.data(), bn2.data(), w3.data(), w4.data(), bn3.data()},
                                                      E, F1, D, F2, scfg.s2s_bn_eps);
            float* d = c->dev_alloc(pk.size());
            E2V_HIP(hipMemcpy(d, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
            v.eegnet = d;
            v.embed = klin(e + "embedding");
        }
        v.pe = keep("s2s.positional_encoding.pe").d();
        // nn.MultiheadAttention: in_proj whole (self-attention) or as its q rows and its k | v rows (cross-attention)
        auto in_proj = [&](const std::string& n, int row0, int rows) {
            const WTensor& w = keep(n + ".in_proj_weight");
            const WTensor& b = keep(n + ".in_proj_bias");
            return mk_lin(w.d() + (size_t)row0 * C, b.d() + row0, C, rows);
        };
        for (int i = 0; i < scfg.s2s_encoder_layers; ++i) {
            const std::string l = "s2s.transformer_encoder.layers." + std::to_string(i);
            S2sEncLayerW w;
            w.qkv = in_proj(l + ".self_attn", 0, 3 * C); w.out = klin(l + ".self_attn.out_proj");
            w.fc1 = klin(l + ".linear1"); w.fc2 = klin(l + ".linear2");
            w.ln1 = knorm(l + ".norm1"); w.ln2 = knorm(l + ".norm2");
            v.enc.push_back(w);
        }
        for (int i = 0; i < scfg.s2s_decoder_layers; ++i) {
            const std::string l = "s2s.transformer_decoder.layers." + std::to_string(i);
            S2sDecLayerW w;
            w.qkv = in_proj(l + ".self_attn", 0, 3 * C); w.out = klin(l + ".self_attn.out_proj");
            w.q2 = in_proj(l + ".multihead_attn", 0, C); w.kv2 = in_proj(l + ".multihead_attn", C, 2 * C);
            w.out2 = klin(l + ".multihead_attn.out_proj");
            w.fc1 = klin(l + ".linear1"); w.fc2 = klin(l + ".linear2");
            w.ln1 = knorm(l + ".norm1"); w.ln2 = knorm(l + ".norm2"); w.ln3 = knorm(l + ".norm3");
            v.dec.push_back(w);
        }
        keep("s2s.txtpredictor.weight"); keep("s2s.txtpredictor.bias");
        v.txt = padded_head("s2s.txtpredictor.weight", "s2s.txtpredictor.bias", scfg.s2s_txt_classes, C, false);
        v.pred = klin("s2s.predictor");
        c->s2s = std::move(v);
    }
    void pack_glm() {
        const e2v_glm_config& g = c->gcfg;
        GlmW v;
        const int F = g.glm_filters, K = g.glm_taps, E = g.glm_emb;
        // every tensor stays where e2v_load_tensor put it and is read back from there (pack_s2s)
        auto keep = [&](const std::string& k) -> const WTensor& {
            const WTensor& w = t(k);
            const int rows = w.shape.size() > 1 ? (int)w.shape[0] : 1;
            bind_raw(k, w.d(), rows, (int)(w.numel / (size_t)rows));
            return w;
        };
        auto klin = [&](const std::string& n) {
            const WTensor& w = keep(n + ".weight");
            return mk_lin(w.d(), keep(n + ".bias").d(), (int)w.shape[1], (int)w.shape[0]);
        };
        auto head = [&](const std::string& n, int L) {
            keep(n + ".weight"); keep(n + ".bias");
            return padded_head(n + ".weight", n + ".bias", L, 2 * E, false);
        };
        auto host = [&](const std::string& k) {
            const WTensor& w = keep(k);
            std::vector<float> h(w.numel);
            E2V_HIP(hipMemcpy(h.data(), w.d(), w.numel * sizeof(float), hipMemcpyDeviceToHost));
            return h;
        };
        // shallownet: the two convolutions and the BatchNorm (eval mode: running statistics) folded on the host
        auto shallow = [&](const std::string& n, int C) {
            GlmNetW w;
            const std::vector<float> w1 = host(n + ".net.0.weight"), b1 = host(n + ".net.0.bias"), w2 = host(n + ".net.1.weight"), b2 = host(n + ".net.1.bias");
            std::vector<float> bn;
            for (const char* f : {".weight", ".bias", ".running_mean", ".running_var"}) {
                const std::vector<float> part = host(n + ".net.2" + f);
                bn.insert(bn.end(), part.begin(), part.end());
            }
            for (int i = 0; i < F; ++i) E2V_REQUIRE(bn[3 * F + i] + g.glm_bn_eps > 0.f, E2V_EINVAL, n + ".net.2.running_var + eps must be positive");
            const std::vector<float> pk = shallownet_fold(ShallowHostW{w1.data(), b1.data(), w2.data(), b2.data(), bn.data()}, C, F, K, g.glm_bn_eps);
            float* d = c->dev_alloc(pk.size());
            E2V_HIP(hipMemcpy(d, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
            w.fold = d;
            w.out = klin(n + ".out");
            return w;
        };
        // mlpnet: the first linear's K (electrodes * bands: 310) padded to a multiple of 4 with zero columns, in a block of its own
        auto mlp = [&](const std::string& n, int in) {
            GlmMlpW w;
            w.in = in;
            const int inp = (in + 3) / 4 * 4;
            if (inp == in) {
                w.l1 = klin(n + ".net.1");
            } else {
                const WTensor& m = keep(n + ".net.1.weight");
                const int out = (int)m.shape[0];
                float* wp = c->dev_alloc((size_t)out * inp);
                pad_cols(m.d(), in, wp, inp, out, s);
                w.l1 = mk_lin(wp, keep(n + ".net.1.bias").d(), inp, out);
            }
            w.l2 = klin(n + ".net.3");
            w.l3 = klin(n + ".net.5");
            return w;
        };
        if (g.glm_raw_out > 0) {
            v.raw_global = shallow("glm.raw.globalnet", g.glm_electrodes);
            v.raw_occ = shallow("glm.raw.occipital_localnet", g.glm_occ_count);
            v.raw_head = head("glm.raw.out", g.glm_raw_out);
        }
        if (g.glm_mlp_out > 0) {
            v.mlp_global = mlp("glm.mlp.globalnet", g.glm_electrodes * g.glm_bands);
            v.mlp_occ = mlp("glm.mlp.occipital_localnet", g.glm_occ_count * g.glm_bands);
            v.mlp_head = head("glm.mlp.out", g.glm_mlp_out);
        }
        c->glm = std::move(v);
    }
    void pack(e2v_ctx::Part p) {
        switch (p) {
            case e2v_ctx::UNET: pack_unet(); break;
            case e2v_ctx::VAE: pack_vae(); break;
            case e2v_ctx::SEM: pack_sem(); break;
            case e2v_ctx::TEXT: pack_text(); break;
            case e2v_ctx::IMAGE: pack_image(); break;
            case e2v_ctx::VIDEO: pack_video(); break;
            case e2v_ctx::CLIPV: pack_clipv(); break;
            case e2v_ctx::S2S: pack_s2s(); break;
            case e2v_ctx::GLM: pack_glm(); break;
            case e2v_ctx::N_PARTS: break;
        }
    }
};

}  // namespace

void e2v_ctx::finalize(int which) {
    Packer P{this};
    AllocPart part_guard(this, -1);                  // (an error below leaves no part selected)
    // everything that can refuse the call is checked BEFORE a part is freed: a failed finalize leaves the context as it was
    for (int p = 0; p < N_PARTS; ++p)
        if (which & kParts[p].bit) require_part((Part)p);
    E2V_REQUIRE(!(which & kParts[S2S].bit) || !dry_run(), E2V_ESTATE, "the Seq2Seq latent model has no dry run");
    E2V_REQUIRE(!(which & kParts[GLM].bit) || !dry_run(), E2V_ESTATE, "GLMNet has no dry run");
    for (const auto& k : keys)
        if (which & kParts[key_part(k)].bit) P.t(k);
    E2V_HIP(hipDeviceSynchronize());                 // a part finalized before may still be in use by queued work
    for (int p = 0; p < N_PARTS; ++p) {
        if (!(which & kParts[p].bit)) continue;
        free_part(p);
        alloc_part = p;
        P.f32_only = kParts[p].f32_only;
        P.pack((Part)p);
    }
    alloc_part = -1;
    resolve_bindings();
    E2V_HIP(hipStreamSynchronize(nullptr));
    E2V_HIP(hipGetLastError());
    if (dry_run()) which &= kParts[UNET].bit | kParts[VAE].bit;      // nothing was allocated, nothing to drop; a dry run describes these two only
    else
        for (const std::string& k : P.superseded) {  // the torch-layout copies of re-laid-out tensors are no longer needed
            WTensor& w = raw.at(k);
            if (w.mem) { w.mem.release(); w.loaded = false; }
        }
    for (int p = 0; p < N_PARTS; ++p)
        if (which & kParts[p].bit) ready[p] = true;
}

// =====================================================================================================
// in-place weight update (e2v_update_tensor)
// =====================================================================================================
namespace {

template <class FL, class FC> void visit(ResW& r, FL& fl, FC& fc) { fc(r.c1); fc(r.c2); fl(r.temb); fl(r.sc); }
template <class FL> void visit(TransW& w, FL& fl) {
    for (LinW* l : {&w.proj_in, &w.proj_out, &w.a1_qkv, &w.a1_out, &w.a2_q, &w.a2_kv, &w.a2_out, &w.ff1, &w.ff2, &w.at_qkv, &w.at_out}) fl(*l);
}
template <class FL, class FC> void visit(UNetW& u, FL& fl, FC& fc) {
    fc(u.conv_in); fc(u.conv_out); fl(u.te1); fl(u.te2);
    for (auto* blocks : {&u.down, &u.up})
        for (auto& b : *blocks) {
            for (auto& r : b.res) visit(r, fl, fc);
            for (auto& a : b.attn) visit(a, fl);
            if (b.resample) fc(b.rs);
        }
    visit(u.mid_r0, fl, fc); visit(u.mid_r1, fl, fc); visit(u.mid_attn, fl);
}
template <class FL, class FC> void visit(VAEW& v, FL& fl, FC& fc) {
    fl(v.post_quant); fl(v.quant);
    for (ConvW* c : {&v.dec_in, &v.dec_out, &v.enc_in, &v.enc_out}) fc(*c);
    for (ResW* r : {&v.dec_mid0, &v.dec_mid1, &v.enc_mid0, &v.enc_mid1}) visit(*r, fl, fc);
    for (VAEAttnW* a : {&v.dec_attn, &v.enc_attn}) { fl(a->qkv); fl(a->proj); }
    for (auto* blocks : {&v.dec_up, &v.enc_down})
        for (auto& b : *blocks) {
            for (auto& r : b.res) visit(r, fl, fc);
            if (b.resample) fc(b.rs);
        }
}

}  // namespace

// finalize() records a binding while the owner is still a temporary of the Packer; once the parts sit in the context, the owner is
// found again by the fp32 block it was built around (LinW::w / ConvW::raw: one per object)
void e2v_ctx::resolve_bindings() {
    std::unordered_map<const void*, LinW*> lins;
    std::unordered_map<const void*, ConvW*> convs;
    auto fl = [&](LinW& l) { if (l.w) lins[l.w] = &l; };
    auto fc = [&](ConvW& c) { if (c.raw) convs[c.raw] = &c; };
    visit(unet, fl, fc);
    visit(vae, fl, fc);
    for (auto& l : sem) fl(l);
    for (auto& l : text.layers) { fl(l.qkv); fl(l.out); fl(l.fc1); fl(l.fc2); }
    for (VisionTowerW* v : {&image, &video, &clipv}) {
        for (auto& l : v->layers) { fl(l.qkv); fl(l.out); fl(l.fc1); fl(l.fc2); }
        fl(v->patch); fl(v->head);
    }
    for (auto& kv : bind) {
        WBind& b = kv.second;
        if (b.kind == WBind::LIN) { auto it = lins.find(b.anchor); b.lin = it != lins.end() ? it->second : nullptr; }
        if (b.kind == WBind::CONV) { auto it = convs.find(b.anchor); b.conv = it != convs.end() ? it->second : nullptr; }
    }
}

void e2v_ctx::update_tensor(const std::string& key, const void* data, e2v_dtype dtype, bool on_device, hipStream_t s) {
    WTensor& t = raw.at(key);
    auto bi = bind.find(key);
    E2V_REQUIRE(bi != bind.end(), E2V_ESTATE, "no binding for " + key);
    const WBind& b = bi->second;
    const size_t esz = dtype == E2V_F32 ? 4 : 2;
    Act stage;
    if (!on_device) {                       // host source: staged in its own type, widened by the kernel
        stage = Act(pool, (int64_t)((t.numel * esz + 4095) / 4096), 1024);
        E2V_HIP(hipMemcpyAsync(stage.p, data, t.numel * esz, hipMemcpyHostToDevice, s));
        data = stage.p;
    }
    WeightScatterArgs a;
    a.src = data; a.src_mode = dtype == E2V_F32 ? H16_NONE : dtype == E2V_BF16 ? H16_BF16 : H16_FP16;
    a.rows = b.rows; a.in = b.in; a.row_off = b.row_off; a.half = b.half; a.blk = b.blk;
    const float* main32 = nullptr;          // the fp32 destination of the main launch
    switch (b.kind) {
        case WBind::RAW:
            a.d32 = b.dst; a.ld32 = b.in;
            break;
        case WBind::LIN: {
            E2V_REQUIRE(b.lin && b.row_off + b.rows <= b.lin->out && b.in <= b.lin->in, E2V_ESTATE, "stale binding for " + key);
            const LinW& l = *b.lin;
            a.d32 = const_cast<float*>(l.w); a.ld32 = l.in;
            a.d16b = const_cast<void*>(l.w16); a.d16h = const_cast<void*>(l.w16h); a.ld16 = l.in16;
            a.d3 = const_cast<void*>(l.w3); a.ld3 = l.in; a.plane = (long long)l.out * l.in;
            break;
        }
        case WBind::CONV:
            E2V_REQUIRE(b.conv && (size_t)b.conv->cout * b.conv->cin * 9 == t.numel, E2V_ESTATE, "stale binding for " + key);
            a.d32 = const_cast<float*>(b.conv->raw); a.ld32 = b.in;
            break;
    }
    main32 = a.d32;
    weight_scatter(a, s);
    if (t.d() && t.loaded && t.d() != main32) {         // the uploaded block is kept next to a re-laid-out copy (K-padded layer): a later
        WeightScatterArgs r;                        // finalize of this part must find the new values there
        r.src = data; r.src_mode = a.src_mode; r.rows = 1; r.in = (int)t.numel; r.d32 = t.d(); r.ld32 = r.in;
        weight_scatter(r, s);
    }
    if (b.kind == WBind::CONV) {            // every layout that exists is derived again, as conv_form derived it
        const ConvW& w = *b.conv;
        if (w.w) conv_fill(w, FORM_DIRECT32, s);
        if (w.w16) conv_fill(w, FORM_BF16, s);
        if (w.w16h) conv_fill(w, FORM_F16, s);
        if (w.w16_up2) conv_fill(w, FORM_BF16_UP2, s);
        if (w.w16h_up2) conv_fill(w, FORM_F16_UP2, s);
        if (w.wino) conv_fill(w, FORM_WINO2, s);
        if (w.wino4) conv_fill(w, FORM_WINO4, s);
    }
    E2V_HIP(hipGetLastError());
}

// =====================================================================================================
// weight read-back (e2v_read_tensor): the inverse map of update_tensor
// =====================================================================================================
WeightGatherArgs e2v_ctx::read_source(const std::string& key, int form) {
    auto bi = bind.find(key);
    E2V_REQUIRE(bi != bind.end(), E2V_ESTATE, "no binding for " + key);
    const WBind& b = bi->second;
    E2V_REQUIRE(form == E2V_FORM_F32 || b.kind == WBind::LIN, E2V_EINVAL,
                "e2v_read_tensor: only the weight of a linear keeps 16-bit copies or f32x3 planes with an inverse; read E2V_FORM_F32 of " + key);
    E2V_REQUIRE(weight_forms(key) & form, E2V_ESTATE, "form not built for " + key + " (e2v_op_weight_forms says which are)");
    WeightGatherArgs a;
    a.rows = b.rows; a.in = b.in; a.row_off = b.row_off; a.half = b.half; a.blk = b.blk;
    switch (b.kind) {
        case WBind::RAW:
            a.src = b.dst; a.ld = b.in; a.row_off = 0;
            break;
        case WBind::LIN: {
            E2V_REQUIRE(b.lin && b.row_off + b.rows <= b.lin->out && b.in <= b.lin->in, E2V_ESTATE, "stale binding for " + key);
            const LinW& l = *b.lin;
            if (form == E2V_FORM_F32) { a.src = l.w; a.ld = l.in; }
            else if (form == E2V_FORM_BF16) { a.src = l.w16; a.src_mode = H16_BF16; a.ld = l.in16; }
            else if (form == E2V_FORM_F16) { a.src = l.w16h; a.src_mode = H16_FP16; a.ld = l.in16; }
            else { a.src = l.w3; a.x3 = 1; a.ld = l.in; a.plane = (long long)l.out * l.in; }
            break;
        }
        case WBind::CONV:
            E2V_REQUIRE(b.conv && (size_t)b.conv->cout * b.conv->cin * 9 == (size_t)b.in, E2V_ESTATE, "stale binding for " + key);
            a.src = b.conv->raw; a.ld = b.in;
            break;
    }
    return a;
}

void e2v_ctx::read_tensor(const std::string& key, int form, void* out, e2v_dtype dtype, bool on_device, hipStream_t s) {
    const WTensor& t = raw.at(key);
    WeightGatherArgs a = read_source(key, form);
    E2V_REQUIRE((size_t)a.rows * a.in == t.numel, E2V_ESTATE, "stale binding for " + key);
    const size_t esz = dtype == E2V_F32 ? 4 : 2;
    Act stage;
    if (!on_device) stage = Act(pool, (int64_t)((t.numel * esz + 4095) / 4096), 1024);      // gathered here in `dtype`, then copied out
    a.dst = on_device ? out : stage.p;
    a.dst_mode = dtype == E2V_F32 ? H16_NONE : dtype == E2V_BF16 ? H16_BF16 : H16_FP16;
    if (bind.at(key).kind == WBind::LIN || a.half > 0)
        weight_gather(a, s);
    else                                    // conv and RAW tensors with no row map: a type-converting copy
        cvt_rows(a.src, a.ld, 0, a.dst, a.in, a.dst_mode, a.rows, a.in, a.in, s);
    E2V_HIP(hipGetLastError());
    if (!on_device) {
        E2V_HIP(hipMemcpyAsync(out, stage.p, t.numel * esz, hipMemcpyDeviceToHost, s));
        E2V_HIP(hipStreamSynchronize(s));
    }
}

int e2v_ctx::weight_forms(const std::string& key) {
    auto bi = bind.find(key);
    E2V_REQUIRE(bi != bind.end(), E2V_ESTATE, "no binding for " + key);
    const WBind& b = bi->second;
    int m = 0;
    if (b.kind == WBind::RAW) m = b.dst ? E2V_FORM_F32 : 0;
    if (b.kind == WBind::LIN && b.lin) {
        const LinW& l = *b.lin;
        m = (l.w ? E2V_FORM_F32 : 0) | (l.w16 ? E2V_FORM_BF16 : 0) | (l.w16h ? E2V_FORM_F16 : 0) | (l.w3 ? E2V_FORM_X3 : 0);
    }
    if (b.kind == WBind::CONV && b.conv) {
        const ConvW& w = *b.conv;
        m = (w.raw ? E2V_FORM_F32 : 0) | (w.w16 ? E2V_FORM_BF16 : 0) | (w.w16h ? E2V_FORM_F16 : 0) | (w.w ? E2V_FORM_CONV_DIRECT32 : 0) |
            (w.wino ? E2V_FORM_WINO2 : 0) | (w.wino4 ? E2V_FORM_WINO4 : 0) | (w.w16_up2 ? E2V_FORM_BF16_UP2 : 0) |
            (w.w16h_up2 ? E2V_FORM_F16_UP2 : 0) | (w.wino_x3 ? E2V_FORM_WINO2_X3 : 0) | (w.wino4_x3 ? E2V_FORM_WINO4_X3 : 0);
    }
    return m;
}

// =====================================================================================================
// graph runner
// =====================================================================================================
namespace {

struct Geo { int nimg, H, W; };     // images (= n*F frames) and their map size

// What a launch sets beyond its required arguments, by name (plain aggregates: a call site assigns the fields it means)
struct LinOpt {
    const float* resid = nullptr; int ldr = 0;               // out += resid
    const float* a1 = nullptr; int c1 = 0, lda1 = 0;         // second source: the last c1 of the K columns come from a1
    bool geglu = false;                                      // out[M][N/2]
    bool f32_io = false, out_f32 = false;                    // bf16-activation mode: see Runner::linear
    bool relu = false;                                       // out = max(out, 0) after the bias
};
struct ConvOpt {
    const float* rowbias = nullptr; int rows_per_sample = 1;
    int rb_ld = -1;              // stride between the samples' rowbias rows (0: one row for all; < 0: cout)
    const float* resid = nullptr;
    int gn_P = 0;                // > 0: the input is the RAW tensor and GroupNorm's affine + SiLU (statistics already in c->gn_scale,
                                 // slabs of gn_P rows) is applied on the way in -- only valid where the policy picks a Winograd form
    bool out_f32 = false;
    bool want_rb = false;        // a GroupNorm follows -- leave the row-block sums with the output (Act::rb) where the tensor can carry them
};
struct ResOpt {
    const float* temb_silu = nullptr; int temb_dim = 0;      // SiLU(emb) rows, one per sample (null: the block has no time embedding)
    const float* rb0 = nullptr; const float* rb1 = nullptr;  // row-block sums of x0 / x1 (Act::rb of the tensors; null: none)
};

struct Runner {
    e2v_ctx* c;
    hipStream_t s;
    const bool small_family;          // the dispatch family of the API call this runner serves (model.h), fixed for its lifetime
    int res_idx = 0, tr_idx = 0;      // position in the per-generate caches (resnets with a time embedding / transformers)
    int tower = -1;                   // >= 0: the runner serves a metric tower and this is ITS mode (e2v_set_tower_dtype), not the context's
    Pool& pool() { return c->pool; }
    // bf16-activation mode (e2v_set_compute_dtype(E2V_BF16)): every activation the graph stores in HBM is bf16; accumulation,
    // GroupNorm / LayerNorm statistics, softmax and the time-embedding rows stay fp32
    int h16() const { return tower >= 0 ? tower : c->bf16_compute ? c->h16_mode : 0; }      // the mode flag of every 16-bit launch: 1 bf16, 2 fp16 (h16.h)
    bool bf() const { return h16() != 0; }
    bool fp16() const { return h16() == H16_FP16; }
    const void* w16_of(const LinW& w) { return fp16() ? c->lin_f16(w, s) : c->lin_b16(w, s); }
    Act new_act(int64_t rows, int C) { return Act(pool(), rows, C, bf()); }
    // fp32 rows -> bf16 rows padded to `cpad` channels (boundary tensors: latents, z, images, conditioning)
    Act to_act16(const float* x, int cols, int cpad, int64_t rows) {
        Act o(pool(), rows, cpad, true);
        pad_cols(x, cols, o.p, cpad, rows, s, h16());
        return o;
    }

    // Small-batch family: ask for split-K where the launch leaves most of the chip idle AND K is deep enough to pay for the fp32
    // partials (each run at least E2V_SPLITK_MIN_DEPTH deep: the partial planes cost 8 bytes per output and run, a run of depth d
    // 2 d flops per output).  Returns the workspace the launch needs (kept alive by the caller until the launch is queued).
    Act sk_setup(IgemmArgs& g) {
        static const int* const on = knob("E2V_SPLITK", 1);
        static const int* const min_depth = E2V_AB_KNOB("E2V_SPLITK_MIN_DEPTH", 2048);     // (1024 / 640 and 400 tiles measured +-0: `make ab` only)
        static const int* const max_tiles = E2V_AB_KNOB("E2V_SPLITK_MAX_TILES", 256);
        if (!small_family || !g.a_bf16 || !*on || *min_depth < 64) return Act();
        const long K = (long)g.taps * (g.c0 + g.c1);
        const long tiles = (long)((g.M + 127) / 128) * ((g.N + 127) / 128);
        if (tiles >= *max_tiles || K < 2L * *min_depth) return Act();
        const int want = (int)std::min<long>(std::min<long>((512 + tiles - 1) / tiles, K / *min_depth), 16);
        return splitk_attach(pool(), g, want);
    }

    void gn_ws(int samples, int P, int C) {
        const size_t guard = (size_t)pool_guard_kib() * 1024;          // E2V_POOL_GUARD: guarded like a dev_alloc block
        c->gn_part.ensure((size_t)samples * groupnorm_chunks(P) * C * 2 * sizeof(float), guard, s);
        c->gn_scale.ensure((size_t)samples * C * 2 * sizeof(float), guard, s);      // (pointers steer the graph: a null workspace reads as "no GroupNorm in front")
    }

    // what gn and gn_stats share: the two sources, the affine, the slabs and the workspaces (grown here)
    GroupNormArgs gn_args(const NormW& w, const float* x0, int c0, const float* x1, int c1, int samples, int P, int groups, float eps) {
        const int C = c0 + c1;
        E2V_REQUIRE(C == w.c && C % groups == 0 && c0 % 4 == 0 && c1 % 4 == 0, E2V_ESHAPE, "GroupNorm channel mismatch");
        gn_ws(samples, P, C);
        GroupNormArgs a;
        a.bf16 = h16();
        a.x0 = x0; a.x1 = x1; a.c0 = c0; a.c1 = c1; a.ld0 = c0; a.ld1 = c1;
        a.gamma = w.g; a.beta = w.b; a.samples = samples; a.P = P; a.groups = groups; a.eps = eps;
        a.ws_part = c->gn_part.blk.f32(); a.ws_scale = c->gn_scale.blk.f32();
        return a;
    }

    // rb0 / rb1: row-block sums that came with the source tensors (Act::rb; null: none) -- the statistics pass over such a source is
    // skipped (bf16 mode, P a multiple of 64)
    Act gn(const NormW& w, const float* x0, int c0, const float* x1, int c1, int samples, int P, int groups, float eps,
           bool act, const float* rb0 = nullptr, const float* rb1 = nullptr) {
        GroupNormArgs a = gn_args(w, x0, c0, x1, c1, samples, P, groups, eps);
        Act out = new_act((int64_t)samples * P, c0 + c1);
        a.out = out.p; a.ldo = c0 + c1; a.silu = act ? 1 : 0;
        if (bf() && P % 64 == 0) { a.rb0 = rb0; a.rb1 = c1 > 0 ? rb1 : nullptr; }
        // (16-bit modes only: the fp32 mode keeps one summation order at every batch.  E2V_GN_FUSED_SMALL = 3: the one-kernel form in
        // BOTH families -- the A/B that priced it at B = 32, profiles/r05_shape_ab_b32_gn_fused.log)
        static const int* const gn_fused = knob("E2V_GN_FUSED_SMALL", 1);
        a.small_chunks = (small_family && bf()) ? 1 : 0;
        a.fused_small = (bf() && (small_family || *gn_fused == 3)) ? 1 : 0;
        groupnorm(a, s);
        return out;
    }

    // statistics only: (scale, shift) per (slab, channel) left in c->gn_scale for the conv's input transform
    void gn_stats(const NormW& w, const float* x0, int c0, const float* x1, int c1, int samples, int P, int groups, float eps) {
        groupnorm_stats(gn_args(w, x0, c0, x1, c1, samples, P, groups, eps), s);
    }

    Act ln(const NormW& w, const Act& x) {
        E2V_REQUIRE(x.C == w.c && x.C % 4 == 0 && x.C <= 1280, E2V_ESHAPE, "LayerNorm width unsupported");
        Act out = new_act(x.rows, x.C);
        layernorm(x.p, x.C, w.g, w.b, out.p, x.C, (int)x.rows, x.C, 1e-5f, s, h16());
        return out;
    }

    // out[M][N] = A[M][K] W^T + b (+ resid); geglu: out[M][N/2].
    // bf16-activation mode: A, resid and out are bf16 unless `f32_io` (the time-embedding MLP: fp32 rows in, fp32 rows out,
    // fp32 arithmetic) or `out_f32` (a boundary tensor: VAE moments, attention scores)
    Act linear(const LinW& w, const float* a, int lda, int64_t M, const LinOpt& o = {}) {
        const bool b16 = bf() && !o.f32_io;
        const int K = b16 ? w.in16 : w.in;
        const int K0 = K - o.c1;
        const int gran = b16 ? 8 : 4;
        E2V_REQUIRE(K0 > 0 && K0 % gran == 0 && o.c1 % gran == 0 && lda % gran == 0, E2V_ESHAPE, "linear: K must be a multiple of 4 (bf16: 8)");
        Act out(pool(), M, o.geglu ? w.out / 2 : w.out, b16 && !o.out_f32);
        IgemmArgs g;
        g.a0 = a; g.c0 = K0; g.lda0 = lda; g.a1 = o.a1; g.c1 = o.c1; g.lda1 = o.lda1;
        g.w = w.w; g.ldw = w.in; g.ldw16 = w.in16; g.out = out.p; g.ldc = out.C; g.bias = w.b;
        g.resid = o.resid; g.ldr = o.ldr; g.M = (int)M; g.N = w.out; g.taps = 1; g.geglu = o.geglu ? 1 : 0; g.relu = o.relu ? 1 : 0;
        if (b16) { g.w16 = w16_of(w); g.a_bf16 = h16(); g.out_f32 = o.out_f32 ? 1 : 0; g.resid_bf16 = o.resid ? 1 : 0; }
        if (c->x3_compute && w.w3) { g.x3 = 1; g.w3 = w.w3; g.w3_plane = (long long)w.out * w.in; }
        Act skws = sk_setup(g);
        igemm(g, s);
        return out;
    }
    static LinOpt residual(const float* resid, int ldr) { LinOpt o; o.resid = resid; o.ldr = ldr; return o; }
    static LinOpt f32_rows() { LinOpt o; o.f32_io = true; return o; }

    // 3x3 conv over `geo.nimg` images; (Hi, Wi) = logical input size (after nearest resize), (Ho, Wo) output size
    Act conv3(const ConvW& w, const float* x0, int c0, const float* x1, int c1, Geo geo, int Hi, int Wi, int Ho, int Wo,
              int stride, int pad, const ConvOpt& o = {}) {
        E2V_REQUIRE(c0 + c1 == (bf() ? w.cin_pad16 : w.cin_pad), E2V_ESHAPE, "conv: input channels do not match the weight");
        Act out(pool(), (int64_t)geo.nimg * Ho * Wo, w.cout, bf() && !o.out_f32);
        Conv3 d;
        d.x0 = x0; d.c0 = c0; d.x1 = x1; d.c1 = c1; d.nimg = geo.nimg; d.Hs = geo.H; d.Ws = geo.W;
        d.Hi = Hi; d.Wi = Wi; d.Ho = Ho; d.Wo = Wo; d.stride = stride; d.pad = pad;
        d.cout = w.cout; d.out = out.p; d.bias = w.b;
        d.rowbias = o.rowbias; d.rb_ld = o.rb_ld < 0 ? w.cout : o.rb_ld; d.rows_per_sample = o.rows_per_sample; d.resid = o.resid;
        if (const int wm = c->conv_wino_tile(w.cin, w.cout, stride, pad, Hi, Wi, Ho, Wo)) {
            c->conv_form(w, wm == 4 ? e2v_ctx::FORM_WINO4 : e2v_ctx::FORM_WINO2, s);
            const void* U3 = !c->x3_compute ? nullptr : wm == 4 ? w.wino4_x3 : w.wino_x3;
            conv3_wino(c, d, wm, wm == 4 ? w.wino4 : w.wino, U3, c->gn_scale.blk.f32(), o.gn_P, s);
            return out;
        }
        E2V_REQUIRE(o.gn_P == 0, E2V_EINVAL, "conv: fused GroupNorm needs the Winograd path");
        E2V_REQUIRE(c1 == 0 || c0 % 32 == 0, E2V_ESHAPE, "conv: the concat seam must be a multiple of 32 channels");
        IgemmArgs g = conv3_igemm(d);
        g.ldw = w.ldw; g.ldw16 = w.ldw16;
        if (bf()) { g.a_bf16 = h16(); g.out_f32 = o.out_f32 ? 1 : 0; g.resid_bf16 = o.resid ? 1 : 0; }
        // (small-batch family: the four parity launches of a small layer are a handful of 256-row tiles each -- 131 us per launch
        // measured at B = 1 on the 9x16 -> 18x32 conv -- while the gather form takes split-K: the sub-pixel form needs >= 128 tiles)
        const bool up2x_small = small_family && (long)((out.rows / 4 + 255) / 256) * ((w.cout + 319) / 320) < 128;
        if (bf() && c0 == w.cin && !up2x_small && bgemm_up2x_applies(g)) {       // exact 2x resize (Upsample3D): four 2x2 convs on the source map
            c->conv_form(w, fp16() ? e2v_ctx::FORM_F16_UP2 : e2v_ctx::FORM_BF16_UP2, s);
            bgemm_up2x_launch(g, fp16() ? w.w16h_up2 : w.w16_up2, s);
            return out;
        }
        c->conv_form(w, fp16() ? e2v_ctx::FORM_F16 : bf() ? e2v_ctx::FORM_BF16 : e2v_ctx::FORM_DIRECT32, s);
        g.w = w.w; g.w16 = fp16() ? w.w16h : w.w16;
        // GroupNorm statistics from the producer -- BUILT, BIT-EXACT, MEASURED AND NOT ADOPTED (`make ab` builds, E2V_GN_RB = 1; DESIGN
        // section 9, profiles/r04_shape_ab_gn_producer_sums.log): the sums are ALWAYS the canonical ones -- from the epilogue when the
        // launch runs on the 256-row staged kernel (E2V_GN_RB_EPILOGUE = 0: never, for the bit-identity test), else from rowblock_sums
        // over the stored tensor -- so a result never depends on which kernel (i.e. which batch size) served the layer.  At B = 32 the
        // GroupNorms save 4.0 ms per step + decode and the convs that take the sums lose 6.2 (+4..8 % each: the 256-row kernel is one
        // workgroup per CU, nothing hides a longer tile tail, while the statistics pass it replaces streams at 5 TB/s).
        static const int* const rb_on = E2V_AB_KNOB("E2V_GN_RB", 0);
        static const int* const rb_epi = E2V_AB_KNOB("E2V_GN_RB_EPILOGUE", 1);
        bool epilogue_sums = false;
        if (*rb_on && o.want_rb && h16() == H16_BF16 && !o.out_f32 && rbsum_capable(out.rows, w.cout)) {
            out.rb = pool().get((size_t)(out.rows / 64) * w.cout * 2);
            if (*rb_epi) { g.rbsum = out.rb; epilogue_sums = igemm_writes_rbsum(g); if (!epilogue_sums) g.rbsum = nullptr; }
        }
        Act skws = sk_setup(g);
        igemm(g, s);
        if (epilogue_sums) dry_tag(" +rbsum");
        if (out.rb && !epilogue_sums) rowblock_sums(out.p, w.cout, w.cout, out.rows, rbsum_rows_per_pass(w.cout), out.rb, s);
        return out;
    }

    // ResnetBlock3D.forward (resnet.py:174-204); x1 = skip tensor concatenated on channels (may be null).
    // samples x P rows share GroupNorm statistics and one time-embedding row; geo describes the frames.
    // The output carries its own row-block sums when P allows.
    Act resnet(const ResW& w, const float* x0, int c0, const float* x1, int c1, int samples, int P, Geo geo, int groups,
               float eps, const ResOpt& o = {}) {
        const bool rbw = bf() && P % 64 == 0;            // the GroupNorms that read conv1's / this block's output can use the sums
        E2V_REQUIRE(c0 + c1 == w.cin, E2V_ESHAPE, "resnet: channel mismatch");
        auto wino = [&](const ConvW& cw) { return c->conv_wino_tile(cw.cin, cw.cout, 1, 1, geo.H, geo.W, geo.H, geo.W) != 0; };
        Act tp;
        ConvOpt o1, o2;                                  // conv1 adds the time-embedding row of its sample, conv2 the shortcut
        o1.rows_per_sample = P;
        if (w.temb.w) {
            if (c->step_cache_on) {      // e2v_generate: time_emb_proj(SiLU(emb(t))) of every step was computed up front; one row
                o1.rowbias = c->temb_cache[res_idx++].p + (size_t)c->step_cache_step * w.cout;    // serves all samples (stride 0)
                o1.rb_ld = 0;
            } else {
                E2V_REQUIRE(o.temb_silu != nullptr, E2V_EINVAL, "resnet needs a time embedding");
                tp = linear(w.temb, o.temb_silu, o.temb_dim, samples, f32_rows());                          // :183 (fp32 rows)
                o1.rowbias = tp.p;
            }
        }
        Act h1;
        if (wino(w.c1)) {                        // GroupNorm + SiLU applied inside the conv's input transform
            gn_stats(w.n1, x0, c0, x1, c1, samples, P, groups, eps);                                  // :177-178
            o1.gn_P = P;
            h1 = conv3(w.c1, x0, c0, x1, c1, geo, geo.H, geo.W, geo.H, geo.W, 1, 1, o1);              // :180,186
        } else {
            Act hn = gn(w.n1, x0, c0, x1, c1, samples, P, groups, eps, true, o.rb0, o.rb1);          // :177-178
            o1.want_rb = rbw;
            h1 = conv3(w.c1, hn.p, w.cin, nullptr, 0, geo, geo.H, geo.W, geo.H, geo.W, 1, 1, o1);     // :180,186
        }
        Act sc;
        o2.resid = x0;
        if (w.sc.w) {                                                                                 // :199-200
            LinOpt cat;
            cat.a1 = x1; cat.c1 = c1; cat.lda1 = c1;
            sc = linear(w.sc, x0, c0, (int64_t)samples * P, cat);
            o2.resid = sc.p;
        } else {
            E2V_REQUIRE(c1 == 0, E2V_ESHAPE, "identity shortcut with a concatenated input");
        }
        if (wino(w.c2)) {
            gn_stats(w.n2, h1.p, w.cout, nullptr, 0, samples, P, groups, eps);                        // :188,194
            o2.gn_P = P;
            return conv3(w.c2, h1.p, w.cout, nullptr, 0, geo, geo.H, geo.W, geo.H, geo.W, 1, 1, o2);  // :197,202
        }
        Act h2 = gn(w.n2, h1.p, w.cout, nullptr, 0, samples, P, groups, eps, true, h1.rb);           // :188,194
        h1.reset();
        o2.want_rb = rbw;
        return conv3(w.c2, h2.p, w.cout, nullptr, 0, geo, geo.H, geo.W, geo.H, geo.W, 1, 1, o2);      // :197,202
    }

    // Transformer3DModel.forward + BasicTransformerBlock.forward (attention.py:89-136, 232-269)
    Act twice(const Act& a) {                        // [a ; a] along the rows
        Act d(pool(), 2 * a.rows, a.C, a.bf16);
        const size_t bytes = a.bytes();
        E2V_HIP(hipMemcpyAsync(d.p, a.p, bytes, hipMemcpyDeviceToDevice, s));
        E2V_HIP(hipMemcpyAsync(reinterpret_cast<char*>(d.p) + bytes, a.p, bytes, hipMemcpyDeviceToDevice, s));
        return d;
    }

    // n_shared > 0: `x` holds only n_shared = n / 2 samples whose two copies (the uncond / cond halves of a classifier-free
    // guidance batch, pipeline_tuneeeg2video.py:313) would be bit-identical up to the first use of the conditioning: the
    // per-frame GroupNorm, proj_in and the whole sparse-causal self-attention run once, then the tokens are duplicated.
    // `cond` is in the activation type (bf16 mode: already converted, see unet_forward_cl).
    Act transformer(const TransW& w, const Act& x_in, int n, int F, int HW, const float* cond, int T, int heads, int groups,
                    int n_shared = 0) {
        const int C = w.C, D = C / heads;
        const int64_t rows = (int64_t)n * F * HW;
        const int n1 = n_shared > 0 ? n_shared : n;                       // samples up to and including attn1
        const int64_t rows1 = (int64_t)n1 * F * HW;
        E2V_REQUIRE(n_shared == 0 || 2 * n_shared == n, E2V_EINVAL, "shared prefix needs n == 2 * n_shared");
        const Act* xp = &x_in;
        const float scale = 1.0f / std::sqrt((float)D);
        E2V_REQUIRE(C % heads == 0 && D % 8 == 0, E2V_EINVAL, "attention head dim must be a multiple of 8");
        const int io16 = h16();
        Act t;
        {
            Act hn = gn(w.norm, xp->p, C, nullptr, 0, n1 * F, HW, groups, 1e-6f, false, xp->rb);      // :99 (per frame)
            t = linear(w.proj_in, hn.p, C, rows1);                                                    // :101-103
        }
        {   // attn1: sparse-causal self-attention                                                      :234-243
            Act nrm = ln(w.ln1, t);
            Act qkv = linear(w.a1_qkv, nrm.p, C, rows1);
            nrm.reset();
            Act ao = new_act(rows1, C);
            AttnArgs a;
            a.q = qkv.p; a.ldq = 3 * C; a.k = qkv.at(C); a.v = qkv.at(2 * C); a.ldkv = 3 * C; a.o = ao.p; a.ldo = C;
            a.n = n1; a.F = F; a.heads = heads; a.D = D; a.Nq = HW; a.Nk = HW; a.mode = 0; a.scale = scale;
            a.io_bf16 = io16;
            a.x3 = c->x3_compute ? 1 : 0;
            flash_attention(a, s);
            qkv.reset();
            t = linear(w.a1_out, ao.p, C, rows1, residual(t.p, C));
        }
        Act x2;
        if (n_shared > 0) {                          // from here on the two halves see different conditioning
            t = twice(t);
            x2 = twice(*xp);
            xp = &x2;
        }
        {   // attn2: cross-attention to the cond tokens (identical for the F frames of a sample)         :245-255
            Act nrm = ln(w.ln2, t);
            Act q = linear(w.a2_q, nrm.p, C, rows);
            nrm.reset();
            Act kv_own;                        // e2v_generate computes to_k / to_v of the conditioning once for all steps
            const bool cached = c->step_cache_on;
            if (!cached) kv_own = linear(w.a2_kv, cond, w.a2_kv.in, (int64_t)n * T);
            const Act& kv = cached ? c->kv_cache[tr_idx] : kv_own;
            ++tr_idx;
            Act ao = new_act(rows, C);
            AttnArgs a;
            a.q = q.p; a.ldq = C; a.k = kv.p; a.v = kv.at(C); a.ldkv = 2 * C; a.o = ao.p; a.ldo = C;
            a.n = n; a.F = F; a.heads = heads; a.D = D; a.Nq = HW; a.Nk = T; a.mode = 1; a.scale = scale;
            a.io_bf16 = io16;
            a.x3 = c->x3_compute ? 1 : 0;
            flash_attention(a, s);
            t = linear(w.a2_out, ao.p, C, rows, residual(t.p, C));
        }
        {   // GEGLU feed-forward                                                                          :258
            Act nrm = ln(w.ln3, t);
            LinOpt gated;
            gated.geglu = true;
            Act hgate = linear(w.ff1, nrm.p, C, rows, gated);
            nrm.reset();
            t = linear(w.ff2, hgate.p, 4 * C, rows, residual(t.p, C));
        }
        {   // temporal attention over the F frames of each pixel                                         :261-267
            Act nrm = ln(w.lnt, t);
            Act qkv = linear(w.at_qkv, nrm.p, C, rows);
            nrm.reset();
            Act ao = new_act(rows, C);
            temporal_attention(qkv.p, 3 * C, ao.p, C, n, F, HW, heads, D, scale, s, io16);
            qkv.reset();
            t = linear(w.at_out, ao.p, C, rows, residual(t.p, C));
        }
        return linear(w.proj_out, t.p, C, rows, residual(xp->p, C));                                           // :123,130
    }

    // AttentionBlock of the VAE mid block (diffusers 0.11.1): one head over H*W tokens, per image.  The scores and the softmax
    // are fp32 in both modes; in bf16-activation mode the probabilities are rounded once, on their way into the PV product.
    Act vae_attention(const VAEAttnW& w, const Act& x, int nimg, int HW, int groups, float eps) {
        const int C = w.C;
        const int64_t rows = (int64_t)nimg * HW;
        Act qkv;
        {
            Act hn = gn(w.norm, x.p, C, nullptr, 0, nimg, HW, groups, eps, false);
            qkv = linear(w.qkv, hn.p, C, rows);
        }
        Act o = vae_attention_core(qkv, nimg, HW, C);
        return linear(w.proj, o.p, C, rows, residual(x.p, C));
    }

    // what lies between the qkv linear and the projection: softmax(q k^T C^-0.5) v per image over the fused rows qkv [nimg*HW][3C] in
    // the activation type, which are released as soon as V is transposed.  Also e2v_op_vae_attention_core (api.cpp), which passes fp32
    // tensors [nimg*HW][HW] to receive the scaled scores (before the softmax overwrites them) and the probabilities (16-bit modes: the
    // 16-bit copy the PV product reads, widened); the graph passes neither.
    Act vae_attention_core(Act& qkv, int nimg, int HW, int C, float* scores_out = nullptr, float* probs_out = nullptr) {
        E2V_REQUIRE(HW % (bf() ? 8 : 4) == 0, E2V_EINVAL, "VAE attention needs H*W to be a multiple of 4 (bf16: 8)");
        const int64_t rows = (int64_t)nimg * HW;
        Act sc(pool(), rows, HW);                                   // fp32 scores
        {
            IgemmArgs g;
            g.a0 = qkv.p; g.c0 = C; g.lda0 = 3 * C; g.w = qkv.at(C); g.ldw = 3 * C;
            g.out = sc.p; g.ldc = HW; g.M = HW; g.N = HW; g.taps = 1; g.alpha = 1.0f / std::sqrt((float)C);
            g.batch = nimg; g.sa0 = (long long)HW * 3 * C; g.sw = (long long)HW * 3 * C; g.sout = (long long)HW * HW;
            if (bf()) { g.a_bf16 = h16(); g.out_f32 = 1; g.w16 = qkv.at(C); g.ldw16 = 3 * C; }
            igemm(g, s);
        }
        if (scores_out) E2V_HIP(hipMemcpyAsync(scores_out, sc.p, sc.bytes(), hipMemcpyDeviceToDevice, s));
        Act p16;
        if (bf()) p16 = Act(pool(), rows, HW, true);
        softmax_rows(sc.p, HW, (int)rows, HW, s, bf() ? p16.p : nullptr, bf() ? h16() : H16_BF16);
        if (probs_out) {
            if (bf()) cvt_rows(p16.p, HW, h16(), probs_out, HW, 0, rows, HW, HW, s);      // exact
            else E2V_HIP(hipMemcpyAsync(probs_out, sc.p, sc.bytes(), hipMemcpyDeviceToDevice, s));
        }
        Act vt = new_act((int64_t)nimg * C, HW);
        transpose2d(qkv.at(2 * C), 3 * C, vt.p, HW, HW, C, nimg, (long long)HW * 3 * C, (long long)C * HW, s, bf() ? 1 : 0);
        qkv.reset();
        Act o = new_act(rows, C);
        {
            IgemmArgs g;
            g.a0 = bf() ? p16.p : sc.p; g.c0 = HW; g.lda0 = HW; g.w = vt.p; g.ldw = HW; g.out = o.p; g.ldc = C;
            g.M = HW; g.N = C; g.taps = 1; g.batch = nimg;
            g.sa0 = (long long)HW * HW; g.sw = (long long)C * HW; g.sout = (long long)HW * C;
            if (bf()) { g.a_bf16 = h16(); g.w16 = vt.p; g.ldw16 = HW; }
            igemm(g, s);
        }
        return o;
    }

    // time embedding (unet.py:324-345) of the n_t timesteps in c->d_timesteps, `rows` rows: sinusoid -> linear_1 -> SiLU -> linear_2
    // -> SiLU (resnets consume SiLU(emb)); fp32 rows in both modes.  tap(emb) sees linear_2's output (unet.py:345).
    template <class Tap>
    Act time_embedding(int n_t, int rows, int t_is_f32, Tap&& tap) {
        const int boc0 = c->cfg.block_out_channels[0];
        Act sin(pool(), rows, boc0);
        timestep_sinusoid(reinterpret_cast<const long long*>(c->d_timesteps.blk.data()), n_t, sin.p, rows, boc0, c->cfg.flip_sin_to_cos, c->cfg.freq_shift, s, t_is_f32);
        return time_mlp(sin, rows, tap);
    }
    // ... the part after the sinusoid
    template <class Tap>
    Act time_mlp(const Act& sin, int rows, Tap&& tap) {
        const int boc0 = c->cfg.block_out_channels[0], temb_dim = boc0 * 4;
        Act e1 = linear(c->unet.te1, sin.p, boc0, rows, f32_rows());
        silu(e1.p, e1.p, (long long)rows * temb_dim, s);
        Act emb = linear(c->unet.te2, e1.p, temb_dim, rows, f32_rows());
        tap(emb);
        silu(emb.p, emb.p, (long long)rows * temb_dim, s);
        return emb;
    }
};

int down_size(int x) { return (x - 1) / 2 + 1; }     // 3x3, stride 2, padding 1

}  // namespace

// -----------------------------------------------------------------------------------------------------
// UNet3DConditionModel.forward (unet.py:278-413), channel-last in and out
// -----------------------------------------------------------------------------------------------------
Act e2v_ctx::unet_forward_cl(const float* sample_cl, const int64_t* host_t, int n_t, const float* cond, int N, int F,
                             int H, int W, int T, hipStream_t s, bool cfg_pair, const float* host_tf) {
    require_ready(UNET);
    E2V_REQUIRE(n_t == 1 || n_t == N, E2V_EINVAL, "timesteps must have 1 or N entries");
    // cfg_pair: `sample_cl` holds N / 2 samples standing for [x ; x] (one timestep): everything before the first use of the
    // conditioning -- conv_in, the first resnet, the first transformer block up to its cross-attention -- is computed once
    E2V_REQUIRE(!cfg_pair || (N % 2 == 0 && n_t == 1 && !unet.down[0].attn.empty()), E2V_EINVAL, "cfg_pair needs an even batch, one timestep and a first block with attention");
    const int N1 = cfg_pair ? N / 2 : N;
    Runner R{this, s, unet_small_family(N)};                  // B <= 4 clips with their guidance pairs (model.h)
    const int groups = cfg.norm_num_groups;
    // heads of the blocks of resolution level l (unet.py:110-111,131,151,165,194: down block l, the mid block = level 3, up block 3 - l)
    auto heads_at = [&](int l) { return cfg.attention_heads_per_block[l] > 0 ? cfg.attention_heads_per_block[l] : cfg.attention_heads; };
    const float eps = cfg.norm_eps;
    const int boc0 = cfg.block_out_channels[0], temb_dim = boc0 * 4;

    // test aid (e2v_op_unet_forward_taps): activation [n * F * h * w][C] -> fp32 NCFHW at the sink's cursor
    auto tap = [&](const Act& a, int n, int C, int f, int h, int w) {
        TapSink& t = *tap_sink;
        const int64_t fhw = (int64_t)f * h * w, count = (int64_t)n * C * fhw;
        E2V_REQUIRE(t.count < 16 && t.used + count <= t.cap, E2V_EINVAL, "tap buffer too small");
        const float* rows = a.p;
        Act wide;
        if (a.bf16) {
            wide = Act(pool, a.rows, a.C);
            cvt_rows(a.p, a.C, h16_mode, wide.p, a.C, 0, a.rows, a.C, a.C, s);
            rows = wide.p;
        }
        cl_to_ncfhw(rows, a.C, t.buf + t.used, n, C, (int)fhw, 1.0f, 0.0f, 0, 0.f, 0.f, s);
        const int64_t shp[5] = {n, C, f, h, w};
        for (int i = 0; i < 5; ++i) t.shapes[t.count][i] = shp[i];
        t.used += count; ++t.count;
    };
    long long* d_t = timesteps(N, s);
    static_assert(sizeof(long long) == sizeof(int64_t), "int64");
    if (host_tf) E2V_HIP(hipMemcpyAsync(d_t, host_tf, sizeof(float) * n_t, hipMemcpyHostToDevice, s));
    else E2V_HIP(hipMemcpyAsync(d_t, host_t, sizeof(int64_t) * n_t, hipMemcpyHostToDevice, s));
    Act temb_silu;
    if (!step_cache_on)
        temb_silu = R.time_embedding(n_t, N, host_tf ? 1 : 0, [&](const Act& emb) { if (tap_sink) tap(emb, N, temb_dim, 1, 1, 1); });   // taps["emb"]
    // bf16-activation mode: the two fp32 boundary tensors are converted once -- the latents (zero-padded to 8 channels, the
    // 16-byte granule of the bf16 kernels) and, when no per-run cache holds to_k / to_v already, the conditioning
    Act sample16, cond16;
    const int cin_act = R.bf() ? unet.conv_in.cin_pad16 : unet.conv_in.cin_pad;
    if (R.bf()) {
        sample16 = R.to_act16(sample_cl, unet.conv_in.cin_pad, cin_act, (int64_t)N1 * F * H * W);
        sample_cl = sample16.p;
        if (!step_cache_on) {
            cond16 = R.to_act16(cond, cfg.cross_attention_dim, cfg.cross_attention_dim, (int64_t)N * T);
            cond = cond16.p;
        }
    }

    int hs[4], ws[4];
    hs[0] = H; ws[0] = W;
    for (int i = 1; i < 4; ++i) { hs[i] = down_size(hs[i - 1]); ws[i] = down_size(ws[i - 1]); }

    struct Skip { Act a; int lvl; };
    std::vector<Skip> skips;
    skips.reserve(16);
    auto P_of = [&](int l) { return F * hs[l] * ws[l]; };
    auto geo_of = [&](int l) { return Geo{N * F, hs[l], ws[l]}; };
    ResOpt ro;                                                                      // every resnet: SiLU(emb) ...
    ro.temb_silu = temb_silu.p; ro.temb_dim = temb_dim;
    auto res_opt = [&](const float* rb0, const float* rb1 = nullptr) { ResOpt o = ro; o.rb0 = rb0; o.rb1 = rb1; return o; };   // ... + the sources' row-block sums

    Act x = R.conv3(unet.conv_in, sample_cl, cin_act, nullptr, 0, Geo{N1 * F, hs[0], ws[0]}, H, W, H, W, 1, 1);   // :358
    Act x_shared;                                     // cfg_pair: the N / 2-sample conv_in output feeding the first resnet
    if (cfg_pair) { x_shared = std::move(x); x = R.twice(x_shared); }
    // The skip tensors alias the running activation in the reference; here the running tensor is moved
    // into the skip list and read from there (no copy) -- `x` then points at the list's last entry.
    auto keep = [&](Act&& a, int lvl) -> const Act& {
        skips.push_back(Skip{std::move(a), lvl});
        return skips.back().a;
    };
    const Act* cur = &keep(std::move(x), 0);                                                         // :361
    for (int i = 0; i < 4; ++i) {                                                                    // :362-373
        const UNetW::Block& b = unet.down[i];
        for (size_t j = 0; j < b.res.size(); ++j) {
            Act h;
            if (cfg_pair && i == 0 && j == 0) {      // shared prefix: N / 2 samples through the resnet and up to attn2
                h = R.resnet(b.res[j], x_shared.p, x_shared.C, nullptr, 0, N1, P_of(i), Geo{N1 * F, hs[0], ws[0]}, groups, eps, ro);
                x_shared.reset();
                h = R.transformer(b.attn[j], h, N, F, hs[i] * ws[i], cond, T, heads_at(i), groups, N1);
            } else {
                h = R.resnet(b.res[j], cur->p, cur->C, nullptr, 0, N, P_of(i), geo_of(i), groups, eps, res_opt(cur->rb));
                if (!b.attn.empty()) h = R.transformer(b.attn[j], h, N, F, hs[i] * ws[i], cond, T, heads_at(i), groups);
            }
            cur = &keep(std::move(h), i);
        }
        if (b.resample) {                                                                            // resnet.py:99-107
            ConvOpt o;
            o.want_rb = R.bf() && P_of(i + 1) % 64 == 0;               // (the next level's first GroupNorm and, as a skip, a later one read it)
            Act d = R.conv3(b.rs, cur->p, cur->C, nullptr, 0, geo_of(i), hs[i], ws[i], hs[i + 1], ws[i + 1], 2, 1, o);
            cur = &keep(std::move(d), i + 1);
        }
        if (tap_sink) { const int l = b.resample ? i + 1 : i; tap(*cur, N, cfg.block_out_channels[i], F, hs[l], ws[l]); }       // taps["down{i}"]
    }
    // mid (unet_blocks.py:199-205)
    Act h = R.resnet(unet.mid_r0, cur->p, cur->C, nullptr, 0, N, P_of(3), geo_of(3), groups, eps, res_opt(cur->rb));
    h = R.transformer(unet.mid_attn, h, N, F, hs[3] * ws[3], cond, T, heads_at(3), groups);
    h = R.resnet(unet.mid_r1, h.p, h.C, nullptr, 0, N, P_of(3), geo_of(3), groups, eps, res_opt(h.rb));
    if (tap_sink) tap(h, N, cfg.block_out_channels[3], F, hs[3], ws[3]);                               // taps["mid"]
    // up (unet.py:381-404)
    for (int i = 0; i < 4; ++i) {
        const UNetW::Block& b = unet.up[i];
        const int lvl = 3 - i;
        for (size_t j = 0; j < b.res.size(); ++j) {
            E2V_REQUIRE(!skips.empty() && skips.back().lvl == lvl, E2V_ESTATE, "skip bookkeeping out of step");
            Skip sk = std::move(skips.back());                                                       // unet_blocks.py:485-487
            skips.pop_back();
            Act o = R.resnet(b.res[j], h.p, h.C, sk.a.p, sk.a.C, N, P_of(lvl), geo_of(lvl), groups, eps, res_opt(h.rb, sk.a.rb));
            if (!b.attn.empty()) o = R.transformer(b.attn[j], o, N, F, hs[lvl] * ws[lvl], cond, T, heads_at(lvl), groups);
            h = std::move(o);
        }
        if (b.resample) {   // Upsample3D: nearest to the next skip's (f,h,w) then 3x3 conv (resnet.py:58-69, unet.py:389-390)
            h = R.conv3(b.rs, h.p, h.C, nullptr, 0, geo_of(lvl), hs[lvl - 1], ws[lvl - 1], hs[lvl - 1], ws[lvl - 1], 1, 1);
        }
        if (tap_sink) { const int l = b.resample ? lvl - 1 : lvl; tap(h, N, cfg.block_out_channels[lvl], F, hs[l], ws[l]); }   // taps["up{i}"]
    }
    Act hn = R.gn(unet.norm_out, h.p, h.C, nullptr, 0, N, P_of(0), groups, eps, true, h.rb);           // :406-407
    h.reset();
    ConvOpt f32_out;
    f32_out.out_f32 = true;                                                                            // eps: fp32
    Act out = R.conv3(unet.conv_out, hn.p, hn.C, nullptr, 0, geo_of(0), H, W, H, W, 1, 1, f32_out);   // :408
    E2V_HIP(hipGetLastError());
    return out;
}

// What a denoising loop can compute once instead of once per step ("precompute all 50 x 22 vectors once per
// run"): the time-embedding MLP and every resnet's time_emb_proj for all evaluations (one GEMM of `steps` rows per resnet
// instead of `steps` GEMMs of N identical rows), and to_k / to_v of the conditioning of every cross-attention.  Row-wise
// the arithmetic is the uncached one, so results are bit-identical.  Row i belongs to EVALUATION i (PNDM evaluates one timestep
// twice); an integral timestep takes the int64 sinusoid path and a fractional one the fp32 path, as e2v_unet_forward /
// e2v_unet_forward_ft would for that evaluation alone: one sinusoid launch per run of evaluations of one kind (a DDIM / PNDM /
// DPM-Solver++ schedule is one run; linspace(0, 999, 7)[::-1] = 999, 832.5, 666, ... alternates).
void e2v_ctx::build_step_caches(const EvalTime* ev, int steps, const float* cond, int N, int T, bool small_family, hipStream_t s) {
    Runner R{this, s, small_family};
    temb_cache.clear();
    kv_cache.clear();
    const int boc0 = cfg.block_out_channels[0], temb_dim = boc0 * 4;
    // the buffer holds `steps` int64 values followed by `steps` floats (entry i of the array its kind names is the one read)
    std::vector<int64_t> ti(steps);
    std::vector<float> tf(steps);
    bool any_frac = false;
    for (int i = 0; i < steps; ++i) { ti[i] = ev[i].t; tf[i] = ev[i].tf; any_frac = any_frac || ev[i].frac; }
    long long* d_ti = timesteps(any_frac ? 2 * steps : steps, s);
    const float* d_tf = reinterpret_cast<const float*>(d_ti + steps);
    E2V_HIP(hipMemcpyAsync(d_ti, ti.data(), sizeof(int64_t) * steps, hipMemcpyHostToDevice, s));
    if (any_frac) E2V_HIP(hipMemcpyAsync(const_cast<float*>(d_tf), tf.data(), sizeof(float) * steps, hipMemcpyHostToDevice, s));
    Act sin(pool, steps, boc0);
    for (int a = 0; a < steps;) {
        int b = a + 1;
        while (b < steps && ev[b].frac == ev[a].frac) ++b;
        const long long* src = ev[a].frac ? reinterpret_cast<const long long*>(d_tf + a) : d_ti + a;
        timestep_sinusoid(src, b - a, sin.p + (size_t)a * boc0, b - a, boc0, cfg.flip_sin_to_cos, cfg.freq_shift, s, ev[a].frac ? 1 : 0);
        a = b;
    }
    Act emb = R.time_mlp(sin, steps, [](const Act&) {});
    Act cond16;
    if (R.bf()) {
        cond16 = R.to_act16(cond, cfg.cross_attention_dim, cfg.cross_attention_dim, (int64_t)N * T);
        cond = cond16.p;
    }
    auto add_res = [&](const ResW& r) {
        if (r.temb.w) temb_cache.push_back(R.linear(r.temb, emb.p, temb_dim, steps, R.f32_rows()));
    };
    auto add_tr = [&](const TransW& w) { kv_cache.push_back(R.linear(w.a2_kv, cond, w.a2_kv.in, (int64_t)N * T)); };
    for (const auto& b : unet.down) { for (const auto& r : b.res) add_res(r); for (const auto& a : b.attn) add_tr(a); }
    add_res(unet.mid_r0); add_tr(unet.mid_attn); add_res(unet.mid_r1);
    for (const auto& b : unet.up) { for (const auto& r : b.res) add_res(r); for (const auto& a : b.attn) add_tr(a); }
}

// -----------------------------------------------------------------------------------------------------
// AutoencoderKL (diffusers 0.11.1).  Images are independent: "samples" = frames, F = 1.
// -----------------------------------------------------------------------------------------------------
void e2v_ctx::vae_decode_frames(const float* z_cl, int nf, int h, int w, float* out_cl, hipStream_t s, bool small) {
    require_ready(VAE);
    Runner R{this, s, small};                                 // the CALL decodes at most four clips (the caller knows: a pass may be a call's ragged last group)
    const int g = cfg.vae_norm_num_groups;
    const float eps = cfg.vae_norm_eps;
    const int lat = cfg.vae_latent_channels;
    int H = h, W = w;
    Act z16;
    int zc = lat;
    if (R.bf()) {                                // bf16-activation mode: z zero-padded to the 8-channel granule
        zc = vae.post_quant.in16;
        z16 = R.to_act16(z_cl, lat, zc, (int64_t)nf * H * W);
        z_cl = z16.p;
    }
    Act x = R.linear(vae.post_quant, z_cl, zc, (int64_t)nf * H * W);
    if (R.bf() && x.C != vae.dec_in.cin_pad16) {         // 4 -> 8 channels for the 3x3 conv's 16-byte pieces
        Act xp(pool, x.rows, vae.dec_in.cin_pad16, true);
        E2V_HIP(hipMemsetAsync(xp.p, 0, xp.bytes(), s));
        E2V_HIP(hipMemcpy2DAsync(xp.p, (size_t)xp.C * 2, x.p, (size_t)x.C * 2, (size_t)x.C * 2, (size_t)x.rows, hipMemcpyDeviceToDevice, s));
        x = std::move(xp);
    }
    x = R.conv3(vae.dec_in, x.p, x.C, nullptr, 0, Geo{nf, H, W}, H, W, H, W, 1, 1);
    x = R.resnet(vae.dec_mid0, x.p, x.C, nullptr, 0, nf, H * W, Geo{nf, H, W}, g, eps);
    x = R.vae_attention(vae.dec_attn, x, nf, H * W, g, eps);
    x = R.resnet(vae.dec_mid1, x.p, x.C, nullptr, 0, nf, H * W, Geo{nf, H, W}, g, eps);
    for (size_t i = 0; i < vae.dec_up.size(); ++i) {
        const VAEW::Block& b = vae.dec_up[i];
        for (const ResW& r : b.res) x = R.resnet(r, x.p, x.C, nullptr, 0, nf, H * W, Geo{nf, H, W}, g, eps);
        if (b.resample) {        // F.interpolate(scale_factor=2, nearest) + 3x3 conv
            x = R.conv3(b.rs, x.p, x.C, nullptr, 0, Geo{nf, H, W}, 2 * H, 2 * W, 2 * H, 2 * W, 1, 1);
            H *= 2; W *= 2;
        }
    }
    Act hn = R.gn(vae.dec_norm_out, x.p, x.C, nullptr, 0, nf, H * W, g, eps, true);
    x.reset();
    ConvOpt f32_out;
    f32_out.out_f32 = true;                                                                            // frames: fp32
    Act y = R.conv3(vae.dec_out, hn.p, hn.C, nullptr, 0, Geo{nf, H, W}, H, W, H, W, 1, 1, f32_out);
    E2V_HIP(hipMemcpyAsync(out_cl, y.p, (size_t)y.rows * y.C * sizeof(float), hipMemcpyDeviceToDevice, s));
    E2V_HIP(hipGetLastError());
}

void e2v_ctx::vae_encode_frames(const float* img_cl4, int n, int H0, int W0, float* moments_cl, hipStream_t s) {
    require_ready(VAE);
    Runner R{this, s, n <= 12};                               // frames, whatever E2V_SMALL_FAMILY_CLIPS says (ADVICE.md finding 2 would derive it from the knob)
    const int g = cfg.vae_norm_num_groups;
    const float eps = cfg.vae_norm_eps;
    int H = H0, W = W0;
    Act img16;
    int ic = vae.enc_in.cin_pad;
    if (R.bf()) {
        ic = vae.enc_in.cin_pad16;
        img16 = R.to_act16(img_cl4, vae.enc_in.cin_pad, ic, (int64_t)n * H * W);
        img_cl4 = img16.p;
    }
    Act x = R.conv3(vae.enc_in, img_cl4, ic, nullptr, 0, Geo{n, H, W}, H, W, H, W, 1, 1);
    for (size_t i = 0; i < vae.enc_down.size(); ++i) {
        const VAEW::Block& b = vae.enc_down[i];
        for (const ResW& r : b.res) x = R.resnet(r, x.p, x.C, nullptr, 0, n, H * W, Geo{n, H, W}, g, eps);
        if (b.resample) {        // F.pad(x, (0,1,0,1)) then 3x3 stride-2 conv without padding
            const int Ho = (H + 1 - 3) / 2 + 1, Wo = (W + 1 - 3) / 2 + 1;
            x = R.conv3(b.rs, x.p, x.C, nullptr, 0, Geo{n, H, W}, H, W, Ho, Wo, 2, 0);
            H = Ho; W = Wo;
        }
    }
    x = R.resnet(vae.enc_mid0, x.p, x.C, nullptr, 0, n, H * W, Geo{n, H, W}, g, eps);
    x = R.vae_attention(vae.enc_attn, x, n, H * W, g, eps);
    x = R.resnet(vae.enc_mid1, x.p, x.C, nullptr, 0, n, H * W, Geo{n, H, W}, g, eps);
    Act hn = R.gn(vae.enc_norm_out, x.p, x.C, nullptr, 0, n, H * W, g, eps, true);
    x.reset();
    Act y = R.conv3(vae.enc_out, hn.p, hn.C, nullptr, 0, Geo{n, H, W}, H, W, H, W, 1, 1);
    LinOpt f32_out;
    f32_out.out_f32 = true;                                                                            // moments: fp32
    Act m = R.linear(vae.quant, y.p, y.C, y.rows, f32_out);
    E2V_HIP(hipMemcpyAsync(moments_cl, m.p, (size_t)m.rows * m.C * sizeof(float), hipMemcpyDeviceToDevice, s));
    E2V_HIP(hipGetLastError());
}

// e2v_op_vae_attention_core: Runner::vae_attention_core, the code the two graphs above run, on the caller's fp32 tensors.  16-bit modes:
// qkv rounded once to the type on entry, the 16-bit result widened (exactly) on exit.
void e2v_ctx::vae_attention_core(const float* qkv, int nimg, int HW, int C, float* out, float* scores, float* probs, hipStream_t s) {
    Runner R{this, s, false};
    const int64_t rows = (int64_t)nimg * HW;
    Act in;
    if (R.bf()) {
        in = Act(pool, rows, 3 * C, true);
        cvt_rows(qkv, 3 * C, 0, in.p, 3 * C, R.h16(), rows, 3 * C, 3 * C, s);
    } else {                                     // the caller's rows as they lie (no pool: reset() leaves them alone)
        in.p = const_cast<float*>(qkv); in.rows = rows; in.C = 3 * C;
    }
    Act o = R.vae_attention_core(in, nimg, HW, C, scores, probs);
    if (R.bf()) cvt_rows(o.p, C, R.h16(), out, C, 0, rows, C, C, s);
    else E2V_HIP(hipMemcpyAsync(out, o.p, o.bytes(), hipMemcpyDeviceToDevice, s));
    E2V_HIP(hipGetLastError());
}

// -----------------------------------------------------------------------------------------------------
// The encoder layers of a metric tower (parts 16 / 32 / 64: pre-LN, no mask, head dim 64) over n sequences of T token rows, in the
// mode of the tower the runner serves (Runner::tower, e2v_set_tower_dtype) -- ONE body for the three modes, and in its fp32 form, with
// the causal kernel as `attn32`, the layers of the text encoder (text_encode):
//   fp32 (0)    fp32 rows, the linears as the time-embedding MLP takes them (f32_rows), attention by `attn32` (the tower's fp32 kernel);
//   bf16 / fp16 the token rows live in HBM as 16-bit; LayerNorm is the 16-bit kernel (fp32 statistics, the tower's eps); the linears
//               are 16-bit MFMA with fp32 accumulation, fp32 bias and residual added before the one store rounding; the activation is
//               computed in fp32 on 16-bit storage, in place; attention is flash_attention on the 16-bit rows (mode 1, F = 1,
//               Nq = Nk = T: fp32 scores and softmax, 16-bit P and output).
// Every kernel computes a row from its own sequence in an order fixed by (T, C, I), and the runner is of the large dispatch family (no
// split-K), so a sequence's bits do not depend on n.
// -----------------------------------------------------------------------------------------------------
namespace {

LinOpt tower_rows(const Runner& R) { LinOpt o; o.f32_io = !R.bf(); return o; }      // fp32 mode: fp32 rows whatever the context's mode

template <class Attn32>
Act tower_layers(Runner& R, const std::vector<TextLayerW>& layers, Act x, int n, int T, int heads, int I, float eps, int act, Attn32 attn32) {
    const int C = heads * 64, h16 = R.h16();
    const int64_t M = (int64_t)n * T;
    hipStream_t s = R.s;
    E2V_REQUIRE(!h16 || I % 8 == 0, E2V_ESHAPE, "a tower in 16-bit mode needs an intermediate width that is a multiple of 8");
    auto ln = [&](const NormW& w, const Act& in, Act& out) { layernorm(in.p, C, w.g, w.b, out.p, C, (int)M, C, eps, s, h16); };
    auto plus = [&](const Act& r) { LinOpt o = tower_rows(R); o.resid = r.p; o.ldr = C; return o; };
    for (const TextLayerW& l : layers) {
        Act h(R.pool(), M, C, R.bf());
        ln(l.ln1, x, h);
        Act qkv = R.linear(l.qkv, h.p, C, M, tower_rows(R));
        Act a(R.pool(), M, C, R.bf());
        if (!h16) {
            attn32(qkv.p, a.p);
        } else {
            AttnArgs g;
            g.q = qkv.at(0); g.ldq = 3 * C; g.k = qkv.at(C); g.v = qkv.at(2 * C); g.ldkv = 3 * C; g.o = a.p; g.ldo = C;
            g.n = n; g.F = 1; g.heads = heads; g.D = 64; g.Nq = T; g.Nk = T; g.mode = 1; g.scale = 0.125f; g.io_bf16 = h16;
            flash_attention(g, s);
        }
        x = R.linear(l.out, a.p, C, M, plus(x));
        ln(l.ln2, x, h);
        Act f = R.linear(l.fc1, h.p, C, M, tower_rows(R));
        text_activation(f.p, M * I, act, s, h16);
        x = R.linear(l.fc2, f.p, I, M, plus(x));
    }
    return x;
}

// the LayerNorm in front of a tower's head: `rows` rows of x at stride ldx (the class rows, or pooled fp32 rows) -> fp32 rows
void tower_head_ln(const Runner& R, const NormW& w, const float* x, int ldx, bool x_is_f32, float* out, int rows, int C, float eps) {
    if (R.h16() && !x_is_f32) layernorm_f32_out(x, ldx, w.g, w.b, out, C, rows, C, eps, R.s, R.h16());
    else layernorm(x, ldx, w.g, w.b, out, C, rows, C, eps, R.s);
}

}  // namespace

// -----------------------------------------------------------------------------------------------------
// CLIPTextModel.forward(input_ids)[0] (transformers: CLIPTextTransformer -- embeddings, pre-LN encoder layers under the causal
// mask, final_layer_norm).  fp32 rows and fp32 arithmetic whatever the context's compute mode (the linears go the way of the
// time-embedding MLP), so the same ids give the same bits in every mode.
// -----------------------------------------------------------------------------------------------------
void e2v_ctx::text_encode(const int* ids, int B, int T, float* out, hipStream_t s) {
    require_ready(TEXT);
    Runner R{this, s, false};
    R.tower = H16_NONE;                                          // tower_layers in its fp32 form: fp32 rows, the fp32 LayerNorm and activation
    const int C = cfg.text_hidden;                               // = 64 * text_heads (e2v_create refuses any other): the width tower_layers derives
    const int64_t M = (int64_t)B * T;
    Act x(pool, M, C);
    text_embed(ids, text.tok, text.pos, x.p, (int)M, T, C, s);
    x = tower_layers(R, text.layers, std::move(x), B, T, cfg.text_heads, cfg.text_intermediate, cfg.text_norm_eps, cfg.text_act,
                     [&](const float* qkv, float* a) { text_causal_attention(qkv, 3 * C, a, C, B, T, cfg.text_heads, s); });
    layernorm(x.p, C, text.ln_f.g, text.ln_f.b, out, C, (int)M, C, cfg.text_norm_eps, s);
    E2V_HIP(hipGetLastError());
}

// -----------------------------------------------------------------------------------------------------
// The frame-input metric towers (image_classify, video_classify, clip_embed below) are one runner.  A tower is a VisionTowerW, its
// sizes (TowerDims, filled from the config at the call site) and what the call site passes as lambdas: the preprocess call, the fp32
// attention kernel, and what is done with the head's rows.  Whether a class token is embedded, the LayerNorm in front of the layers
// and class-row or token-mean pooling follow from the weights (cls, pre_ln.g).
// -----------------------------------------------------------------------------------------------------
namespace {

// host tables per key (the resize tables of a tower's preprocess per (part, H, W)), at most 64 of them
template <class Key, class Plan, class Make>
const Plan& prep_cached(std::map<Key, Plan>& cache, const Key& key, Make make) {
    auto it = cache.find(key);
    if (it == cache.end()) {
        if (cache.size() >= 64) cache.clear();
        it = cache.emplace(key, make()).first;
    }
    return it->second;
}

struct TowerDims { int C, I, P, T, K, heads; float eps, head_eps; int act; };      // K: patch row length; head_eps: of the LayerNorm in front of the head

struct TowerRun {
    Runner R;                 // in the tower's own mode
    const PrepPlan& plan;
    Act tables;               // plan.words on the device
    int chunk;                // sequences per pass
    const int* tab() const { return reinterpret_cast<const int*>(tables.p); }
};

// what the three share before the first launch, in this order: the ready check, the 16-bit mode's limit on K (`k_what` names K in the
// tower's terms), the plan of this frame size and its band check, the upload of its tables, the chunk knob
TowerRun tower_begin(e2v_ctx* c, e2v_ctx::Part part, const std::string& who, const char* k_what, int K, int H, int W, int chunk_knob, hipStream_t s) {
    c->require_ready(part);
    Runner R{c, s, false};
    R.tower = c->tower_h16[part];
    E2V_REQUIRE(!R.h16() || K % 8 == 0, E2V_ESHAPE, who + ": a 16-bit tower needs " + k_what + " to be a multiple of 8");
    const PrepPlan& plan = c->prep_plan(part, H, W);
    E2V_REQUIRE(plan.band >= 1, E2V_ESHAPE, who + ": the source rows of one output row do not fit the preprocess kernel's LDS band");
    return TowerRun{R, plan, upload_plan(c->pool, plan, s), std::min(std::max(chunk_knob, 1), 4096)};      // (the plan lives in the context)
}

// One pass of ni sequences: prep(rows) fills the patch rows; the patch linear; the token rows (with the class token where the tower has
// one, through pre_ln where it has one); the layers; the class rows, or the mean over the tokens, through head_ln -- fp32 from there
// on -- and the fp32 head, whose rows [ni][head.out] go to finish.
template <class Prep, class Attn32, class Finish>
void tower_chunk(Runner& R, const VisionTowerW& w, const TowerDims& d, int ni, Prep prep, Attn32 attn32, Finish finish) {
    Pool& pool = R.pool();
    hipStream_t s = R.s;
    const int h16 = R.h16(), C = d.C, T = d.T;
    const int64_t M = (int64_t)ni * T, Mp = (int64_t)ni * (w.cls ? T - 1 : T);
    Act x(pool, M, C, R.bf());
    {
        Act rows(pool, Mp, d.K, R.bf());
        prep(rows.p);
        Act patches = R.linear(w.patch, rows.p, d.K, Mp, tower_rows(R));
        Act tok;                                                // the token rows in front of pre_ln
        if (w.pre_ln.g) tok = Act(pool, M, C, R.bf());
        float* e = w.pre_ln.g ? tok.p : x.p;
        token_embed(patches.p, w.cls, w.pos, e, ni, T, C, s, h16);
        if (w.pre_ln.g) layernorm(tok.p, C, w.pre_ln.g, w.pre_ln.b, x.p, C, (int)M, C, d.eps, s, h16);
    }
    x = tower_layers(R, w.layers, std::move(x), ni, T, d.heads, d.I, d.eps, d.act, attn32);
    Act mean;                                                   // fp32 from here on: the mean reads the 16-bit rows of a 16-bit tower
    if (!w.cls) mean = Act(pool, ni, C);
    Act pooled(pool, ni, C);
    if (w.cls) {                                                // head_ln on the class rows only (row stride T * C)
        tower_head_ln(R, w.head_ln, x.p, T * C, false, pooled.p, ni, C, d.head_eps);
    } else {
        token_mean(x.p, mean.p, ni, T, C, s, h16);
        tower_head_ln(R, w.head_ln, mean.p, C, true, pooled.p, ni, C, d.head_eps);
    }
    Act out = R.linear(w.head, pooled.p, C, ni, R.f32_rows());
    finish(out);
}

}  // namespace

Act e2v::upload_plan(Pool& pool, const PrepPlan& plan, hipStream_t s) {
    Act tables(pool, (int64_t)plan.words.size(), 1);
    E2V_HIP(hipMemcpyAsync(tables.p, plan.words.data(), plan.words.size() * sizeof(int), hipMemcpyHostToDevice, s));
    return tables;
}

const PrepPlan& e2v_ctx::prep_plan(Part tower, int H, int W) {
    return prep_cached(prep_plans, std::array<int, 3>{(int)tower, H, W}, [&] {
        if (tower == IMAGE) {                                    // ViTImageProcessor: the whole frame to S x S, no crop
            const int S = cfg.vit_image_size;
            return e2v::prep_plan(H, W, PrepWindow{S, S, 0, 0}, S, cfg.vit_patch_size, image_lut, kResizeBilinear);
        }
        if (tower == VIDEO)
            return e2v::prep_plan(H, W, video_crop(H, W, cfg.vmae_resize_edge, cfg.vmae_image_size), cfg.vmae_image_size, cfg.vmae_patch_size,
                                  video_lut, kResizeBilinear);
        return e2v::prep_plan(H, W, video_crop(H, W, vcfg.clipv_resize_edge, vcfg.clipv_image_size), vcfg.clipv_image_size,
                              vcfg.clipv_patch_size, clipv_lut, vcfg.clipv_resample);
    });
}

const std::vector<float>& e2v_ctx::de_psd_plan(int samples) {
    return prep_cached(de_psd_plans, std::array<int, 2>{samples, 0}, [&] { return e2v::de_psd_plan(samples); });
}

// -----------------------------------------------------------------------------------------------------
// ViTImageProcessor + ViTForImageClassification.forward(pixel_values).logits (transformers: ViTEmbeddings -- patch convolution,
// class token, position embeddings --, pre-LN encoder layers without a mask, the final LayerNorm, the classifier on the class row),
// then the softmax and the top-3 indices img_classify_metric takes from it (40_class_run_metrics.py:95-98).  The arithmetic is the
// TOWER's mode (e2v_set_tower_dtype; tower_layers above), fp32 by default, whatever the context's compute mode; the head is fp32
// always.  Images are walked in chunks of E2V_VIT_CHUNK (64): every kernel
// here computes a row from that row's image alone and in an order that does not depend on the row count, so the chunking does not
// show in the result.
// -----------------------------------------------------------------------------------------------------
void e2v_ctx::image_classify(const FrameSrc& src, int n, int F, int H, int W, float* logits, float* probs, int* top3, hipStream_t s) {
    static const int* const chunk_knob = knob("E2V_VIT_CHUNK", 64);
    const int P = cfg.vit_patch_size, L = cfg.vit_num_labels;
    const TowerDims d{cfg.vit_hidden, cfg.vit_intermediate, P, image_tokens(), 3 * P * P, cfg.vit_heads, cfg.vit_norm_eps, cfg.vit_norm_eps, 1};
    auto t = tower_begin(this, IMAGE, "e2v_image_classify", "3 * patch_size^2", d.K, H, W, *chunk_knob, s);
    const int h16 = t.R.h16();
    const long long total = (long long)n * F;
    for (long long i0 = 0; i0 < total; i0 += t.chunk) {
        const int ni = (int)std::min<long long>(t.chunk, total - i0);
        tower_chunk(t.R, image, d, ni,
                    [&](float* rows) { frame_preprocess(src, n, F, 1, i0, ni, t.plan, t.tab(), P, rows, "image_preprocess", s, h16); },
                    [&](const float* qkv, float* a) { image_attention(qkv, 3 * d.C, a, d.C, ni, d.T, d.heads, s); },
                    [&](const Act& lg) {
                        image_head(lg.p, lg.C, L, ni, logits ? logits + (size_t)i0 * L : nullptr, probs ? probs + (size_t)i0 * L : nullptr,
                                   top3 ? top3 + (size_t)i0 * 3 : nullptr, s);
                    });
    }
    E2V_HIP(hipGetLastError());
}

// -----------------------------------------------------------------------------------------------------
// VideoMAEImageProcessor + VideoMAEForVideoClassification.forward(pixel_values).logits (transformers: VideoMAEEmbeddings -- the
// tubelet convolution and the fixed sinusoid table --, pre-LN encoder layers without a mask, no final LayerNorm under
// use_mean_pooling, the mean over the tokens, fc_norm at nn.LayerNorm's default eps, the classifier), then the softmax and the top-3
// indices video_classify_metric takes from it (40_class_run_metrics.py:128-139).  The tower's own mode, as image_classify.
// Clips are walked in chunks of E2V_VMAE_CHUNK (16): every kernel here computes a row from that row's clip alone and in an order
// that does not depend on the row count, so the chunking does not show in the result.
// -----------------------------------------------------------------------------------------------------
void e2v_ctx::video_classify(const FrameSrc& src, int n, int F, int H, int W, float* logits, float* probs, int* top3, hipStream_t s) {
    require_ready(VIDEO);
    E2V_REQUIRE(F == cfg.vmae_num_frames, E2V_ESHAPE, "e2v_video_classify: F must be vmae_num_frames");
    static const int* const chunk_knob = knob("E2V_VMAE_CHUNK", 16);
    const int P = cfg.vmae_patch_size, ts = cfg.vmae_tubelet_size, L = cfg.vmae_num_labels;
    const TowerDims d{cfg.vmae_hidden, cfg.vmae_intermediate, P, video_tokens(), 3 * ts * P * P, cfg.vmae_heads, cfg.vmae_norm_eps,
                      1e-5f, 1};                                 // fc_norm = nn.LayerNorm(hidden): the default eps
    auto t = tower_begin(this, VIDEO, "e2v_video_classify", "3 * tubelet_size * patch_size^2", d.K, H, W, *chunk_knob, s);
    const int h16 = t.R.h16(), chunk = std::min(t.chunk, 65535 / F);
    for (int i0 = 0; i0 < n; i0 += chunk) {
        const int ni = std::min(chunk, n - i0);
        tower_chunk(t.R, video, d, ni,
                    [&](float* rows) { frame_preprocess(src, n, F, ts, (long long)i0 * F, ni * F, t.plan, t.tab(), P, rows, "video_preprocess", s, h16); },
                    [&](const float* qkv, float* a) { token_attention(qkv, 3 * d.C, a, d.C, ni, d.T, d.heads, s); },
                    [&](const Act& lg) {
                        image_head(lg.p, lg.C, L, ni, logits ? logits + (size_t)i0 * L : nullptr, probs ? probs + (size_t)i0 * L : nullptr,
                                   top3 ? top3 + (size_t)i0 * 3 : nullptr, s);
                    });
    }
    E2V_HIP(hipGetLastError());
}

// -----------------------------------------------------------------------------------------------------
// CLIPImageProcessor + CLIPVisionModelWithProjection.forward(pixel_values).image_embeds (transformers: CLIPVisionEmbeddings -- the
// patch convolution without bias, the class embedding, position embeddings --, pre_layrnorm over every token row, pre-LN encoder
// layers without a mask, post_layernorm on the class row, visual_projection without bias): what the reference's clip_score
// (40_class_run_metrics.py:20-55) normalises and multiplies.  The processor is the video classifier's crop-window preprocess with
// bicubic tables and one frame per image; the rest is image_classify with a LayerNorm in front of the layers and clipv_act.  The
// tower's own mode, as image_classify.  Images are walked in chunks of E2V_CLIPV_CHUNK (256: at B/32's 50 tokens an image a
// GEMM then sees 12800 rows, about the 64 x 197 = 12608 of the image classifier's chunk); every kernel here computes a row from
// that row's image alone and in an order that does not depend on the row count, so the chunking does not show in the result.
// -----------------------------------------------------------------------------------------------------
void e2v_ctx::clip_embed(const FrameSrc& src, int n, int F, int H, int W, float* embeds, hipStream_t s) {
    static const int* const chunk_knob = knob("E2V_CLIPV_CHUNK", 256);
    const int P = vcfg.clipv_patch_size, E = vcfg.clipv_projection_dim;
    const TowerDims d{vcfg.clipv_hidden, vcfg.clipv_intermediate, P, clipv_tokens(), 3 * P * P, vcfg.clipv_heads, vcfg.clipv_norm_eps,
                      vcfg.clipv_norm_eps, vcfg.clipv_act};
    auto t = tower_begin(this, CLIPV, "e2v_clip_embed", "3 * patch_size^2", d.K, H, W, *chunk_knob, s);
    const int h16 = t.R.h16();
    const long long total = (long long)n * F;
    for (long long i0 = 0; i0 < total; i0 += t.chunk) {
        const int ni = (int)std::min<long long>(t.chunk, total - i0);
        tower_chunk(t.R, clipv, d, ni,
                    [&](float* rows) { frame_preprocess(src, n, F, 1, i0, ni, t.plan, t.tab(), P, rows, "video_preprocess", s, h16); },
                    [&](const float* qkv, float* a) { image_attention(qkv, 3 * d.C, a, d.C, ni, d.T, d.heads, s); },
                    [&](const Act& emb) { copy_rows(emb.p, emb.C, embeds + (size_t)i0 * E, E, ni, E, s); });
    }
    E2V_HIP(hipGetLastError());
}

// -----------------------------------------------------------------------------------------------------
// myTransformer.forward in eval mode (my_autoregressive_transformer.py:151-192) and the slice its inference keeps (:383-384).
//   windows   MyEEGNet_embedding of every window (eegnet_embed, then the Linear), + the sinusoid rows (:154,161)
//   encoder   nn.TransformerEncoderLayer x L, post-LN, ReLU, no mask, no final norm (:171)
//   text      txtpredictor of the mean over the window rows (:187,190)
//   decoder   new_tgt starts as one zero row and never receives a position (:176); pass i runs the layers over rows 0 .. i under the
//             causal mask and appends the last output row (:177-181).  Under that mask rows 0 .. i - 1 come out of every layer exactly as
//             in the pass before, so pass i computes ROW i alone, against the keys and values each layer kept of the earlier rows --
//             the reference's arithmetic for that row, 1 / (i + 1) of its work; the memory's keys and values of every layer are
//             projected once per call.  Only the passes the requested tokens need are run.
//   latents   predictor of the requested token rows (:190), in the caller's layout
// fp32 rows and fp32 arithmetic whatever the context's compute mode (the linears go the way of the time-embedding MLP, no split-K:
// the runner is of the large family), and every kernel computes a row from its own clip in an order fixed by the config: a clip's bits
// depend neither on B nor on its place in the batch.
// -----------------------------------------------------------------------------------------------------
void e2v_ctx::seq2seq_latents(const EegnetArgs& eeg_in, int B, int first, int count, int layout, float* latents, float* txt_logits,
                              float* tokens, hipStream_t s) {
    require_ready(S2S);
    Runner R{this, s, false};
    const int C = scfg.s2s_d_model, H = scfg.s2s_heads, Dh = C / H, W = scfg.s2s_windows, T1 = scfg.s2s_steps + 1;
    const int feat = s2s_features(), L = scfg.s2s_txt_classes;
    const float eps = scfg.s2s_norm_eps, scale = 1.0f / std::sqrt((float)Dh);
    const bool decode = latents || tokens;
    const int passes = decode ? first + count - 1 : 0;
    const int64_t MW = (int64_t)B * W;
    auto ln = [&](const NormW& w, const float* x, int ldx, float* y, int ldy, int rows) { layernorm(x, ldx, w.g, w.b, y, ldy, rows, C, eps, s); };
    auto plus = [&](const float* r, int ldr) { LinOpt o = R.f32_rows(); o.resid = r; o.ldr = ldr; return o; };
    LinOpt relu = R.f32_rows();
    relu.relu = true;
    auto attend = [&](const float* q, long long sq, int ldq, const float* k, const float* v, long long skv, int ldkv, float* o, long long so,
                      int ldo, int Nq, int Nk, int pos0, bool causal) {
        SeqAttnArgs a;
        a.q = q; a.sq = sq; a.ldq = ldq; a.k = k; a.v = v; a.skv = skv; a.ldkv = ldkv; a.o = o; a.so = so; a.ldo = ldo;
        a.B = B; a.heads = H; a.D = Dh; a.Nq = Nq; a.Nk = Nk; a.q_pos0 = pos0; a.causal = causal ? 1 : 0; a.scale = scale;
        seq_attention(a, s);
    };

    // ---- windows -> encoder rows ----
    Act x(pool, MW, C);
    {
        Act f(pool, MW, feat);
        EegnetArgs e = eeg_in;
        e.pack = s2s.eegnet; e.out = f.p; e.B = B; e.W = W; e.C = scfg.s2s_electrodes; e.T = scfg.s2s_samples;
        e.F1 = scfg.s2s_f1; e.D = scfg.s2s_d; e.F2 = scfg.s2s_f2;
        eegnet_embed(e, s);
        Act emb = R.linear(s2s.embed, f.p, feat, MW, R.f32_rows());
        token_embed(emb.p, nullptr, s2s.pe, x.p, B, W, C, s);
    }
    for (const S2sEncLayerW& l : s2s.enc) {
        Act qkv = R.linear(l.qkv, x.p, C, MW, R.f32_rows());
        Act a(pool, MW, C);
        attend(qkv.p, (long long)W * 3 * C, 3 * C, qkv.p + C, qkv.p + 2 * C, (long long)W * 3 * C, 3 * C, a.p, (long long)W * C, C, W, W, 0, false);
        Act y = R.linear(l.out, a.p, C, MW, plus(x.p, C));
        ln(l.ln1, y.p, C, x.p, C, (int)MW);
        Act f = R.linear(l.fc1, x.p, C, MW, relu);
        y = R.linear(l.fc2, f.p, scfg.s2s_ffn, MW, plus(x.p, C));
        ln(l.ln2, y.p, C, x.p, C, (int)MW);
    }
    if (txt_logits) {
        Act mean(pool, B, C);
        token_mean(x.p, mean.p, B, W, C, s);
        Act lg = R.linear(s2s.txt, mean.p, C, B, R.f32_rows());
        copy_rows(lg.p, lg.C, txt_logits, L, B, L, s);
    }
    if (decode) {
        const int rows = passes + 1;                             // token rows this call holds
        Act tok(pool, (int64_t)B * rows, C);
        E2V_HIP(hipMemsetAsync(tok.p, 0, tok.bytes(), s));       // row 0 of every clip: torch.zeros; the others are written below
        const long long st = (long long)rows * C;                // clip stride of the token rows
        std::vector<Act> memkv, cache;                           // per layer: k | v of the memory [B W][2C], of the token rows [B rows][2C]
        for (const S2sDecLayerW& l : s2s.dec) {
            if (passes > 0) {
                memkv.push_back(R.linear(l.kv2, x.p, C, MW, R.f32_rows()));
                cache.emplace_back(pool, (int64_t)B * passes, 2 * C);
            }
        }
        for (int i = 0; i < passes; ++i) {
            const float* h = tok.p + (size_t)i * C;              // row i of every clip
            int ldh = (int)st;
            Act cur;
            for (size_t li = 0; li < s2s.dec.size(); ++li) {
                const S2sDecLayerW& l = s2s.dec[li];
                const long long sc = (long long)passes * 2 * C;
                Act qkv = R.linear(l.qkv, h, ldh, B, R.f32_rows());
                copy_rows(qkv.p + C, 3 * C, cache[li].p + (size_t)i * 2 * C, (int)sc, B, 2 * C, s);
                Act a(pool, B, C);
                attend(qkv.p, 3 * C, 3 * C, cache[li].p, cache[li].p + C, sc, 2 * C, a.p, C, C, 1, i + 1, i, true);
                Act y = R.linear(l.out, a.p, C, B, plus(h, ldh));
                Act h1(pool, B, C);
                ln(l.ln1, y.p, C, h1.p, C, B);
                Act q2 = R.linear(l.q2, h1.p, C, B, R.f32_rows());
                attend(q2.p, C, C, memkv[li].p, memkv[li].p + C, (long long)W * 2 * C, 2 * C, a.p, C, C, 1, W, 0, false);
                y = R.linear(l.out2, a.p, C, B, plus(h1.p, C));
                Act h2(pool, B, C);
                ln(l.ln2, y.p, C, h2.p, C, B);
                Act f = R.linear(l.fc1, h2.p, C, B, relu);
                y = R.linear(l.fc2, f.p, scfg.s2s_ffn, B, plus(h2.p, C));
                if (li + 1 == s2s.dec.size()) {                  // the last layer's row IS the appended token
                    ln(l.ln3, y.p, C, tok.p + (size_t)(i + 1) * C, (int)st, B);
                } else {
                    cur = Act(pool, B, C);
                    ln(l.ln3, y.p, C, cur.p, C, B);
                    h = cur.p; ldh = C;
                }
            }
        }
        if (tokens) copy_rows(tok.p, (int)st, tokens, T1 * C, B, rows * C, s);
        if (latents) {
            Act sel(pool, (int64_t)B * count, C);
            copy_rows(tok.p + (size_t)first * C, (int)st, sel.p, count * C, B, count * C, s);
            Act lat = R.linear(s2s.pred, sel.p, C, (int64_t)B * count, R.f32_rows());
            if (layout == 0) E2V_HIP(hipMemcpyAsync(latents, lat.p, lat.bytes(), hipMemcpyDeviceToDevice, s));
            else seq_latents_bcfhw(lat.p, latents, B, count, scfg.s2s_latent_channels, scfg.s2s_latent_h * scfg.s2s_latent_w, s);
        }
    }
    E2V_HIP(hipGetLastError());
}

// -----------------------------------------------------------------------------------------------------
// glfnet.forward in eval mode (EEG2Video/models/models.py:352-373): the global shallownet over all electrodes and the occipital one
// over electrodes occ_first .. occ_first + occ_count - 1 of the same clip (read through the electrode stride, no gathered copy), each
// the ShallowNet kernel and its linear; the head over the concatenated embeddings.  fp32 rows and fp32 arithmetic whatever the
// context's compute mode, every value in an order fixed by the config: a clip's bits depend neither on B nor on its place in the batch.
// -----------------------------------------------------------------------------------------------------
namespace {
void glm_finish(Runner& R, const LinW& head, const Act& a, const Act& b, int E, int L, int B, float* logits, float* features, int* labels) {
    Act feat(R.pool(), B, 2 * E);
    copy_rows(a.p, a.C, feat.p, 2 * E, B, E, R.s);
    copy_rows(b.p, b.C, feat.p + E, 2 * E, B, E, R.s);
    Act lg = R.linear(head, feat.p, 2 * E, B, R.f32_rows());
    glm_outputs(lg.p, lg.C, feat.p, 2 * E, L, B, logits, features, labels, R.s);
}
}  // namespace

void e2v_ctx::glmnet_raw(const ShallowArgs& eeg_in, int B, float* logits, float* features, int* labels, hipStream_t s) {
    require_ready(GLM);
    Runner R{this, s, false};
    const int E = gcfg.glm_emb, feat = glm_raw_features();
    auto net = [&](const GlmNetW& w, int first, int count) {
        Act maps(pool, B, feat);
        ShallowArgs a = eeg_in;
        a.eeg += (long long)first * a.channel_stride;
        if (a.mean) { a.mean += (size_t)first * gcfg.glm_samples; a.scale += (size_t)first * gcfg.glm_samples; }
        a.w = w.fold;
        a.c = w.fold + shallownet_fold_floats(count, gcfg.glm_filters, gcfg.glm_taps) - shallownet_fold_floats(0, gcfg.glm_filters, 0);      // (the constants close the pack)
        a.out = maps.p; a.ldo = feat;
        a.B = B; a.C = count; a.T = gcfg.glm_samples; a.F = gcfg.glm_filters; a.K = gcfg.glm_taps; a.P = gcfg.glm_pool; a.S = gcfg.glm_pool_stride;
        shallownet(a, s);
        return R.linear(w.out, maps.p, feat, B, R.f32_rows());
    };
    Act g = net(glm.raw_global, 0, gcfg.glm_electrodes);
    Act o = net(glm.raw_occ, gcfg.glm_occ_first, gcfg.glm_occ_count);
    glm_finish(R, glm.raw_head, g, o, E, gcfg.glm_raw_out, B, logits, features, labels);
    E2V_HIP(hipGetLastError());
}

// glfnet_mlp.forward (EEG2Video/models/models.py:375-413): two mlpnets (Linear, erf GELU, Linear, GELU, Linear) over the flattened
// [electrodes][bands] features and over their occipital rows, the same head.  The rows are copied into K-padded buffers of their own
// first: 310 is no multiple of 4, and the occipital rows start 1000 bytes into a row.
void e2v_ctx::glmnet_mlp(const float* de, int B, float* logits, float* features, int* labels, hipStream_t s) {
    require_ready(GLM);
    Runner R{this, s, false};
    const int E = gcfg.glm_emb, bands = gcfg.glm_bands, row = gcfg.glm_electrodes * bands;
    auto net = [&](const GlmMlpW& w, int first) {
        const int inp = w.l1.in;
        Act x(pool, B, inp);
        if (inp != w.in) E2V_HIP(hipMemsetAsync(x.p, 0, x.bytes(), s));
        copy_rows(de + (size_t)first * bands, row, x.p, inp, B, w.in, s);
        Act h1 = R.linear(w.l1, x.p, inp, B, R.f32_rows());
        text_activation(h1.p, (long long)B * h1.C, 1, s);
        Act h2 = R.linear(w.l2, h1.p, h1.C, B, R.f32_rows());
        text_activation(h2.p, (long long)B * h2.C, 1, s);
        return R.linear(w.l3, h2.p, h2.C, B, R.f32_rows());
    };
    Act g = net(glm.mlp_global, 0);
    Act o = net(glm.mlp_occ, gcfg.glm_occ_first);
    glm_finish(R, glm.mlp_head, g, o, E, gcfg.glm_mlp_out, B, logits, features, labels);
    E2V_HIP(hipGetLastError());
}
