// clip_vision.hpp — what turns a picture into IP-Adapter image tokens (stable-diffusion.cpp:2164-2215): the CLIP preprocessing tables, the CLIP vision tower and the
// Resampler of the "plus" adapters, as ggml graphs on the context's backend.
//
// Node-for-node restatement of src/model/te/clip.hpp:212-237 (CLIPVisionEmbeddings::forward), :364-391 (CLIPVisionModel::forward), :447-463
// (CLIPVisionModelProjection::forward) and src/model/adapter/ip_adapter.hpp:68-113 (Resampler::forward); the encoder layers are the text tower's ClipLayer /
// MultiheadAttention (text_encoders.hpp) unchanged.  The preprocessing restates src/core/util.cpp:695-758 and the default (Nearest) mode of sd::ops::interpolate,
// src/core/tensor.hpp:1224-1299.
#pragma once
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "text_encoders.hpp"

namespace sdmi {

struct ClipVisionConfig {  // clip.hpp:332-362, :426-445
    ClipVersion version       = CLIP_VIT_L_14;
    int64_t num_channels      = 3;
    int64_t patch_size        = 14;
    int64_t image_size        = 224;
    int64_t hidden_size       = 1024;
    int64_t intermediate_size = 4096;
    int64_t n_head            = 16;
    int64_t n_layer           = 24;
    int64_t projection_dim    = 768;
    bool use_gelu             = true;  // clip.hpp:21-25: tanh-GELU for d_model 1024 / 1280, quick-GELU otherwise (so bigG's 1664 gets quick-GELU)

    int64_t num_patches() const { return (image_size / patch_size) * (image_size / patch_size); }
    int64_t num_positions() const { return num_patches() + 1; }
    static bool gelu_rule(int64_t d_model) { return d_model == 1024 || d_model == 1280; }
    static ClipVisionConfig vit_l() { return ClipVisionConfig(); }
    static ClipVisionConfig vit_h() {
        ClipVisionConfig c;
        c.version = CLIP_VIT_H_14;
        c.hidden_size = 1280, c.intermediate_size = 5120, c.n_head = 16, c.n_layer = 32, c.projection_dim = 1024;
        c.use_gelu = gelu_rule(c.hidden_size);
        return c;
    }
    static ClipVisionConfig vit_bigg() {  // CLIPVisionModelProjection leaves projection_dim at its default for bigG (clip.hpp:439-441)
        ClipVisionConfig c;
        c.version = CLIP_VIT_BIGG_14;
        c.hidden_size = 1664, c.intermediate_size = 8192, c.n_head = 16, c.n_layer = 48;
        c.use_gelu = gelu_rule(c.hidden_size);
        return c;
    }
    // same topology at test width (intermediate = 2 hidden like ClipTextConfig::tiny)
    static ClipVisionConfig tiny(int64_t hidden, int64_t heads, int64_t layers, int64_t image_size, int64_t patch_size, int64_t proj) {
        ClipVisionConfig c;
        c.hidden_size = hidden, c.intermediate_size = 2 * hidden, c.n_head = heads, c.n_layer = layers, c.image_size = image_size, c.patch_size = patch_size;
        c.projection_dim = proj;
        c.use_gelu       = gelu_rule(hidden);
        return c;
    }
    ClipTextConfig layer_config() const {  // what ClipLayer::init reads
        ClipTextConfig t;
        t.hidden_size = hidden_size, t.intermediate_size = intermediate_size, t.n_head = n_head, t.n_layer = n_layer, t.use_gelu = use_gelu;
        return t;
    }
};

struct ClipVisionModel {  // CLIPVisionModelProjection: vision_model + visual_projection
    ClipVisionConfig cfg;
    ggml_tensor *patch_embedding = nullptr, *class_embedding = nullptr, *position_embedding = nullptr, *visual_projection = nullptr;
    LayerNorm pre_ln, post_ln;
    std::vector<ClipLayer> layers;

    void init(ParamStore& ps, const std::string& prefix, const ClipVisionConfig& c) {
        cfg                   = c;
        const std::string vm  = prefix + "vision_model.";
        // clip.hpp:189-197: f16 patch weight, f32 class embedding and position table
        patch_embedding    = ps.add(vm + "embeddings.patch_embedding.weight", GGML_TYPE_F16, {c.patch_size, c.patch_size, c.num_channels, c.hidden_size}, InitKind::WEIGHT,
                                    c.num_channels * c.patch_size * c.patch_size);
        class_embedding    = ps.add(vm + "embeddings.class_embedding", GGML_TYPE_F32, {c.hidden_size}, InitKind::BIAS, c.hidden_size);
        position_embedding = ps.add(vm + "embeddings.position_embedding.weight", GGML_TYPE_F32, {c.hidden_size, c.num_positions()}, InitKind::BIAS, c.hidden_size);
        pre_ln.init(ps, vm + "pre_layernorm.", c.hidden_size);
        const ClipTextConfig lc = c.layer_config();
        layers.resize(c.n_layer);
        for (int64_t i = 0; i < c.n_layer; ++i) layers[i].init(ps, vm + "encoder.layers." + std::to_string(i) + ".", lc);
        post_ln.init(ps, vm + "post_layernorm.", c.hidden_size);
        // CLIPProjection (clip.hpp:394-424, transpose_weight false): ne = [in = hidden, out = projection_dim], f32 unless the file says otherwise
        visual_projection = ps.add(prefix + "visual_projection.weight", GGML_TYPE_F32, {c.hidden_size, c.projection_dim}, InitKind::WEIGHT, c.hidden_size);
    }

    // CLIPVisionEmbeddings::forward (clip.hpp:212-237): pixel_values [S, S, 3, N] -> [hidden, num_positions, N]
    ggml_tensor* embeddings(GraphCtx& g, ggml_tensor* pixel_values) const {
        ggml_context* c   = g.ctx;
        const int64_t N   = pixel_values->ne[3], E = cfg.hidden_size, np = cfg.num_patches();
        const int P       = (int)cfg.patch_size;
        ggml_tensor* pe   = ext_conv_2d(c, pixel_values, patch_embedding, nullptr, P, P, 0, 0, 1, 1, g.conv_direct);  // [G, G, E, N]
        pe                = ggml_reshape_3d(c, pe, np, E, N);
        pe                = ggml_cont(c, ggml_permute(c, pe, 1, 0, 2, 3));  // [E, np, N]
        pe                = ggml_reshape_4d(c, pe, 1, E, np, N);
        ggml_tensor* cls  = ggml_new_tensor_2d(c, GGML_TYPE_F32, E, N);
        cls               = ggml_repeat(c, class_embedding, cls);
        cls               = ggml_reshape_4d(c, cls, 1, E, 1, N);
        ggml_tensor* x    = ggml_concat(c, cls, pe, 2);  // [1, E, np + 1, N]
        x                 = ggml_reshape_3d(c, x, E, cfg.num_positions(), N);
        return ggml_add(c, x, position_embedding);
    }

    // CLIPVisionModelProjection::forward over CLIPVisionModel::forward: pooled [projection_dim, N], else the hidden state BEFORE post_layernorm [hidden, num_positions, N]
    ggml_tensor* forward(GraphCtx& g, ggml_tensor* pixel_values, bool return_pooled, int clip_skip) const {
        ggml_context* c = g.ctx;
        ggml_tensor* x  = embeddings(g, pixel_values);
        x               = pre_ln.forward(g, x);
        // CLIPEncoder::forward (clip.hpp:96-122); the vision model hands clip_skip through whether pooled or not (:377)
        // (restated with its loop form: clip_skip = n_layer + 1 runs no layer, a larger one never meets the break and runs them all)
        int layer_idx = (int)cfg.n_layer - 1;
        if (clip_skip > 0) layer_idx = (int)cfg.n_layer - clip_skip;
        for (int i = 0; i < (int)cfg.n_layer; ++i) {
            if (i == layer_idx + 1) break;
            x = layers[i].forward(g, x, nullptr);
        }
        if (!return_pooled) return x;  // clip.hpp:389 (post_layernorm is built there too, but nothing reads it: not part of the graph)
        x                   = post_ln.forward(g, x);
        ggml_tensor* pooled = ggml_cont(c, ggml_view_2d(c, x, x->ne[0], x->ne[2], x->nb[2], 0));  // token 0 of every image
        return ext_linear(c, pooled, visual_projection, nullptr);
    }
};

// Resampler — ip_adapter.hpp:34-113 (dim_head 64, heads = dim / 64)
struct Resampler {
    int64_t dim = 0, depth = 0, num_queries = 0, embed_dim = 0, output_dim = 0, ff_inner = 0, heads = 0;
    ggml_tensor* latents = nullptr;
    Linear proj_in, proj_out;
    LayerNorm norm_out;
    struct Layer {
        LayerNorm norm1, norm2, ff_norm;
        Linear to_q, to_kv, to_out, ff_fc1, ff_fc2;
    };
    std::vector<Layer> layers;

    void init(ParamStore& ps, const std::string& prefix, int64_t dim_, int64_t depth_, int64_t num_queries_, int64_t embed_dim_, int64_t output_dim_, int64_t ff_inner_) {
        dim = dim_, depth = depth_, num_queries = num_queries_, embed_dim = embed_dim_, output_dim = output_dim_, ff_inner = ff_inner_;
        heads   = dim / 64;
        latents = ps.add(prefix + "latents", GGML_TYPE_F32, {dim, num_queries, 1}, InitKind::BIAS, dim);
        proj_in.init(ps, prefix + "proj_in.", embed_dim, dim);
        proj_out.init(ps, prefix + "proj_out.", dim, output_dim);
        norm_out.init(ps, prefix + "norm_out.", output_dim);
        layers.resize(depth);
        for (int64_t i = 0; i < depth; ++i) {
            const std::string p = prefix + "layers." + std::to_string(i);
            Layer& l            = layers[i];
            l.norm1.init(ps, p + ".0.norm1.", dim);
            l.norm2.init(ps, p + ".0.norm2.", dim);
            l.to_q.init(ps, p + ".0.to_q.", dim, dim, false);
            l.to_kv.init(ps, p + ".0.to_kv.", dim, dim * 2, false);
            l.to_out.init(ps, p + ".0.to_out.", dim, dim, false);
            l.ff_norm.init(ps, p + ".1.0.", dim);
            l.ff_fc1.init(ps, p + ".1.1.", dim, ff_inner, false);
            l.ff_fc2.init(ps, p + ".1.3.", ff_inner, dim, false);
        }
    }

    // image_embeds [embed_dim, n_tok, N] -> [output_dim, num_queries, N]
    ggml_tensor* forward(GraphCtx& g, ggml_tensor* image_embeds) const {
        ggml_context* c  = g.ctx;
        const int64_t N  = image_embeds->ne[2];
        ggml_tensor* x   = proj_in.forward(g, image_embeds);
        ggml_tensor* lat = latents;
        GraphCtx gm      = g;  // ip_adapter.hpp:96 passes flash_attn = false: the manual attention path whatever the context's setting
        gm.flash_attn    = false;
        if (N > 1) lat = ggml_repeat(c, lat, ggml_new_tensor_3d(c, GGML_TYPE_F32, dim, num_queries, N));
        for (const Layer& l : layers) {
            ggml_tensor* xn    = l.norm1.forward(g, x);
            ggml_tensor* ln    = l.norm2.forward(g, lat);
            ggml_tensor* q     = l.to_q.forward(g, ln);
            ggml_tensor* kv_in = ggml_concat(c, xn, ln, 1);
            ggml_tensor* kv    = l.to_kv.forward(g, kv_in);
            const int64_t L    = kv->ne[1];
            ggml_tensor* k     = ggml_cont(c, ggml_view_3d(c, kv, dim, L, N, kv->nb[1], kv->nb[2], 0));
            ggml_tensor* v     = ggml_cont(c, ggml_view_3d(c, kv, dim, L, N, kv->nb[1], kv->nb[2], dim * kv->nb[0]));
            ggml_tensor* attn  = ext_attention(gm, q, k, v, heads);
            attn               = l.to_out.forward(g, attn);
            lat                = ggml_add(c, lat, attn);
            ggml_tensor* h     = l.ff_norm.forward(g, lat);
            h                  = l.ff_fc1.forward(g, h);
            h                  = ggml_gelu_erf(c, h);
            h                  = l.ff_fc2.forward(g, h);
            lat                = ggml_add(c, lat, h);
        }
        lat = proj_out.forward(g, lat);
        return norm_out.forward(g, lat);
    }
};

// ---- clip_preprocess (util.cpp:725-758) as two source-index tables: output pixel (x, y) of the S x S crop reads source pixel (xi[x], yi[y]) ----
// scale = the larger of S / w and S / h in f32; the resized extents are (int64)(scale * extent), truncated; the resize is sd::ops::interpolate's default Nearest,
// src = dst * in / out in integers (tensor.hpp:1292); the crop offsets are max((resized - S) / 2, 0).  Where f32 rounding leaves a resized extent one short of S
// (scale * extent just under S) the reference reads behind its resized tensor; here that last index takes the last source pixel.
inline void clip_preprocess_tables(int w, int h, int S, std::vector<int32_t>& xi, std::vector<int32_t>& yi) {
    const float width_scale = (float)S / (float)w, height_scale = (float)S / (float)h;
    const float scale       = std::fmax(width_scale, height_scale);
    const int64_t rw = (int64_t)(scale * (float)w), rh = (int64_t)(scale * (float)h);
    const int64_t h_off = std::max<int64_t>((rh - S) / 2, 0), w_off = std::max<int64_t>((rw - S) / 2, 0);
    xi.resize(S);
    yi.resize(S);
    for (int64_t x = 0; x < S; ++x) xi[x] = (int32_t)std::min<int64_t>(rw > 0 ? (x + w_off) * w / rw : 0, w - 1);
    for (int64_t y = 0; y < S; ++y) yi[y] = (int32_t)std::min<int64_t>(rh > 0 ? (y + h_off) * h / rh : 0, h - 1);
}

// host restatement of the kernel (backends without the export: the CPU oracle of the tests); images [n][h][w][3] u8 -> out [S, S, 3, n]
inline void clip_preprocess_host(const uint8_t* images, int w, int h, int64_t n, int S, const std::vector<int32_t>& xi, const std::vector<int32_t>& yi, float* out) {
    static const float means[3] = {0.48145466f, 0.4578275f, 0.40821073f}, stds[3] = {0.26862954f, 0.26130258f, 0.27577711f};
    for (int64_t b = 0; b < n; ++b)
        for (int c = 0; c < 3; ++c)
            for (int y = 0; y < S; ++y)
                for (int x = 0; x < S; ++x) {
                    volatile float v = (float)images[((b * h + yi[y]) * (int64_t)w + xi[x]) * 3 + c];
                    v                = v / 255.f;
                    v                = std::min(std::max((float)v, 0.f), 1.f);
                    volatile float d = v - means[c];
                    out[((b * 3 + c) * (int64_t)S + y) * S + x] = d / stds[c];
                }
}

}  // namespace sdmi
