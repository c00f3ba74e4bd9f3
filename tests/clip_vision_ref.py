"""References for the CLIP vision tower, the Resampler and the CLIP preprocessing (tests/test_clip_vision_cpu.py, tests/test_gpu_clip_vision.py).

  clip_preprocess      NumPy restatement of the reference's sd_image_to_tensor + clip_preprocess (src/core/util.cpp:695-758) with the default Nearest mode of
                       sd::ops::interpolate (src/core/tensor.hpp:1279-1299), float32 arithmetic throughout; `mutant` switches one step to a plausible wrong version
                       (the self-checks of the CPU suite show that each of them changes the output)
  tower / resampler / image_proj    PyTorch float64 on the engine's own parameter tensors (Engine.get_tensor), so the stored f16 roundings are shared
  patch_embed          NumPy CLIPVisionEmbeddings on integer data (exact in f16 x f16 -> f32)
"""
import numpy as np

MEANS = np.array([0.48145466, 0.4578275, 0.40821073], np.float32)  # util.cpp:722
STDS = np.array([0.26862954, 0.26130258, 0.27577711], np.float32)  # util.cpp:723


def preprocess_tables(w, h, S, mutant=None):
    """(xi, yi): output pixel (x, y) of the S x S crop reads source pixel (xi[x], yi[y])."""
    f = np.float32
    width_scale = f(S) / f(w)   # util.cpp:731
    height_scale = f(S) / f(h)  # :732
    scale = min(width_scale, height_scale) if mutant == "min_ratio" else max(width_scale, height_scale)  # :733 fmax
    if mutant == "round_extent":
        rw, rh = int(np.rint(f(scale * f(w)))), int(np.rint(f(scale * f(h))))
    else:
        rw, rh = int(f(scale * f(w))), int(f(scale * f(h)))  # :735-736: static_cast<int64_t> truncates
    if mutant == "ceil_offset":
        h_off, w_off = max(-((S - rh) // 2), 0), max(-((S - rw) // 2), 0)  # (rounds the half up)
    else:
        h_off, w_off = max(int((rh - S) / 2), 0), max(int((rw - S) / 2), 0)  # :742-743 (C++ integer division truncates toward zero)
    # tensor.hpp:1292: input_coord = output_coord * input_extent / output_extent in int64; the crop (:746-752) shifts the output coordinate.  Where f32 rounding leaves a
    # resized extent one short of S the reference indexes behind its resized tensor; the engine documents that it takes the last source pixel there
    xi = np.array([min((x + w_off) * w // rw if rw > 0 else 0, w - 1) for x in range(S)], np.int64)
    yi = np.array([min((y + h_off) * h // rh if rh > 0 else 0, h - 1) for y in range(S)], np.int64)
    return xi, yi


def clip_preprocess(images, S, mutant=None):
    """images [n, H, W, 3] uint8 -> pixel values [n, 3, S, S] float32."""
    img = np.asarray(images)
    if img.ndim == 3:
        img = img[None]
    n, h, w, _ = img.shape
    xi, yi = preprocess_tables(w, h, S, mutant)
    v = img[:, yi][:, :, xi].astype(np.float32) / np.float32(255.0)  # ggml_extend.hpp:188-194: value /= 255.f       [n, S, S, 3]
    means = MEANS[[2, 1, 0]] if mutant == "swap_means" else MEANS
    if mutant == "clamp_after":
        out = np.clip((v - means) / STDS, np.float32(0), np.float32(1))
    else:
        v = np.clip(v, np.float32(0), np.float32(1))  # util.cpp:754
        out = (v - means) / STDS                      # :757, two float32 operations
    return np.ascontiguousarray(out.astype(np.float32).transpose(0, 3, 1, 2))


def patch_embed(px, w, cls, pos, P):
    """px [n, 3, S, S], w [E, 3, P, P], cls [E], pos [np + 1, E] -> [n, np + 1, E] in float64 (clip.hpp:212-237)."""
    px = np.asarray(px, np.float64)
    n, _, S, _ = px.shape
    G = S // P
    E = w.shape[0]
    patches = px.reshape(n, 3, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(n, G * G, 3 * P * P)  # patch p = gx + G * gy, k = kx + P * (ky + P * c)
    y = patches @ np.asarray(w, np.float64).reshape(E, -1).T
    x = np.concatenate([np.broadcast_to(np.asarray(cls, np.float64), (n, 1, E)), y], axis=1)
    return x + np.asarray(pos, np.float64)


# ---------------------------------------------------------------------------------------------------- torch float64
def _t(a):
    import torch

    return torch.from_numpy(np.asarray(a, np.float64))


def _ln(x, w, b, eps=1e-5):
    import torch

    return torch.nn.functional.layer_norm(x, (x.shape[-1],), _t(w), _t(b), eps)


def _attention(q, k, v, heads):
    """q [n, Lq, C], k / v [n, Lk, C] -> [n, Lq, C]"""
    import torch

    n, Lq, Cq = q.shape
    d = Cq // heads
    qh = q.reshape(n, Lq, heads, d).transpose(1, 2)
    kh = k.reshape(n, -1, heads, d).transpose(1, 2)
    vh = v.reshape(n, -1, heads, d).transpose(1, 2)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / np.sqrt(d), dim=-1)
    return (p @ vh).transpose(1, 2).reshape(n, Lq, Cq)


def _act(x, use_gelu):
    import torch

    return torch.nn.functional.gelu(x, approximate="tanh") if use_gelu else x * torch.sigmoid(1.702 * x)  # ggml_gelu (tanh form) / ggml_gelu_quick


def layers_run(n_layer, clip_skip):
    """CLIPEncoder::forward (clip.hpp:102-112): `break` at i == layer_idx + 1 with layer_idx = n_layer - clip_skip for clip_skip > 0; an index below 0 is never met"""
    if clip_skip <= 0:
        return n_layer
    stop = n_layer - clip_skip + 1
    return n_layer if stop < 0 else min(n_layer, stop)


def tower(engine, px, return_pooled, clip_skip, prefix="clip_vision."):
    """CLIPVisionModelProjection::forward in float64 on the engine's parameters.  px [n, 3, S, S] -> pooled [n, proj] or hidden state [n, positions, hidden]."""
    import torch

    info = engine.clip_vision_info()
    g = lambda name: engine.get_tensor(prefix + name)
    vm = "vision_model."
    P, E, heads, L = info["patch_size"], info["hidden_size"], info["n_head"], info["n_layer"]
    pxh = np.asarray(px, np.float32).astype(np.float16)  # the im2col matrix of the conv is f16 on every route
    x = _t(patch_embed(pxh, g(vm + "embeddings.patch_embedding.weight"), g(vm + "embeddings.class_embedding"), g(vm + "embeddings.position_embedding.weight"), P))
    x = _ln(x, g(vm + "pre_layernorm.weight"), g(vm + "pre_layernorm.bias"))
    for i in range(layers_run(L, clip_skip)):
        p = f"{vm}encoder.layers.{i}."
        lin = lambda h, nm: h @ _t(g(p + nm + ".weight")).T + _t(g(p + nm + ".bias"))
        h = _ln(x, g(p + "layer_norm1.weight"), g(p + "layer_norm1.bias"))
        a = _attention(lin(h, "self_attn.q_proj"), lin(h, "self_attn.k_proj"), lin(h, "self_attn.v_proj"), heads)
        x = x + lin(a, "self_attn.out_proj")
        h = _ln(x, g(p + "layer_norm2.weight"), g(p + "layer_norm2.bias"))
        x = x + lin(_act(lin(h, "mlp.fc1"), bool(info["use_gelu"])), "mlp.fc2")
    if not return_pooled:
        return x.numpy()  # clip.hpp:389: the state before post_layernorm
    x = _ln(x, g(vm + "post_layernorm.weight"), g(vm + "post_layernorm.bias"))
    return (x[:, 0] @ _t(g("visual_projection.weight")).T).numpy()


def resampler(engine, embeds, depth, prefix="ip_adapter.image_proj."):
    """Resampler::forward (ip_adapter.hpp:68-113) in float64, exact-erf GELU.  embeds [n, n_tok, embed_dim] -> [n, num_queries, output_dim]."""
    import torch

    g = lambda name: _t(engine.get_tensor(prefix + name))
    e = _t(embeds)
    n = e.shape[0]
    x = e @ g("proj_in.weight").T + g("proj_in.bias")
    lat = g("latents").reshape(1, -1, x.shape[-1]).repeat(n, 1, 1)
    dim = x.shape[-1]
    heads = dim // 64
    for i in range(depth):
        p = f"layers.{i}."
        xn = torch.nn.functional.layer_norm(x, (dim,), g(p + "0.norm1.weight"), g(p + "0.norm1.bias"), 1e-5)
        ln = torch.nn.functional.layer_norm(lat, (dim,), g(p + "0.norm2.weight"), g(p + "0.norm2.bias"), 1e-5)
        q = ln @ g(p + "0.to_q.weight").T
        kv = torch.cat([xn, ln], dim=1) @ g(p + "0.to_kv.weight").T
        a = _attention(q, kv[..., :dim], kv[..., dim:], heads)
        lat = lat + a @ g(p + "0.to_out.weight").T
        h = torch.nn.functional.layer_norm(lat, (dim,), g(p + "1.0.weight"), g(p + "1.0.bias"), 1e-5)
        h = torch.nn.functional.gelu(h @ g(p + "1.1.weight").T) @ g(p + "1.3.weight").T
        lat = lat + h
    out = lat @ g("proj_out.weight").T + g("proj_out.bias")
    return torch.nn.functional.layer_norm(out, (out.shape[-1],), g("norm_out.weight"), g("norm_out.bias"), 1e-5).numpy()


def image_proj(engine, embeds, num_tokens, prefix="ip_adapter.image_proj."):
    """ImageProjModel::forward (ip_adapter.hpp:22-31) in float64.  embeds [n, clip_dim] -> [n, num_tokens, ctx_dim]."""
    import torch

    g = lambda name: _t(engine.get_tensor(prefix + name))
    x = _t(embeds) @ g("proj.weight").T + g("proj.bias")
    x = x.reshape(x.shape[0], num_tokens, -1)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g("norm.weight"), g("norm.bias"), 1e-5).numpy()


def gelu_erf(x):
    import torch

    t = _t(x)
    return (0.5 * t * (1.0 + torch.erf(t / np.sqrt(2.0)))).numpy()


def gelu_tanh(x):
    t = np.asarray(x, np.float64)
    return 0.5 * t * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (t + 0.044715 * t ** 3)))


def rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
