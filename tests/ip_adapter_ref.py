"""NumPy restatement of the IP-Adapter pieces (block.hpp:380-389, ip_adapter.hpp:10-32) for the tests.

  exact           the decoupled cross-attention in float64: softmax(scale q k^T) v + ip_scale * softmax(scale q k_ip^T) v_ip
  fused_model     the operand rounding k_flash_short_ip documents: Q as f16, K and K_ip as f16(f16(k) * scale * log2e), two one-pass softmaxes,
                  P_txt / sum_txt and ip_scale * P_ip / sum_ip each rounded to f16, V and V_ip as f16, one f32 accumulator
  plain_model     the same on the plain-node route: two launch_flash_attn launches (k_flash_short for the text keys, the tile kernel for the 1 .. 32 image
                  keys), each result an f32 tensor, SCALE, ADD
  image_proj      ImageProjModel: Linear(clip_dim -> num_tokens * ctx_dim) + bias, reshape, LayerNorm over ctx_dim (eps 1e-5)
  ip_key_of / ip_key_masked   which image key an accumulator register of a lane holds, and whether its initial value masks it (the kernel's index logic)
All attention functions take q [HN, Lq, d], k / v [HN, Lk, d], k_ip / v_ip [HN, Lk_ip, d]."""
import numpy as np

import attn_scores as AS


def exact(q, k, v, k_ip, v_ip, scale, ip_scale):
    return AS.exact(q, k, v, scale) + float(ip_scale) * AS.exact(q, k_ip, v_ip, scale)


def _scaled_k16(k, scale):
    return AS.f16r(np.asarray(k, np.float32).astype(np.float16).astype(np.float32) * np.float32(scale * AS.LOG2E))


def fused_model(q, k, v, k_ip, v_ip, scale, ip_scale):
    q16 = AS.f16r(q)
    out = np.zeros(q16.shape[:-1] + (v.shape[-1],))
    for kk, vv, w in ((k, v, 1.0), (k_ip, v_ip, float(np.float32(ip_scale)))):
        s = q16 @ _scaled_k16(kk, scale).transpose(0, 2, 1)
        p = np.exp2(s - s.max(-1, keepdims=True))
        p = AS.f16r(p * (w / p.sum(-1, keepdims=True)))
        out += p @ AS.f16r(vv)
    return out


def _plain_attention(q, k, v, scale):
    """one FLASH_ATTN_EXT node on launch_flash_attn: k_flash_short for 64 < Lk <= 96 at d <= 64, d % 8 == 0; else the tile kernel (the max slot at d = 40)"""
    d, Lk = q.shape[-1], k.shape[-2]
    if 64 < Lk <= 96 and d <= 64 and d % 8 == 0:
        return AS.onepass_model(q, k, v, scale)
    return AS.deferred_model(AS.f16r(q), k, v, scale, mslot=AS.uses_max_slot(d, Lk, fast=d % 8 == 0))[0]


def plain_model(q, k, v, k_ip, v_ip, scale, ip_scale):
    a = _plain_attention(q, k, v, scale).astype(np.float32)
    b = _plain_attention(q, k_ip, v_ip, scale).astype(np.float32)
    return (a + b * np.float32(ip_scale)).astype(np.float64)


def heads_to_tokens(o, H):
    """[N * H, Lq, d] (head index n * H + h) -> [N, Lq, H * d]: the layout behind FLASH_ATTN_EXT -> VIEW -> CONT -> RESHAPE"""
    HN, Lq, d = o.shape
    return o.reshape(HN // H, H, Lq, d).transpose(0, 2, 1, 3).reshape(HN // H, Lq, H * d)


def image_proj(embeds, proj_w, proj_b, norm_w, norm_b, num_tokens, eps=1e-5):
    """embeds [n, clip_dim]; proj_w [num_tokens * ctx_dim, clip_dim]; -> [n, num_tokens, ctx_dim] in float64"""
    e = np.asarray(embeds, np.float64)
    x = e @ np.asarray(proj_w, np.float64).T + np.asarray(proj_b, np.float64)
    x = x.reshape(e.shape[0], num_tokens, -1)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * np.asarray(norm_w, np.float64) + np.asarray(norm_b, np.float64)


# ---- k_flash_short_ip index logic: the 32x32 MFMA accumulator of S^T = K Q^T.  Lane l holds query (l & 31); register r of the image block holds image key
# (r & 3) + 8 * (r >> 2) + 4 * (l >> 5); the block's accumulator starts at -inf for keys >= Lk_ip and at 0 otherwise
def ip_key_of(lane, r):
    return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)


def ip_key_masked(lane, r, lk_ip):
    return ip_key_of(lane, r) >= lk_ip


def ip_pv_slot(lane, r):
    """(P V k-step t, element j of its A fragment) register r is packed into: pi[t][j] = si[t * 8 + j]"""
    return r >> 3, r & 7
