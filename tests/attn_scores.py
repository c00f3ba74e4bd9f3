"""Attention inputs whose scores MOVE the running max, and NumPy models of what the attention kernels do with them.

Standard-normal Q / K scaled by 1/sqrt(d) give scores with a standard deviation of ~1.44 log2 units: after the first key tile the deferred
running max of k_flash_attn (it moves only when a tile's max exceeds it by more than FA_THR = 8 log2 units) never moves again, so the
accumulator rescale, the `l_run` scale, the max-slot rewrite and the split vote never run on a non-zero accumulator.  The families below keep
q, k, v standard normal and overwrite channel 0 so that the score gains a_i * b_j / sqrt(d) with a chosen row profile a and key profile b
(values stay below ~125 log2 units: far inside f16 for every operand).

The models restate only the operand rounding the kernels document (csrc/kernels/flash_attn.hip, planner.cpp plan_manual_attention):
  deferred_model  k_flash_attn: 64-key tiles, the move voted per 32-query block, the max moved as the kernel moves it, P rounded to f16
  onepass_model   k_flash_short: Q as f16, K as f16(f16(k) * scale * log2e), true row max, P normalised and then rounded to f16
  gemm_model      head dims > 160: Q, K, P and V as f16, scores in f32
Their distance from `exact` is the part of a kernel's error that is rounding by design; tests/test_kernel_logic.py pins what the families do
to the max on the model, tests/test_gpu_attention_scores.py runs them through the kernels."""
import numpy as np

LOG2E = 1.4426950408889634
KINDS = ("ramp3", "ramp12", "spike_last", "spike_mid", "descend", "offset_neg", "offset_pos")
MOVING = ("ramp3", "ramp12", "spike_last", "spike_mid")       # the max moves after tile 0 (with enough keys)
STILL = ("descend", "offset_neg", "offset_pos")               # it must not


def make(kind, Lq, Lk, d, rng):
    """q [Lq, d], k [Lk, d], v [Lk, d] (f32): standard normal, channel 0 of q and k replaced by the family's profiles."""
    q = rng.standard_normal((Lq, d)).astype(np.float32)
    k = rng.standard_normal((Lk, d)).astype(np.float32)
    v = rng.standard_normal((Lk, d)).astype(np.float32)
    i = np.arange(Lq)
    j = np.arange(Lk)
    sd_ = np.sqrt(d)
    ramp_rows = sd_ * (0.5 + (i % 32) / 32.0)
    spike_rows = sd_ * 0.5 * (i % 7)
    if kind == "randn":
        return q, k, v
    if kind == "ramp3":
        a, b = ramp_rows, j * 3.0 / (64.0 * LOG2E)
    elif kind == "ramp12":
        a, b = ramp_rows, j * 12.0 / (64.0 * LOG2E)
    elif kind == "descend":
        a, b = ramp_rows, -j * 6.0 / (64.0 * LOG2E)
    elif kind == "spike_last":
        a, b = spike_rows, np.zeros(Lk)
        b[Lk - 1] = 12.0
    elif kind == "spike_mid":
        a, b = spike_rows, np.zeros(Lk)
        if Lk > 64:
            b[64] = 12.0
        b[Lk // 2] = 14.0
    elif kind == "offset_neg":
        a, b = np.full(Lq, 2.0 * sd_), np.full(Lk, -40.0)
    elif kind == "offset_pos":
        a, b = np.full(Lq, 2.0 * sd_), np.full(Lk, 40.0)
    else:
        raise ValueError(kind)
    q[:, 0] = a
    k[:, 0] = b
    return q, k, v


def make_heads(kind, Lq, Lk, d, HN, rng):
    """HN independent draws of one family: q [HN, Lq, d], k, v [HN, Lk, d]."""
    qs, ks, vs = zip(*(make(kind, Lq, Lk, d, rng) for _ in range(HN)))
    return np.stack(qs), np.stack(ks), np.stack(vs)


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float64)


def rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _chunks(n, step=32):
    return [slice(s, min(n, s + step)) for s in range(0, n, step)]


def exact(q, k, v, scale):
    """softmax(scale * q k^T) v in float64; q [..., Lq, d], k, v [..., Lk, d]."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    if q.ndim == 2:
        return exact(q[None], k[None], v[None], scale)[0]
    out = np.empty(q.shape[:-1] + (v.shape[-1],))
    for c in _chunks(q.shape[0]):
        s = (q[c] @ k[c].transpose(0, 2, 1)) * scale
        s -= s.max(-1, keepdims=True)
        p = np.exp(s)
        p /= p.sum(-1, keepdims=True)
        out[c] = p @ v[c]
    return out


def deferred_model(q, k, v, scale, thr=8.0, mslot=False):
    """k_flash_attn's online softmax with the DEFERRED running max, on float64 scores.
    Returns (out, moves, split, pmax): the output; the block-level moves of the max after tile 0 (one 32-query block, one 64-key tile); how many of
    those were voted by only SOME of the block's rows; the largest P.
    mslot: the max-slot form (d = 40, f16 K / V) — scores relative to the max, the max kept f16-representable, first tile `tmax`, later
    tiles `max(tmax, 0)`."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    if q.ndim == 2:
        o, a, b, c = deferred_model(q[None], k[None], v[None], scale, thr, mslot)
        return o[0], a, b, c
    HN, Lq, _ = q.shape
    Lk, dv = k.shape[1], v.shape[2]
    out = np.empty((HN, Lq, dv))
    moves = split = 0
    pmax = 0.0
    for c in _chunks(HN):
        s_all = (q[c] @ k[c].transpose(0, 2, 1)) * (scale * LOG2E)      # log2 units
        for q0 in range(0, Lq, 32):
            s_blk = s_all[:, q0:q0 + 32]                                        # [h, rows, Lk]
            nh, nr = s_blk.shape[:2]
            m = np.zeros((nh, nr)) if mslot else np.full((nh, nr), -np.inf)
            l = np.zeros((nh, nr))
            o = np.zeros((nh, nr, dv))
            for kt in range(0, Lk, 64):
                s = s_blk[:, :, kt:kt + 64]
                tmax = s.max(-1)
                over = (tmax - m > thr) if (mslot or kt > 0) else np.ones_like(tmax, bool)
                vote = np.ones(nh, bool) if kt == 0 else over.any(-1)           # per head: this block's wave
                if kt > 0:
                    moves += int(vote.sum())
                    split += int((vote & ~over.all(-1)).sum())
                if mslot:
                    rel = tmax - m
                    step = rel if kt == 0 else np.maximum(rel, 0.0)
                    m_new = np.minimum(f16r(np.minimum(m + step, 65504.0)), 65504.0)
                else:
                    m_new = np.maximum(m, tmax)
                m_new = np.where(vote[:, None], m_new, m)
                with np.errstate(invalid="ignore"):
                    alpha = np.where(m_new == m, 1.0, np.exp2(m - m_new))       # m = -inf on the first tile -> 0
                l *= alpha
                o *= alpha[..., None]
                m = m_new
                p = np.exp2(s - m[..., None]).astype(np.float32).astype(np.float16)   # may overflow to inf: reported through pmax
                pmax = max(pmax, float(p.max()))
                p = p.astype(np.float64)
                l += p.sum(-1)
                o += p @ v[c][:, kt:kt + 64]
            out[c, q0:q0 + 32] = o / l[..., None]
    return out, moves, split, pmax


def onepass_model(q, k, v, scale):
    """k_flash_short: the scale rides in K (rounded to f16 a second time), one pass over all keys, P normalised BEFORE it is rounded to f16."""
    if np.ndim(q) == 2:
        return onepass_model(q[None], k[None], v[None], scale)[0]
    q16, v16 = f16r(q), f16r(v)
    k16 = f16r(np.asarray(k, np.float32).astype(np.float16).astype(np.float32) * np.float32(scale * LOG2E))
    out = np.empty(q16.shape[:-1] + (v16.shape[-1],))
    for c in _chunks(q16.shape[0]):
        s = (q16[c] @ k16[c].transpose(0, 2, 1))
        p = np.exp2(s - s.max(-1, keepdims=True))
        p = f16r(p / p.sum(-1, keepdims=True))
        out[c] = p @ v16[c]
    return out


def gemm_model(q, k, v, scale):
    """head dims > 160: S = scale * f16(Q) f16(K)^T kept in f32, row softmax written as f16, O = P f16(V)."""
    if np.ndim(q) == 2:
        return gemm_model(q[None], k[None], v[None], scale)[0]
    q16, k16, v16 = f16r(q), f16r(k), f16r(v)
    out = np.empty(q16.shape[:-1] + (v16.shape[-1],))
    for c in _chunks(q16.shape[0]):
        s = ((q16[c] @ k16[c].transpose(0, 2, 1)) * scale).astype(np.float32).astype(np.float64)
        p = np.exp(s - s.max(-1, keepdims=True))
        p = f16r(p / p.sum(-1, keepdims=True))
        out[c] = p @ v16[c]
    return out


# ---- the GPU cases (tests/test_gpu_attention_scores.py), shared with the model tests of tests/test_kernel_logic.py: (d, Lq, Lk, HN)
FLASH_NODE_CASES = [          # FLASH_ATTN_EXT node, f16 K / V
    (40, 96, 333, 2),         # max slot, one query block per wave
    (40, 200, 333, 512),      # max slot, TWO query blocks per wave (ceil(Lq / 256) * HN = 512), ragged second block, ragged key tail
    (64, 96, 333, 2),         # select-free staging
    (128, 96, 200, 2),        # select-free staging
    (16, 96, 333, 2),         # 48-wide tile without the slot
    (80, 96, 333, 2),         # ones column on the 3-block accumulator
    (96, 64, 200, 2),
    (160, 64, 200, 1),
    (20, 64, 200, 2),         # d % 8 != 0: generic staging
]
MANUAL_CASES = [(40, 96, 333, 2), (64, 96, 200, 2), (80, 64, 200, 2), (160, 64, 130, 1)]     # f32 K / V^T: the !FAST kernel
SHORT_CASES = [(d, 100, Lk, 2) for d in (40, 64) for Lk in (65, 77, 96)]                      # k_flash_short
GEMM_CASES = [(512, 96, 132, 1), (192, 64, 68, 2)]                                            # head dims > 160
BLOCK_CASES = [(40, 8, 300, 300, 2, 320), (40, 8, 130, 77, 3, 768)]                           # (d, H, Lq, Lk, N, ctx): fused operand paths


def uses_max_slot(d, Lk, fast=True):
    """launch_flash_attn: f16 K / V at d = 40 beyond the short-key kernel's range run the max-slot kernels"""
    return fast and d == 40 and not (64 < Lk <= 96)


def ramp_can_move(kind, Lk):
    """Tile t's maximum exceeds tile 0's by at most 1.5 * rise * t log2 units (row profile <= 1.5, `rise` per 64 keys), so crossing the bar of 8
    needs rise * 1.5 * (tiles after the first that hold the ramp) > 8: ramp3 over fewer than three full tiles cannot, everything else here can."""
    return not (kind == "ramp3" and Lk < 192)
