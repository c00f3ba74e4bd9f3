"""The reference of the Linear route tests (linear_cases.py, test_linear_ref_cpu.py, test_gpu_linear_routes.py), and wrong versions of it.  Plain NumPy, no project code.

linear_ref is y = epilogue(x @ dequant(w).T) in float64 (float32 matmul for the few chip-filling shapes: exact under the asserted bound, confirmed on sampled rows in
int64), x [rows, K] the activation rows in graph order, w [M, K].  Epilogues (EPILOGUES): none / bias / bias+res / res+bias / scale (ggml_ext_linear: x * s -> Linear
-> * 1 / s -> + bias, s a power of two) / gate (r + (acc + b) * gate[batch]) / gelu (fc1 + b -> tanh-GELU -> identity fc2) / geglu (FF1 + b -> value * gelu(gate) ->
identity FF2) / presilu (SiLU -> one non-zero weight per row) / ln_next (bias, then + r2; the LayerNorm branch that also reads the Linear is not part of the reference).

Exactness.  The cases use integer-valued operands (make_case_data): every product and every partial sum, in any order, is a multiple of one power of two, and
check_exact asserts that max|x| * max_row(sum_k |w|) + |epilogue terms|, in units of it, stays below 2^24 (this is never larger than the max|x| * max|w| * K of the
conv tests, and it is the sum the kernels really form; the quantised weights hold one +-127 d per block, which the looser product would overcount 100-fold), and
that every exact value written to an f16 operand image (x, w) stays below 2^11 units; the images behind a transcendental are rounded by design and only have to stay
inside f16's range.  float64, float32 and the f16 x f16 -> f32 MFMA then represent every intermediate exactly: K
slices, tile shapes and summation orders cannot change a bit.  The bar is bit for bit, except behind a transcendental (gelu / geglu / presilu), where it is
transcendental_bar below.

Quantised weights are CONSTRUCTED so that dequant(quantise(w)) == w bit for bit (make_quantised): every q8_0 block of 32 holds one +-127 d and otherwise multiples of
d within -2 .. 2, every q4_0 block one -8 d and otherwise multiples of d in -7 d .. 7 d, with d varying from block to block over {1/4, 1/2, 1, 2} — under the
reference's rules (d = amax / 127; d = max / -8) the block stores exactly d.  quantise / dequantise restate those rules in NumPy for the mutants.

MUTANTS are linear_ref with one indexing bug each, one per bug class the cases are meant to catch; they prove (without a GPU) that a case's shapes and data tell such
a bug from the truth."""
from __future__ import annotations

import numpy as np

EXACT_BOUND = 2 ** 24
F16_EXACT = 2 ** 11    # integers below it are exact in an f16 operand image
F16_MAX = 65504.0
EPILOGUES = ("none", "bias", "bias+res", "res+bias", "scale", "gate", "gelu", "geglu", "presilu", "ln_next")
TRANSCENDENTAL = ("gelu", "geglu", "presilu")
PRE_SCALE, POST_SCALE = 0.125, 8.0
QK = 32


# ------------------------------------------------------------------------------------------------ q8_0 / q4_0 in NumPy
def quantise(w: np.ndarray, wtype: str):
    """w [M, K] -> (d [M, K / 32] float32 through f16, q [M, K / 32, 32] integers as stored: q8_0 -127 .. 127, q4_0 0 .. 15) by the reference's rules"""
    M, K = w.shape
    assert K % QK == 0
    b = np.asarray(w, dtype=np.float32).reshape(M, K // QK, QK)
    if wtype == "q8_0":
        d = (np.abs(b).max(axis=2) / np.float32(127.0)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, 1), 0).astype(np.float32)
        q = np.rint(b * inv[..., None]).astype(np.int32)
    elif wtype == "q4_0":
        idx = np.abs(b).argmax(axis=2)                       # the first of the largest magnitudes, signed
        mx = np.take_along_axis(b, idx[..., None], axis=2)[..., 0]
        d = (mx / np.float32(-8.0)).astype(np.float32)
        inv = np.where(d != 0, np.float32(1.0) / np.where(d != 0, d, 1), 0).astype(np.float32)
        q = np.minimum(15, (b * inv[..., None] + np.float32(8.5)).astype(np.int32))
    else:
        raise ValueError(wtype)
    return d.astype(np.float16).astype(np.float32), q


def dequantise(d: np.ndarray, q: np.ndarray, wtype: str, mutant=None) -> np.ndarray:
    """-> float64 [M, K].  mutant: one of the three dequantisation bugs"""
    d = np.asarray(d, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    if mutant == "scale_from_neighbour_block":
        d = np.roll(d, -1, axis=1)
    if wtype == "q4_0":
        if mutant == "q4_nibbles_swapped":   # byte j holds element j (low nibble) and element j + 16 (high nibble)
            q = np.concatenate([q[..., 16:], q[..., :16]], axis=2)
        if mutant != "q4_offset_omitted":
            q = q - 8.0
    return (q * d[..., None]).reshape(q.shape[0], -1)


def make_quantised(rng, M: int, K: int, wtype: str) -> np.ndarray:
    """float32 [M, K] that q8_0 / q4_0 stores exactly"""
    nb = K // QK
    # a random start per row, then steps of 1 or 3 through the four scales: neighbouring blocks never share one
    d = np.array([0.25, 0.5, 1.0, 2.0])[(rng.integers(0, 4, size=(M, 1)) + np.arange(nb)[None, :] * rng.choice(np.array([1, 3]), size=(M, 1))) % 4]
    pos = rng.integers(0, QK, size=(M, nb))
    if wtype == "q8_0":
        lim = np.floor(2.0 / d)[..., None]
        q = np.rint(rng.uniform(-1, 1, size=(M, nb, QK)) * lim)
        peak = 127.0 * rng.choice(np.array([-1.0, 1.0]), size=(M, nb))
    else:
        q = rng.integers(-7, 8, size=(M, nb, QK)).astype(np.float64)
        peak = np.full((M, nb), -8.0)
    np.put_along_axis(q, pos[..., None], peak[..., None], axis=2)
    return (q * d[..., None]).reshape(M, K).astype(np.float32)


# ------------------------------------------------------------------------------------------------ exactness
def _pow2(v: float) -> bool:
    m, _ = np.frexp(float(v))
    return v > 0 and m == 0.5


def check_exact(x, w, *, unit_x=1.0, unit_w=1.0, extra=0.0):
    """max|x| * max_row(sum |w|) + extra < 2^24 in units of unit_x * unit_w, the powers of two x and w are multiples of (x / 8: 1 / 8; quantised w: d >= 1 / 4);
    -> that bound (the largest magnitude any partial sum or output can take)"""
    assert _pow2(unit_x) and _pow2(unit_w)
    for name, a, u in (("x", x, unit_x), ("w", w, unit_w)):
        if not np.array_equal(np.asarray(a) / u, np.rint(np.asarray(a) / u)):
            raise ValueError(f"{name} is not a multiple of {u}: the bit-for-bit bar does not hold")
    if not (float(np.abs(x).max()) / unit_x < F16_EXACT and float(np.abs(w).max()) / unit_w < F16_EXACT):
        raise ValueError("an operand does not fit an f16 image exactly: >= 2^11 units")
    bound = float(np.abs(x).max()) * float(np.abs(np.asarray(w, dtype=np.float64)).sum(axis=1).max()) + extra
    if not bound / (unit_x * unit_w) < EXACT_BOUND:
        raise ValueError(f"exactness bound broken: {bound} / {unit_x * unit_w} >= 2^24")
    return bound


# ------------------------------------------------------------------------------------------------ the functions behind the transcendental epilogues
def gelu64(p):
    p = np.asarray(p, dtype=np.float64)
    return 0.5 * p * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (p + 0.044715 * p ** 3)))


def silu64(p):
    p = np.asarray(p, dtype=np.float64)
    return p / (1.0 + np.exp(-p))


def ulp_f16(v):
    """spacing of f16 at |v| (the subnormal spacing 2^-24 below 2^-14)"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(a)) - 10)


def transcendental_bar(image64, p, factor=1.0):
    """(ulp_f16(image64) + 2^-18 * max(1, |p|)) * factor: the f16 rounding of the image value landing on the nearest value or its neighbour, plus a few f32 ulps on
    1 + tanh(.) / 1 + exp(.) with a factor-16 margin for fast-math intrinsics (an assumption, not a measurement).  gelu: image64 = gelu(p), factor 1.  geglu:
    image64 = v * gelu(g), p = g, factor max(1, |v|).  presilu: image64 = silu(p), factor = |the row's one weight| (the exact product that follows the image)"""
    t1, t2 = transcendental_terms(image64, p, factor)
    return t1 + t2


def transcendental_terms(image64, p, factor=1.0):
    """the two terms of transcendental_bar, each times factor"""
    return np.abs(factor) * ulp_f16(image64), np.abs(factor) * 2.0 ** -18 * np.maximum(1.0, np.abs(p)) + 0.0 * np.asarray(image64)


# ------------------------------------------------------------------------------------------------ the reference
MUTANTS = ("drop_last_k_block_of_a_slice", "read_past_k_padding", "last_column_tile_shifted", "last_row_tile_skipped", "rows_after_256_shifted", "bias_by_row",
           "residual_wrong_ld", "gate_wrong_batch", "siblings_swapped", "q4_nibbles_swapped", "q4_offset_omitted", "scale_from_neighbour_block",
           "slices_summed_s_minus_1", "geglu_halves_swapped")
_DEQUANT_MUTANTS = ("q4_nibbles_swapped", "q4_offset_omitted", "scale_from_neighbour_block")


def mutant_applies(mutant: str, *, rows, K, M, wtype, epi, S=1, batches=1, siblings=1) -> bool:
    """has a Linear of this shape the feature the mutant breaks?"""
    nt = (K + 63) // 64 * 2
    per = (nt + S - 1) // S
    return {"drop_last_k_block_of_a_slice": 32 * (per - 1) < K if S > 1 else True, "read_past_k_padding": K % 64 != 0 and rows > 1, "last_column_tile_shifted": M > 1,
            "last_row_tile_skipped": True, "rows_after_256_shifted": rows > 257, "bias_by_row": epi not in ("none", "presilu") and M > 1 and rows > 1,
            "residual_wrong_ld": epi in ("bias+res", "res+bias", "gate", "ln_next") and rows > 1 and M > 1, "gate_wrong_batch": epi == "gate" and batches > 1,
            "siblings_swapped": siblings > 1, "q4_nibbles_swapped": wtype == "q4_0", "q4_offset_omitted": wtype == "q4_0",
            "scale_from_neighbour_block": wtype in ("q8_0", "q4_0") and K > QK, "slices_summed_s_minus_1": S > 1 and 32 * per * (S - 1) < K,
            "geglu_halves_swapped": epi == "geglu"}[mutant]


def _weights64(w, wtype, mutant):
    if wtype in ("q8_0", "q4_0"):
        d, q = quantise(w, wtype)
        return dequantise(d, q, wtype, mutant if mutant in _DEQUANT_MUTANTS else None)
    return np.asarray(w, dtype=np.float64)


def matmul(x, w, fast=False):
    """x [rows, K] @ w [M, K].T in float64 (fast: through a float32 matmul, exact under check_exact's bound)"""
    return (x.astype(np.float32) @ w.astype(np.float32).T).astype(np.float64) if fast else x @ w.T


def _acc(x, w, *, mutant=None, S=1, bm=128, bn=128, fast=False, true_acc=None):
    """the accumulators [rows, M] float64.  true_acc: x @ w.T where the caller has it already (the K-block mutants then subtract their block's share, exactly)"""
    rows, K = x.shape
    M = w.shape[0]
    nt = (K + 63) // 64 * 2               # stages of 32 over K padded to 64
    per = (nt + S - 1) // S
    acc = matmul(x, w, fast) if true_acc is None else true_acc
    if mutant == "drop_last_k_block_of_a_slice":
        blk = per - 1 if S > 1 else (K + 31) // 32 - 1   # slice 0 loses its last block (unsplit: the last block that holds real columns)
        acc = acc - x[:, 32 * blk:32 * (blk + 1)] @ w[:, 32 * blk:32 * (blk + 1)].T
    elif mutant == "slices_summed_s_minus_1":
        acc = acc - x[:, 32 * per * (S - 1):] @ w[:, 32 * per * (S - 1):].T
    if mutant == "read_past_k_padding":   # lanes K .. of row r hold the first values of row r + 1 and meet those columns' weights
        pad = min((-K) % 64, K)
        acc = acc.copy()
        acc[:-1] += x[1:, :pad] @ w[:, :pad].T
    elif mutant == "last_column_tile_shifted":
        c0 = bn * ((M - 1) // bn)
        acc = acc.copy()
        acc[:, c0:] = acc[:, np.minimum(np.arange(c0, M) + 1, M - 1)] if M - c0 > 1 else acc[:, [c0 - 1]] if c0 else -acc[:, c0:]
    elif mutant == "last_row_tile_skipped":
        acc = acc.copy()
        acc[bm * ((rows - 1) // bm):] = 0
    elif mutant == "rows_after_256_shifted":
        acc = acc.copy()
        acc[256:] = acc[np.minimum(np.arange(256, rows) + 1, rows - 1)]
    return acc


def prepare(x, epi):
    """the activation rows the contraction sees, float64"""
    x = np.asarray(x, dtype=np.float64)
    return silu64(x) if epi == "presilu" else x * PRE_SCALE if epi == "scale" else x


def linear_ref(x, w, wtype="f16", *, epi="none", bias=None, residual=None, gate=None, batches=1, mutant=None, S=1, bm=128, bn=128, fast=False, true_acc=None):
    """x [rows, K], w [M, K] (the values the weight type stores), bias [M], residual [rows, M] (geglu: [rows, M / 2]), gate [batches, M] -> (out float64, p):
    out the epilogue's result ([rows, M]; geglu [rows, M / 2]), p the pre-activations behind a transcendental epilogue (else None)"""
    assert epi in EPILOGUES and (mutant is None or mutant in MUTANTS), (epi, mutant)
    x = np.asarray(x, dtype=np.float64)
    rows, M = x.shape[0], w.shape[0]
    w64 = _weights64(w, wtype, mutant)
    acc = _acc(prepare(x, epi), w64, mutant=mutant, S=S, bm=bm, bn=bn, fast=fast, true_acc=None if mutant in _DEQUANT_MUTANTS else true_acc)
    if epi == "scale":
        acc = acc * POST_SCALE
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        acc = acc + (b[np.arange(rows) % M][:, None] if mutant == "bias_by_row" else b[None, :])
    if epi == "presilu":
        return acc, x
    if epi == "gelu":
        return gelu64(acc), acc
    if epi == "geglu":
        inner = M // 2
        v, g = (acc[:, inner:], acc[:, :inner]) if mutant == "geglu_halves_swapped" else (acc[:, :inner], acc[:, inner:])
        return v * gelu64(g), (v, g)
    if epi == "gate":
        gt = np.asarray(gate, dtype=np.float64)
        per = rows // batches
        bidx = (np.arange(rows) // per + (1 if mutant == "gate_wrong_batch" else 0)) % batches
        acc = acc * gt[bidx]
    if residual is not None:
        r = np.asarray(residual, dtype=np.float64)
        if mutant == "residual_wrong_ld":
            r = r.reshape(-1)[(np.arange(rows)[:, None] * (M - 1) + np.arange(M)[None, :])]
        acc = acc + r
    return acc, None


# ------------------------------------------------------------------------------------------------ data
def ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def nonzero_ints(rng, lo, hi, shape):
    v = rng.integers(lo, hi, size=shape)
    return np.where(v >= 0, v + 1, v).astype(np.float32)


def one_per_row(rng, M, K, wtype):
    """presilu weights: one non-zero per row (columns walked from both ends of K, a random sign), a value the type stores exactly and that leaves each output ONE image value: +-1 for
    f32 / f16 / bf16, +-127 d for q8_0, -8 d for q4_0 (d over {1/4, 1/2, 1, 2})"""
    w = np.zeros((M, K), dtype=np.float32)
    r = np.arange(M)
    col = np.where(r % 2 == 0, (r * 7 + 3) % K, (K - 1 - r * 7) % K)   # from both ends of K: the first and the last block of 32 carry weights
    d = rng.choice(np.array([0.25, 0.5, 1.0, 2.0]), size=M)
    v = {"q8_0": 127.0 * d * rng.choice(np.array([-1.0, 1.0]), size=M), "q4_0": -8.0 * d}.get(wtype, rng.choice(np.array([-1.0, 1.0]), size=M))
    w[np.arange(M), col] = v
    return w
