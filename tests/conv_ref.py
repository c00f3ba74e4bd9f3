"""The reference of the conv route tests (conv_cases.py, test_conv_ref_cpu.py, test_gpu_conv_routes.py), and wrong versions of it.  Plain NumPy, no project code.

conv_ref is a 2-D cross-correlation the way the model graphs state it (ggml_conv_2d: x [N, IC, H, W], w [OC, IC, KH, KW], the same stride and zero padding on both
axes), optionally over a nearest x2 upscale of x, with the epilogue in the reference's order: conv * scale, + bias, + emb, + residual.

Exactness.  The cases use integer-valued operands (make_case_data).  Every product and every partial sum, in any order, is then an integer multiple of one power
of two, and conv_ref asserts that the largest possible sum, in units of it, stays below 2^24: float64, float32 and the f16 x f16 -> f32 MFMA all represent every
intermediate exactly, so K slices, tile shapes, K orders and workgroup orders cannot change a bit.  The bar of the tests is therefore bit for bit, and any difference
is an indexing bug.

MUTANTS are conv_ref with one indexing bug each, one per bug class the cases are meant to catch.  They prove (on a machine without a GPU) that a case's shapes and
data tell such a bug from the truth: a case on which a mutant equals conv_ref could not have caught that bug."""
from __future__ import annotations

import numpy as np

EXACT_BOUND = 2 ** 24


def _pow2(v: float) -> bool:
    m, _ = np.frexp(float(v))
    return v > 0 and m == 0.5


def _check_exact(x, w, K, pre_scale, post_scale, bias, chan_add, residual):
    """max|x| * max|w| * K + |epilogue terms| < 2^24, in units of the operands' common power of two"""
    assert _pow2(pre_scale) and _pow2(post_scale), "Conv2d scales are powers of two"
    for name, a in (("x", x), ("w", w), ("bias", bias), ("chan_add", chan_add), ("residual", residual)):
        if a is not None and not np.array_equal(a, np.rint(a)):
            raise ValueError(f"{name} is not integer-valued: the bit-for-bit bar does not hold")
    unit = min(1.0, pre_scale) * min(1.0, post_scale)
    bound = float(np.abs(x).max()) * pre_scale * float(np.abs(w).max()) * K * max(1.0, post_scale)
    bound += sum(float(np.abs(a).max()) for a in (bias, chan_add, residual) if a is not None)
    if not bound / unit < EXACT_BOUND:
        raise ValueError(f"exactness bound broken: {bound} / {unit} >= 2^24")


class _Geometry:
    def __init__(self, x, w, stride, pad, upscale2x):
        self.N, self.IC, self.H, self.W = x.shape
        self.OC, ic, self.KH, self.KW = w.shape
        assert ic == self.IC, (x.shape, w.shape)
        self.stride, self.pad, self.ups = stride, pad, 2 if upscale2x else 1
        self.CH, self.CW = self.H * self.ups, self.W * self.ups   # the canvas the taps are gathered from
        self.OH = (self.CH + 2 * pad - self.KH) // stride + 1
        self.OW = (self.CW + 2 * pad - self.KW) // stride + 1


MARGIN = 2   # pixels around the canvas: the padding, and one more for the mutants that look one pixel further


def _canvas(x, g: _Geometry, mutant=None):
    """the images (after the nearest x2 upscale: index repetition) inside a margin of MARGIN pixels -> [N, IC, CH + 2 MARGIN, CW + 2 MARGIN].
    The margin is zero; two mutants fill it with something else"""
    def src(size):   # canvas coordinate -> source coordinate
        c = np.arange(size)
        if g.ups == 1:
            return c
        if mutant == "upscale_off_by_one":   # odd coordinates take the next source pixel
            return np.minimum((c + 1) // 2, size // 2 - 1)
        return c // 2

    M, CH, CW = MARGIN, g.CH, g.CW
    cv = x[:, :, src(CH)[:, None], src(CW)[None, :]]
    P = np.zeros((g.N, g.IC, CH + 2 * M, CW + 2 * M))
    P[:, :, M:M + CH, M:M + CW] = cv
    if mutant == "halo_from_neighbour_image":   # the rows above / below an image are the neighbouring image's last / first rows
        P[1:, :, :M, M:M + CW] = cv[:-1, :, CH - M:, :]
        P[:-1, :, M + CH:, M:M + CW] = cv[1:, :, :M, :]
    if mutant == "halo_from_wrapped_row":   # the columns left / right of a row are the previous row's last / the next row's first pixels
        P[:, :, M + 1:M + CH, :M] = cv[:, :, :CH - 1, CW - M:]
        P[:, :, M:M + CH - 1, M + CW:] = cv[:, :, 1:, :M]
    return P


def _conv(x, w, stride, pad, upscale2x=False, mutant=None, S=2):
    """the bare convolution in float64 -> [N, OC, OH, OW]"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    g = _Geometry(x, w, stride, pad, upscale2x)
    nblk = (g.IC + 31) // 32   # 32-channel blocks that hold real channels
    if mutant == "drop_last_k_block":
        w = w.copy()
        w[:, 32 * (nblk - 1):] = 0
    elif mutant == "drop_last_block_of_a_slice":   # slice 0 of S slices over the blocks loses its last one
        per = (nblk + S - 1) // S
        w = w.copy()
        w[:, 32 * (per - 1):32 * per] = 0
    elif mutant == "swap_taps":
        w = np.ascontiguousarray(np.swapaxes(w, 2, 3))
    P = _canvas(x, g, mutant)
    off = MARGIN - pad + (1 if mutant == "stride2_starts_at_1" else 0)

    def tap(n, kh, kw, dc=0):   # canvas pixels under tap (kh, kw) of every output position of image n (dc: so many columns further) -> [IC, OH, OW]
        r0, c0 = off + kh, off + kw + dc
        return P[n, :, r0:r0 + stride * (g.OH - 1) + 1:stride, c0:c0 + stride * (g.OW - 1) + 1:stride]

    taps = [(kh, kw) for kh in range(g.KH) for kw in range(g.KW)]
    w2 = w.transpose(0, 2, 3, 1).reshape(g.OC, len(taps) * g.IC)   # K order (tap, channel)
    pad_lanes = min((-g.IC) % 64, g.IC) if mutant == "pad_lanes_read_next_pixel" else 0
    if pad_lanes:   # the lanes IC .. of every pixel hold the first channels of the NEXT pixel and meet those channels' weights
        w2 = np.concatenate([w2, w.transpose(0, 2, 3, 1)[..., :pad_lanes].reshape(g.OC, -1)], axis=1)
    out = np.empty((g.N, g.OC, g.OH, g.OW))
    for n in range(g.N):
        cols = [tap(n, kh, kw) for kh, kw in taps] + [tap(n, kh, kw, 1)[:pad_lanes] for kh, kw in taps if pad_lanes]
        out[n] = (w2 @ np.concatenate(cols, axis=0).reshape(w2.shape[1], -1)).reshape(g.OC, g.OH, g.OW)   # one matmul per image
    return out


def conv_ref(x, w, stride, pad, *, upscale2x=False, pre_scale=1, post_scale=1, bias=None, chan_add=None, residual=None, mutant=None, S=2):
    """x [N, IC, H, W], w [OC, IC, KH, KW], bias [OC], chan_add [N, OC], residual [N, OC, OH, OW] -> float32 [N, OC, OH, OW].
    mutant: one of MUTANTS (S: the slice count of drop_last_block_of_a_slice), None = the truth"""
    assert mutant is None or mutant in MUTANTS, mutant
    _check_exact(np.asarray(x), np.asarray(w), w.shape[1] * w.shape[2] * w.shape[3], pre_scale, post_scale, bias, chan_add, residual)
    acc = _conv(np.asarray(x, dtype=np.float64) * pre_scale, w, stride, pad, upscale2x, mutant, S)
    N, OC, OH, OW = acc.shape
    if mutant == "tail_rows_bias_only":   # the rows of the last, partial 256-row tile of the [N * OH * OW, OC] output matrix
        rows = N * OH * OW
        flat = acc.transpose(0, 2, 3, 1).reshape(rows, OC).copy()
        flat[256 * (rows // 256):] = 0
        acc = flat.reshape(N, OH, OW, OC).transpose(0, 3, 1, 2)
    out = acc * post_scale
    if bias is not None:
        out = out + np.asarray(bias, dtype=np.float64).reshape(1, OC, 1, 1)
    if chan_add is not None:
        out = out + np.asarray(chan_add, dtype=np.float64).reshape(N, OC, 1, 1)
    if residual is not None:
        out = out + np.asarray(residual, dtype=np.float64)
    if mutant == "last_column_masked_short":   # the last output channel is never stored
        out = out.copy()
        out[:, OC - 1] = 0
    return np.ascontiguousarray(out, dtype=np.float32)


MUTANTS = ("halo_from_neighbour_image", "halo_from_wrapped_row", "drop_last_k_block", "drop_last_block_of_a_slice", "swap_taps", "tail_rows_bias_only",
           "last_column_masked_short", "pad_lanes_read_next_pixel", "upscale_off_by_one", "stride2_starts_at_1")


def mutant_applies(mutant: str, *, N, IC, OC, OH, OW, ks, stride, upscale, S=2) -> bool:
    """has a conv of this geometry the feature the mutant breaks?"""
    nblk = (IC + 31) // 32
    return {"halo_from_neighbour_image": ks == 3 and N > 1, "halo_from_wrapped_row": ks == 3, "drop_last_k_block": True,
            "drop_last_block_of_a_slice": S > 1 and nblk >= S, "swap_taps": ks == 3, "tail_rows_bias_only": (N * OH * OW) % 256 != 0, "last_column_masked_short": True,
            "pad_lanes_read_next_pixel": IC % 64 != 0, "upscale_off_by_one": bool(upscale), "stride2_starts_at_1": stride == 2}[mutant]


def _nonzero_ints(rng, lo, hi, shape):
    """integers of lo .. hi without 0"""
    v = rng.integers(lo, hi, size=shape)   # hi excluded: hi - lo values
    return np.where(v >= 0, v + 1, v).astype(np.float32)


def make_case_data(case, seed: int) -> dict:
    """x in -4 .. 4, w in -2 .. 2, bias in -64 .. 64, residual in -8 .. 8, the embedding branch as integers (emb [N, E] in -2 .. 2, its Linear's weight in -1 .. 1 and
    bias in -8 .. 8): no all-zero channel (the first pixel / tap of each is non-zero), no zero on the border rows and columns of x (a dropped or misplaced halo
    always changes a sum's operands), the last output channel's bias non-zero"""
    rng = np.random.default_rng(seed)
    N, IC, OC, H, W, ks = case.N, case.IC, case.OC, case.H, case.W, case.ks
    x = rng.integers(-4, 5, size=(N, IC, H, W)).astype(np.float32)
    for sl in ((..., 0, slice(None)), (..., H - 1, slice(None)), (..., slice(None), 0), (..., slice(None), W - 1)):
        x[sl] = _nonzero_ints(rng, -4, 4, x[sl].shape)
    w = rng.integers(-2, 3, size=(OC, IC, ks, ks)).astype(np.float32)
    w[:, :, 0, 0] = _nonzero_ints(rng, -2, 2, (OC, IC))
    d = {"x": x, "w": w}
    g = _Geometry(x, w, case.stride, ks // 2, case.upscale)
    epi = case.epilogue
    if "bias" in epi:
        d["bias"] = _nonzero_ints(rng, -64, 64, (OC,))
    if "res" in epi or "res_first" in epi:
        d["residual"] = rng.integers(-8, 9, size=(N, OC, g.OH, g.OW)).astype(np.float32)
    if "emb" in epi:
        E = 32
        d["emb"] = rng.integers(-2, 3, size=(N, E)).astype(np.float32)
        d["emb_w"] = rng.integers(-1, 2, size=(OC, E)).astype(np.float32)
        d["emb_b"] = rng.integers(-8, 9, size=(OC,)).astype(np.float32)
        d["chan_add"] = (d["emb"].astype(np.float64) @ d["emb_w"].astype(np.float64).T + d["emb_b"]).astype(np.float32)
    return d
