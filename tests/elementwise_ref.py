"""Plain NumPy statements of the memory-bound glue ops, written from the ggml semantics (not from the kernels): arithmetic in float64, everything
else by indexing.  Arrays are C-ordered with the ggml dimensions reversed: a tensor with ne = [ne0, ne1, ne2, ne3] is an array of shape
(ne3, ne2, ne1, ne0); every function takes and returns arrays of at most four dimensions and treats missing leading ones as 1.

Correct rounding of +, -, *, / : the float64 result of two float32 operands, rounded to float32, is the correctly rounded float32 result
(53 >= 2 * 24 + 2 mantissa bits: the double rounding is innocuous for these four operations), which is also what NumPy's float32 operators give."""
from __future__ import annotations

from fractions import Fraction

import numpy as np


def as4(a: np.ndarray) -> np.ndarray:
    a = np.asarray(a)
    return a.reshape((1,) * (4 - a.ndim) + a.shape)


def ne_of(a: np.ndarray) -> list[int]:
    """ggml ne of an array"""
    return list(reversed(as4(a).shape))


def _mod_take(b4: np.ndarray, shape4) -> np.ndarray:
    """b indexed by i % b.ne[d] in every dimension, out to shape4"""
    for ax in range(4):
        b4 = np.take(b4, np.arange(shape4[ax]) % b4.shape[ax], axis=ax)
    return b4


def binary(op: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """ADD / SUB / MUL / DIV of f32 tensors, b broadcast onto a by i % b.ne[d]; correctly rounded float32"""
    a4 = as4(a).astype(np.float64)
    b4 = _mod_take(as4(b), a4.shape).astype(np.float64)
    with np.errstate(all="ignore"):
        r = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[op](a4, b4)
        return r.astype(np.float32).reshape(np.asarray(a).shape)


def unary(op: str, x: np.ndarray) -> np.ndarray:
    """float64 value of the activation at the float32 inputs"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        if op == "silu":
            return x / (1.0 + np.exp(-x))
        if op == "sigmoid":
            return 1.0 / (1.0 + np.exp(-x))
        if op == "tanh":
            return np.tanh(x)
        if op == "relu":
            return np.where(x > 0, x, 0.0)
        if op == "neg":
            return -x
        if op == "exp":
            return np.exp(x)
        if op == "gelu":  # the tanh form
            return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * x * (1.0 + 0.044715 * x * x)))
        if op == "gelu_quick":  # the sigmoid form
            return x / (1.0 + np.exp(-1.702 * x))
    raise KeyError(op)


def _round_fraction_to_f32(q: Fraction) -> np.float32:
    """exact rational -> float32, round to nearest even (the values here are far from the subnormal and overflow ranges)"""
    if q == 0:
        return np.float32(0.0)
    sign, q = (-1.0, -q) if q < 0 else (1.0, q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    scaled = q / Fraction(2) ** (e - 23)          # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return np.float32(sign * float(n) * 2.0 ** (e - 23))


def scale_bias(x: np.ndarray, s: float, b: float) -> np.ndarray:
    """x * s + b as ONE fused multiply-add: the exact value rounded once to float32.  float64 holds the product exactly and rounds the sum to 53 bits;
    where that sum lies within one float64 ulp of a float32 rounding boundary the element is redone in exact rational arithmetic."""
    x32 = np.asarray(x, dtype=np.float32)
    s32, b32 = np.float32(s), np.float32(b)
    r64 = x32.astype(np.float64) * np.float64(s32) + np.float64(b32)
    out = r64.astype(np.float32)
    near_tie = (r64.view(np.uint64) & np.uint64(0x1FFFFFFF)).astype(np.int64)  # the 29 bits below a float32 mantissa
    risky = (np.abs(near_tie - 0x10000000) <= 1) & np.isfinite(r64)
    flat_o, flat_x = out.reshape(-1), x32.reshape(-1)
    for i in np.flatnonzero(risky.reshape(-1)):
        flat_o[i] = _round_fraction_to_f32(Fraction(float(flat_x[i])) * Fraction(float(s32)) + Fraction(float(b32)))
    return out


def bf16_bits(a: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns: round to nearest even; a NaN keeps its top bits and gets the quiet bit (bit 6 of the bf16 pattern)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rne = (u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 64, rne).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_to(a: np.ndarray, dtype: str) -> np.ndarray:
    """the float32 value of `a` (f32) after a store as f32 / f16 / bf16"""
    a = np.asarray(a, dtype=np.float32)
    if dtype == "f32":
        return a
    if dtype == "f16":
        with np.errstate(all="ignore"):
            return a.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        return bf16_to_f32(bf16_bits(a)).reshape(a.shape)
    raise KeyError(dtype)


def copy(src: np.ndarray, dst_shape, dtype: str = "f32") -> np.ndarray:
    """DUP / CONT / CPY: element i of the source in logical order becomes element i of the destination in logical order"""
    return round_to(np.ascontiguousarray(src).reshape(dst_shape), dtype)


def concat(a: np.ndarray, b: np.ndarray, dim: int) -> np.ndarray:
    return np.concatenate([as4(a), as4(b)], axis=3 - dim)


def repeat(a: np.ndarray, dst_shape) -> np.ndarray:
    return _mod_take(as4(a), as4(np.empty(dst_shape, dtype=np.int8)).shape)


def upscale_nearest(a: np.ndarray, dst_shape) -> np.ndarray:
    """dst[i] = src[int(i / (float32(dst_ne) / src_ne))] per dimension, the quotient and the division in float32"""
    a4 = as4(a)
    shape4 = as4(np.empty(dst_shape, dtype=np.int8)).shape
    for ax in range(4):
        sf = np.float32(shape4[ax]) / np.float32(a4.shape[ax])
        idx = (np.arange(shape4[ax]).astype(np.float32) / sf).astype(np.int64)
        a4 = np.take(a4, idx, axis=ax)
    return a4


def pad_ext(a: np.ndarray, pads) -> np.ndarray:
    """pads = [lp0, rp0, lp1, rp1, lp2, rp2, lp3, rp3] in ggml dimension order"""
    return np.pad(as4(a), [(pads[2 * d], pads[2 * d + 1]) for d in (3, 2, 1, 0)])


def get_rows(table: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """table (ne3, ne2, rows, nc) decoded to f32, ids (ne2', ne1', ne0') with ne1' = table.ne2 -> (ne2', ne1', ne0', nc): row ids[i12, i11, i10] of plane (i12, i11)"""
    t4 = as4(table)
    i3 = np.asarray(ids).reshape((1,) * (3 - np.asarray(ids).ndim) + np.asarray(ids).shape)
    out = np.empty(i3.shape + (t4.shape[3],), dtype=np.float32)
    for i12 in range(i3.shape[0]):
        for i11 in range(i3.shape[1]):
            out[i12, i11] = t4[i12 % t4.shape[0], i11][i3[i12, i11]]
    return out


def timestep_embedding(t: np.ndarray, dim: int, max_period: int) -> np.ndarray:
    """(n, dim) float64: cos(t f_j) for j < dim/2, then sin(t f_j), f_j = exp(-ln(max_period) j / (dim/2)); a zero in the last column when dim is odd"""
    half = dim // 2
    t = np.asarray(t, dtype=np.float32).astype(np.float64)
    out = np.zeros((t.size, dim), dtype=np.float64)
    if half:
        arg = t[:, None] * np.exp(-np.log(float(max_period)) * np.arange(half) / half)[None, :]
        out[:, :half] = np.cos(arg)
        out[:, half:2 * half] = np.sin(arg)
    return out


def im2col(x: np.ndarray, kw: int, kh: int, s0: int, s1: int, p0: int, p1: int, d0: int, d1: int, is_2d: bool = True, dtype: str = "f32") -> np.ndarray:
    """2-D: x (N, IC, IH, IW) -> (N, OH, OW, IC*KH*KW); 1-D: x (N, IC, IW) -> (1, N, OW, IC*KW).  K order (ic, kh, kw), kw fastest; zero outside the image."""
    x = np.asarray(x, dtype=np.float32)
    if not is_2d:
        n, ic, iw = as4(x).shape[1:]
        x = as4(x).reshape(n, ic, 1, iw)
        kh, s1, p1, d1 = 1, 1, 0, 1
    N, IC, IH, IW = x.shape
    OW = (IW + 2 * p0 - d0 * (kw - 1) - 1) // s0 + 1
    OH = (IH + 2 * p1 - d1 * (kh - 1) - 1) // s1 + 1
    out = np.zeros((N, OH, OW, IC, kh, kw), dtype=np.float32)
    for oh in range(OH):
        for ow in range(OW):
            for ikh in range(kh):
                for ikw in range(kw):
                    ih, iw_ = oh * s1 + ikh * d1 - p1, ow * s0 + ikw * d0 - p0
                    if 0 <= ih < IH and 0 <= iw_ < IW:
                        out[:, oh, ow, :, ikh, ikw] = x[:, :, ih, iw_]
    out = round_to(out.reshape(N, OH, OW, IC * kh * kw), dtype)
    return out if is_2d else out.reshape(1, N, OW, IC * kw)


def assert_same_bits(out: np.ndarray, ref: np.ndarray, nan_bits: bool = False) -> None:
    """float32 arrays equal bit for bit (the sign of a zero included); a NaN matches any NaN unless nan_bits asks for its sign and payload too"""
    out, ref = np.ascontiguousarray(out, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert out.size == ref.size, (out.shape, ref.shape)
    o, r = out.reshape(-1), ref.reshape(-1)
    on, rn = np.isnan(o), np.isnan(r)
    bad = (on != rn) | ((~on | nan_bits) & (o.view(np.uint32) != r.view(np.uint32)))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{int(bad.sum())} of {o.size} elements differ; first at flat index {i}: got {o[i]!r} ({o.view(np.uint32)[i]:#010x}), want {r[i]!r} ({r.view(np.uint32)[i]:#010x})")
