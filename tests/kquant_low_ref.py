"""q2_K / q3_K in plain NumPy, in the style of tests/kquant_ref.py: the super-block layouts packed from their fields, and ggml's dequantize_row_q{2,3}_K in float32,
operations in its order and each rounded on its own (q2_K: dl = d * sc; ml = dmin * mn; y = dl * q - ml;  q3_K: dl = d * sc; y = dl * q).
Fields of nb super-blocks: d, dmin f16 [nb]; q2_K: sc, mn 0 .. 15 [nb, 16], q 0 .. 3 [nb, 256]; q3_K: sc -32 .. 31 [nb, 16] (mn, dmin unused), q -4 .. 3 [nb, 256]
(the signed value: its low two bits go to qs, bit 2 of q + 4 to hmask).  Weight 128 hf + 32 c + l is bit pair c of qs[32 hf + l] and bit 4 hf + c of hmask[l]."""
import numpy as np

Q2_K, Q3_K = 10, 11
TYPES = {"q2_K": Q2_K, "q3_K": Q3_K}
BLOCK_BYTES = {Q2_K: 84, Q3_K: 110}
KERNEL_MAX_ROWS = {Q2_K: 512, Q3_K: 256}   # kq_gemm_supported at the default qgemm16_max_rows = 512: q3_K hands over at half of it (profiles/kquant_low_probe.txt)


def pack(wtype, d, dmin, sc, mn, q) -> np.ndarray:
    """-> uint8 [nb, BLOCK_BYTES] (ggml-common.h block_q2_K / block_q3_K)"""
    nb = len(d)
    d2 = np.asarray(d, np.float16).reshape(nb, 1).view(np.uint8)
    v = (np.asarray(q, np.int32) + (4 if wtype == Q3_K else 0)).reshape(nb, 2, 4, 32)
    qs = sum((v[:, :, c] & 3) << (2 * c) for c in range(4)).reshape(nb, 64)
    if wtype == Q2_K:
        return np.concatenate([np.asarray(sc) | (np.asarray(mn) << 4), qs, d2, np.asarray(dmin, np.float16).reshape(nb, 1).view(np.uint8)], axis=1).astype(np.uint8)
    hmask = sum((v[:, hf, c] >> 2) << (4 * hf + c) for hf in range(2) for c in range(4))
    s6 = np.asarray(sc, np.int32) + 32                                       # scale j: low 4 bits in byte j & 7 (high nibble for j >= 8), high 2 bits in byte 8 + (j & 3)
    s12 = np.concatenate([(s6[:, :8] & 15) | ((s6[:, 8:] & 15) << 4), sum((s6[:, 4 * g:4 * g + 4] >> 4) << (2 * g) for g in range(4))], axis=1)
    return np.concatenate([hmask, qs, s12, d2], axis=1).astype(np.uint8)


def dequant(wtype, d, dmin, sc, mn, q) -> np.ndarray:
    """-> float32 [nb, 256], ggml's operation order; sub-block scale of weight w: w // 16"""
    nb = len(d)
    dl = np.asarray(d, np.float16).astype(np.float32)[:, None] * np.asarray(sc, np.float32)
    y = dl[:, :, None] * np.asarray(q, np.float32).reshape(nb, 16, 16)
    if wtype == Q2_K:
        y = y - (np.asarray(dmin, np.float16).astype(np.float32)[:, None] * np.asarray(mn, np.float32))[:, :, None]
    return y.reshape(nb, 256)


def random_fields(rng, wtype, nb, d, dmin):
    """the first super-blocks take the scale extremes (q2_K: scale / min 15 / 0, 0 / 15, 15 / 15; q3_K: -32, 31, and high two bits that differ per j >> 2); every
    quant value and both states of every hmask bit position occur (256 nb random quants)"""
    if wtype == Q3_K:
        sc, mn = rng.integers(-32, 32, (nb, 16)), np.zeros((nb, 16), np.int64)
        sc[:3] = [np.full(16, -32), np.full(16, 31), 16 * (np.arange(16) >> 2) + np.arange(16) - 32][:nb]
    else:
        sc, mn = rng.integers(0, 16, (nb, 16)), rng.integers(0, 16, (nb, 16))
        sc[:3], mn[:3] = [[15], [0], [15]][:nb], [[0], [15], [15]][:nb]
    return d, dmin, sc, mn, rng.integers(-4 if wtype == Q3_K else 0, 4, (nb, 256))
