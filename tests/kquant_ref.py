"""q4_K / q5_K / q6_K in plain NumPy: the super-block layouts packed from their fields, and ggml's dequantize_row_q{4,5,6}_K in float32, operations in its order
and each rounded on its own (d1 = d * sc; m1 = dmin * m; y = d1 * q - m1;  q6_K: y = (d * sc) * q).  Every backend route multiplies by w16 = f16(y).
Fields of nb super-blocks: d, dmin f16 [nb]; q4_K / q5_K: sc, mn 0 .. 63 [nb, 8], q 0 .. 15 / 31 [nb, 256]; q6_K: sc int8 [nb, 16] (mn, dmin unused), q -32 .. 31."""
import numpy as np

Q4_K, Q5_K, Q6_K = 12, 13, 14
TYPES = {"q4_K": Q4_K, "q5_K": Q5_K, "q6_K": Q6_K}
BLOCK_BYTES = {Q4_K: 144, Q5_K: 176, Q6_K: 210}
QMAX = {Q4_K: 15, Q5_K: 31}


def pack(wtype, d, dmin, sc, mn, q) -> np.ndarray:
    """-> uint8 [nb, BLOCK_BYTES] (ggml-common.h block_q4_K / block_q5_K / block_q6_K)"""
    nb = len(d)
    d2 = np.asarray(d, np.float16).reshape(nb, 1).view(np.uint8)
    if wtype == Q6_K:
        v = (np.asarray(q, np.int32) + 32).reshape(nb, 2, 4, 32)          # weight 128 half + 32 c + l
        ql = (v[:, :, 0:2] & 15) | ((v[:, :, 2:4] & 15) << 4)              # ql[64 half + 32 (c & 1) + l]: low nibble c < 2, high nibble c >= 2
        qh = sum((v[:, :, c] >> 4) << (2 * c) for c in range(4))            # qh[32 half + l]: bits 2 c .. 2 c + 1
        return np.concatenate([ql.reshape(nb, 128), qh.reshape(nb, 64), np.asarray(sc, np.int8).view(np.uint8).reshape(nb, 16), d2], axis=1).astype(np.uint8)
    sc, mn = np.asarray(sc, np.uint8), np.asarray(mn, np.uint8)
    s12 = np.concatenate([sc[:, :4] | ((sc[:, 4:] >> 4) << 6), mn[:, :4] | ((mn[:, 4:] >> 4) << 6), (sc[:, 4:] & 15) | ((mn[:, 4:] & 15) << 4)], axis=1)
    v = np.asarray(q, np.int32).reshape(nb, 4, 2, 32)                        # weight 64 g + 32 part + l: low / high nibble of qs[32 g + l]
    qs = ((v[:, :, 0] & 15) | ((v[:, :, 1] & 15) << 4)).reshape(nb, 128)
    head = [d2, np.asarray(dmin, np.float16).reshape(nb, 1).view(np.uint8), s12]
    if wtype == Q5_K:                                                        # qh[l]: bit j = fifth bit of weight l of sub-block j
        head.append(sum(((v.reshape(nb, 8, 32)[:, j] >> 4) & 1) << j for j in range(8)))
    return np.concatenate(head + [qs], axis=1).astype(np.uint8)


def dequant(wtype, d, dmin, sc, mn, q) -> np.ndarray:
    """-> float32 [nb, 256], ggml's operation order"""
    nb = len(d)
    d = np.asarray(d, np.float16).astype(np.float32)
    if wtype == Q6_K:
        s = np.repeat(np.asarray(sc, np.float32).reshape(nb, 2, 4, 2), 16, axis=3)       # scale index 8 half + 2 c + l // 16
        return ((d[:, None, None, None] * s) * np.asarray(q, np.float32).reshape(nb, 2, 4, 32)).reshape(nb, 256)
    d1 = d[:, None] * np.asarray(sc, np.float32)
    m1 = np.asarray(dmin, np.float16).astype(np.float32)[:, None] * np.asarray(mn, np.float32)
    return (d1[:, :, None] * np.asarray(q, np.float32).reshape(nb, 8, 32) - m1[:, :, None]).reshape(nb, 256)


def random_fields(rng, wtype, nb, d, dmin):
    """every scale value (>= 32 in sub-blocks 4 .. 7 included: the first four super-blocks take the extremes), negative q6_K scales, every quant value"""
    if wtype == Q6_K:
        sc = rng.integers(-128, 128, (nb, 16))
        sc[:2] = [[-128], [127]]
        return d, dmin, sc, np.zeros((nb, 8), np.int64), rng.integers(-32, 32, (nb, 256))
    sc, mn = rng.integers(0, 64, (nb, 8)), rng.integers(0, 64, (nb, 8))
    for i, (a, b) in enumerate([(63, 0), (0, 63), (63, 63), (32, 31)][:nb]):
        sc[i], mn[i] = a, b
    return d, dmin, sc, mn, rng.integers(0, QMAX[wtype] + 1, (nb, 256))
