"""MXFP4 in plain NumPy: block_mxfp4 {u8 e; u8 qs[16]} packed from its fields, and ggml's dequantize_row_mxfp4 in float32: y = KVALUES[q] * d,
d = GGML_E8M0_TO_FP32_HALF(e) = 2^(e - 128) (f32 bits 0x00200000 << e below e = 2, else (e - 1) << 23).  Every backend route multiplies by w16 = f16(y).
Fields of nb blocks: e [nb] 0 .. 255; q [nb, 32] codes 0 .. 15."""
import numpy as np

MXFP4, BLOCK_BYTES = 39, 17
KVALUES = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], np.float32)


def pack(e, q) -> np.ndarray:
    """-> uint8 [nb, 17]: element j in the low nibble of qs[j], element j + 16 in the high"""
    q = np.asarray(q, np.uint8).reshape(len(e), 32)
    return np.concatenate([np.asarray(e, np.uint8).reshape(-1, 1), (q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)], axis=1)


def dequant(e, q) -> np.ndarray:
    """-> float32 [nb, 32]"""
    e = np.asarray(e, np.uint32)
    d = np.where(e < 2, np.uint32(0x00200000) << e, (np.maximum(e, 1) - 1) << np.uint32(23)).astype(np.uint32).view(np.float32)
    with np.errstate(over="ignore"):   # 12 * 2^125 and up: inf
        return KVALUES[np.asarray(q).reshape(len(e), 32)] * d[:, None]
