"""q4_1 / q5_0 / q5_1 / iq4_nl in plain NumPy: the 32-weight block layouts packed from their fields, and ggml's dequantize_row_* in float32
(q4_1 / q5_1: q * d + m; q5_0: (q - 16) * d; iq4_nl: d * KVALUES[q]).  Every backend route multiplies by w16 = f16(y).
Fields of nb blocks: d, m f16 [nb] (m unused by q5_0 / iq4_nl); q [nb, 32] codes 0 .. QMAX."""
import numpy as np

Q4_1, Q5_0, Q5_1, IQ4_NL = 3, 6, 7, 20
TYPES = {"q4_1": Q4_1, "q5_0": Q5_0, "q5_1": Q5_1, "iq4_nl": IQ4_NL}
BLOCK_BYTES = {Q4_1: 20, Q5_0: 22, Q5_1: 24, IQ4_NL: 18}
QMAX = {Q4_1: 15, Q5_0: 31, Q5_1: 31, IQ4_NL: 15}
KVALUES = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float32)


def pack(wtype, d, m, q) -> np.ndarray:
    """-> uint8 [nb, BLOCK_BYTES]: element j in the low nibble of qs[j], element j + 16 in the high; fifth bit of element e = bit e of the little-endian u32 qh"""
    nb = len(d)
    q = np.asarray(q, np.uint32).reshape(nb, 32)
    parts = [np.asarray(d, np.float16).reshape(nb, 1).view(np.uint8)]
    if wtype in (Q4_1, Q5_1):
        parts.append(np.asarray(m, np.float16).reshape(nb, 1).view(np.uint8))
    if wtype in (Q5_0, Q5_1):
        parts.append((((q >> 4) & 1) << np.arange(32, dtype=np.uint32)).sum(axis=1).astype("<u4").reshape(nb, 1).view(np.uint8))
    parts.append(((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8))
    return np.concatenate(parts, axis=1)


def dequant(wtype, d, m, q) -> np.ndarray:
    """-> float32 [nb, 32]"""
    d = np.asarray(d, np.float16).astype(np.float32)[:, None]
    q = np.asarray(q).reshape(len(d), 32)
    if wtype == IQ4_NL:
        return d * KVALUES[q]
    if wtype == Q5_0:
        return (q.astype(np.float32) - np.float32(16)) * d
    return q.astype(np.float32) * d + np.asarray(m, np.float16).astype(np.float32)[:, None]
