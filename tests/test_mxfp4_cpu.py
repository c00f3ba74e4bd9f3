"""MXFP4 Linear weights on the host: type traits, the decoder against tests/mxfp4_ref.py bit for bit, the encoder, a GGUF tensor of type 39 arriving raw."""
import ctypes as C

import numpy as np
import pytest

import mxfp4_ref as MX
from test_bquant_cpu import _dequantize_rows
from test_model_io import _write_gguf


def _quantize(L, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros(x.shape[0] * L.ggml_row_size(MX.MXFP4, x.shape[1]), np.uint8)
    assert L.ggml_quantize_chunk(MX.MXFP4, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 0, x.shape[0], x.shape[1], None) == out.size
    return out


def test_traits_and_decoder_on_every_exponent_and_code(sd):
    L = sd.lib()
    name = C.CFUNCTYPE(C.c_char_p, C.c_int)(("ggml_type_name", L))
    assert L.ggml_blck_size(MX.MXFP4) == 32 and L.ggml_type_size(MX.MXFP4) == 17 and name(MX.MXFP4) == b"mxfp4"
    assert [L.ggml_row_size(MX.MXFP4, K) for K in (32, 320, 3072)] == [17 * K // 32 for K in (32, 320, 3072)]
    e, q = np.arange(256), np.tile(np.repeat(np.arange(16), 2), (256, 1))   # every code in a low and in a high nibble of every exponent
    got = _dequantize_rows(L, MX.MXFP4, MX.pack(e, q), 32 * 256)
    assert np.array_equal(got.view(np.uint32).ravel(), MX.dequant(e, q).view(np.uint32).ravel())


def test_encoder_round_trips_representable_blocks(sd):
    """values k * d with one of magnitude 8 or 12 per block, so that floor(log2(amax)) - 2 gives the block's own exponent back: bytes in = bytes out"""
    rng, nb = np.random.default_rng(39), 253   # (12 * 2^(e - 128) is finite in f32 up to e = 252)
    e, q = np.arange(nb), rng.integers(0, 16, (nb, 32))
    q[q == 8] = 0   # -0 encodes as code 0
    q[np.arange(nb), rng.integers(0, 32, nb)] = rng.choice([6, 7, 14, 15], nb)
    blocks = MX.pack(e, q)
    assert np.array_equal(_quantize(sd.lib(), MX.dequant(e, q).reshape(1, -1)).reshape(nb, 17), blocks)


def test_encoder_error_on_normal_rows(sd):
    """v = x / d lies in (-16, 16) by the choice of e (amax / d in [8, 16)).  Inside the table's range the nearest entry is at most half the gap between the two
    entries around v away; above 12 the last code is taken and the error is |v| - 12 < 4, the last gap."""
    L, rng = sd.lib(), np.random.default_rng(40)
    x = rng.standard_normal((4, 320)).astype(np.float32)
    raw = _quantize(L, x)
    d = MX.dequant(raw.reshape(-1, 17)[:, 0], np.ones((40, 32), int))
    v, err = x.reshape(40, 32) / d, np.abs(_dequantize_rows(L, MX.MXFP4, raw, 320).reshape(40, 32) - x.reshape(40, 32)) / d
    T = np.unique(MX.KVALUES)
    i = np.searchsorted(T, v).clip(1, len(T) - 1)
    assert np.abs(v).max() < 16 and np.abs(v).max(axis=1).min() >= 8
    assert (err <= np.where(np.abs(v) <= 12, (T[i] - T[i - 1]) / 2, np.abs(v) - 12)).all()


def test_gguf_tensor_of_type_39_arrives_raw(sd, oracle, tmp_path):
    eng = sd.Engine(model=sd.SD15_TINY, backend=oracle, wtype=sd.MXFP4)
    n = "model.diffusion_model.input_blocks.4.1.transformer_blocks.0.ff.net.2.weight"   # [256, 64]
    ne, pty, _ = eng.tensor_info(n)
    assert pty == MX.MXFP4 and int(ne[0]) == 256
    rng, nb = np.random.default_rng(41), int(ne[1]) * 8
    e, q = rng.integers(0, 253, nb), rng.integers(0, 16, (nb, 32))   # fields no encoder would produce
    _write_gguf(tmp_path / "m.gguf", [(n, MX.MXFP4, [256, nb // 8], MX.pack(e, q).tobytes())])
    assert eng.load_weights(tmp_path / "m.gguf")["loaded"] == 1
    assert np.array_equal(eng.get_tensor(n).ravel(), MX.dequant(e, q).ravel())
