"""K-quant Linear weights on the host: decoders against tests/kquant_ref.py bit for bit, the plain encoders' round trip, a GGUF tensor of the parameter's K type arriving raw."""
import ctypes as C

import numpy as np
import pytest

import kquant_ref as KQ
from test_model_io import _write_gguf

TYPES = sorted(KQ.TYPES.items())


def _dequantize_rows(L, gtype, raw: np.ndarray, n_per_row: int) -> np.ndarray:
    rows = raw.size // L.ggml_row_size(gtype, n_per_row)
    out = np.empty((rows, n_per_row), np.float32)
    buf = np.ascontiguousarray(raw).reshape(rows, -1)
    for r in range(rows):
        L.ggml_dequantize_row(gtype, buf[r].ctypes.data_as(C.c_void_p), out[r].ctypes.data_as(C.c_void_p), n_per_row)
    return out


@pytest.mark.parametrize("name,gtype", TYPES)
def test_dequantize_row_equals_the_numpy_restatement(sd, name, gtype):
    L, rng, nb = sd.lib(), np.random.default_rng(gtype), 64
    assert L.ggml_blck_size(gtype) == 256 and L.ggml_type_size(gtype) == KQ.BLOCK_BYTES[gtype] and L.ggml_row_size(gtype, 768) == 3 * KQ.BLOCK_BYTES[gtype]
    any_f16 = lambda: (rng.integers(0, 0x7C00, nb).astype(np.uint16) | (rng.integers(0, 2, nb).astype(np.uint16) << 15)).view(np.float16)   # every finite value
    f = KQ.random_fields(rng, gtype, nb, any_f16(), any_f16())
    got = _dequantize_rows(L, gtype, KQ.pack(gtype, *f), 256 * nb)
    with np.errstate(over="ignore", invalid="ignore"):
        want = KQ.dequant(gtype, *f)
    assert np.array_equal(got.view(np.uint32).ravel(), want.view(np.uint32).ravel())


@pytest.mark.parametrize("name,gtype", TYPES)
def test_quantize_chunk_round_trips_within_one_step(sd, name, gtype):
    """a smooth row (a slowly modulated wave with one period per 16 weights: every sub-block spans both signs) comes back within one quantisation step of each
    sub-block, the step of the encoder's own grid: (max - min) / 15 (q4_K), / 31 (q5_K) over 32 weights, / 63 (q6_K) over 16"""
    L, n = sd.lib(), 1024
    i = np.arange(n)
    x = ((1.0 + 0.5 * np.sin(2 * np.pi * i / n)) * np.sin(2 * np.pi * i / 16 + 0.3)).astype(np.float32)[None, :].repeat(2, axis=0).copy()
    out = np.zeros(2 * L.ggml_row_size(gtype, n), np.uint8)
    assert L.ggml_quantize_chunk(gtype, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 0, 2, n, None) == out.size
    back = _dequantize_rows(L, gtype, out, n)
    sub, levels = (16, 63) if gtype == KQ.Q6_K else (32, KQ.QMAX[gtype])
    xs = x.reshape(2, -1, sub)
    step = (xs.max(axis=2) - xs.min(axis=2)) / levels
    err = np.abs(back.reshape(xs.shape) - xs).max(axis=2)
    print(name, "largest error / step:", float((err / step).max()))
    assert (err <= step).all()


@pytest.mark.parametrize("name,gtype", TYPES)
def test_gguf_tensor_of_the_parameters_k_type_arrives_raw(sd, oracle, tmp_path, name, gtype):
    """wtype = the K type: the 256-wide Linear is declared in it, and the file's super-blocks (random fields no encoder would produce) decode to exactly the
    NumPy values — nothing was decoded and re-encoded on the way"""
    e = sd.Engine(model=sd.SD15_TINY, backend=oracle, wtype=gtype)
    n = "model.diffusion_model.input_blocks.4.1.transformer_blocks.0.ff.net.2.weight"   # [256, 64]
    ne, pty, _ = e.tensor_info(n)
    assert pty == gtype and int(ne[0]) == 256
    rng, nb = np.random.default_rng(7 + gtype), int(ne[1])
    d = (rng.integers(1, 64, nb) / 1024).astype(np.float16)
    f = KQ.random_fields(rng, gtype, nb, d, d[::-1].copy())
    _write_gguf(tmp_path / "k.gguf", [(n, gtype, [256, nb], KQ.pack(gtype, *f).tobytes())])
    assert e.load_weights(tmp_path / "k.gguf")["loaded"] == 1
    assert np.array_equal(e.get_tensor(n).ravel(), KQ.dequant(gtype, *f).ravel())
