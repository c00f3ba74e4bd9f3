"""q2_K / q3_K Linear weights on the host: decoders against tests/kquant_low_ref.py bit for bit, the plain encoders' round trip, a GGUF tensor of the parameter's type arriving raw."""
import ctypes as C

import numpy as np
import pytest

import kquant_low_ref as KQ
from test_kquant_cpu import _dequantize_rows
from test_model_io import _write_gguf

TYPES = pytest.mark.parametrize("gtype", sorted(KQ.TYPES.values()), ids=sorted(KQ.TYPES))


@TYPES
def test_dequantize_row_equals_the_numpy_restatement(sd, gtype):
    L, rng, nb = sd.lib(), np.random.default_rng(gtype), 64
    assert L.ggml_blck_size(gtype) == 256 and L.ggml_type_size(gtype) == KQ.BLOCK_BYTES[gtype] and L.ggml_row_size(gtype, 768) == 3 * KQ.BLOCK_BYTES[gtype]
    any_f16 = lambda: (rng.integers(0, 0x7C00, nb).astype(np.uint16) | (rng.integers(0, 2, nb).astype(np.uint16) << 15)).view(np.float16)   # every finite value
    f = KQ.random_fields(rng, gtype, nb, any_f16(), any_f16())
    got = _dequantize_rows(L, gtype, KQ.pack(gtype, *f), 256 * nb)
    with np.errstate(over="ignore", invalid="ignore"):
        want = KQ.dequant(gtype, *f)
    assert np.array_equal(got.view(np.uint32).ravel(), want.view(np.uint32).ravel())


@TYPES
def test_quantize_chunk_round_trips_within_one_step(sd, gtype):
    """the smooth row of tests/test_kquant_cpu.py (every 16-weight sub-block spans both signs) comes back within one step of the encoder's own grid per sub-block:
    q2_K (max - min) / 3; q3_K |x|max / 4 — its rule puts the absolute maximum on code -4, so the other sign clips at 3 steps, an error of up to one step"""
    L, n = sd.lib(), 1024
    i = np.arange(n)
    x = ((1.0 + 0.5 * np.sin(2 * np.pi * i / n)) * np.sin(2 * np.pi * i / 16 + 0.3)).astype(np.float32)[None, :].repeat(2, axis=0).copy()
    out = np.zeros(2 * L.ggml_row_size(gtype, n), np.uint8)
    assert L.ggml_quantize_chunk(gtype, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 0, 2, n, None) == out.size
    xs = x.reshape(2, -1, 16)
    step = (xs.max(axis=2) - xs.min(axis=2)) / 3 if gtype == KQ.Q2_K else np.abs(xs).max(axis=2) / 4
    err = np.abs(_dequantize_rows(L, gtype, out, n).reshape(xs.shape) - xs).max(axis=2)
    print("largest error / step:", float((err / step).max()))
    assert (err <= step).all()


@TYPES
def test_gguf_tensor_of_the_parameters_type_arrives_raw(sd, oracle, tmp_path, gtype):
    """wtype = the type: the 256-wide Linear is declared in it, and the file's super-blocks (random fields no encoder would produce) decode to exactly the NumPy values"""
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
