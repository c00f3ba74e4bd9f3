"""q4_1 / q5_0 / q5_1 / iq4_nl Linear weights on the host: decoders against tests/bquant_ref.py bit for bit, the encoders' round trip, a GGUF tensor of the
parameter's own type arriving raw."""
import ctypes as C

import numpy as np
import pytest

import bquant_ref as BQ
from test_model_io import _write_gguf

TYPES = sorted(BQ.TYPES.items())


def _dequantize_rows(L, gtype, raw: np.ndarray, n_per_row: int) -> np.ndarray:
    rows = raw.size // L.ggml_row_size(gtype, n_per_row)
    out = np.empty((rows, n_per_row), np.float32)
    buf = np.ascontiguousarray(raw).reshape(rows, -1)
    for r in range(rows):
        L.ggml_dequantize_row(gtype, buf[r].ctypes.data_as(C.c_void_p), out[r].ctypes.data_as(C.c_void_p), n_per_row)
    return out


@pytest.mark.parametrize("name,gtype", TYPES)
def test_dequantize_row_equals_the_numpy_restatement(sd, name, gtype):
    L, rng, nb = sd.lib(), np.random.default_rng(gtype), 256
    assert L.ggml_blck_size(gtype) == 32 and L.ggml_type_size(gtype) == BQ.BLOCK_BYTES[gtype] and L.ggml_row_size(gtype, 320) == 10 * BQ.BLOCK_BYTES[gtype]
    any_f16 = lambda: (rng.integers(0, 0x7C00, nb).astype(np.uint16) | (rng.integers(0, 2, nb).astype(np.uint16) << 15)).view(np.float16)   # every finite value
    f = any_f16(), any_f16(), rng.integers(0, BQ.QMAX[gtype] + 1, (nb, 32))
    got = _dequantize_rows(L, gtype, BQ.pack(gtype, *f), 32 * nb)
    with np.errstate(over="ignore", invalid="ignore"):
        want = BQ.dequant(gtype, *f)
    assert np.array_equal(got.view(np.uint32).ravel(), want.view(np.uint32).ravel())


@pytest.mark.parametrize("name,gtype", TYPES)
def test_quantize_chunk_round_trips_within_half_a_step(sd, name, gtype):
    """Blocks on a grid that makes the encoder's d exactly s = 2^-e (so the bound is sharp, no f16 rounding of d or m in it): q4_1 / q5_1 values m + s u / 4
    spanning exactly QMAX steps, q5_0 values s u / 4 in -16 s .. 15.5 s with one at -16 s, iq4_nl values s u in -127 s .. 113 s with one at -127 s; every second
    block negated (q5_0 / iq4_nl: the maximum then has the other sign, d < 0).  |x - dequantize(quantize(x))| <= |d| / 2; iq4_nl: half the table's largest gap, 12 |d|."""
    L, rng, nb = sd.lib(), np.random.default_rng(100 + gtype), 64
    s = (2.0 ** -rng.integers(2, 9, nb)).astype(np.float32)[:, None]
    if gtype in (BQ.Q4_1, BQ.Q5_1):
        u = rng.integers(0, 4 * BQ.QMAX[gtype] + 1, (nb, 32))
        u[:, 3], u[:, 20] = 0, 4 * BQ.QMAX[gtype]
        x = s * rng.integers(-40, 40, (nb, 1)) + s * u / 4
    elif gtype == BQ.Q5_0:
        u = rng.integers(-64, 63, (nb, 32))
        u[:, 20] = -64
        x = s * u / 4
    else:
        u = rng.integers(-127, 114, (nb, 32))
        u[:, 20] = -127
        x = s * u
    x[1::2] *= -1 if gtype in (BQ.Q5_0, BQ.IQ4_NL) else 1
    x = np.ascontiguousarray(x.astype(np.float32).reshape(2, -1))
    out = np.zeros(2 * L.ggml_row_size(gtype, x.shape[1]), np.uint8)
    assert L.ggml_quantize_chunk(gtype, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), 0, 2, x.shape[1], None) == out.size
    d = out.reshape(nb, -1)[:, :2].copy().view(np.float16).astype(np.float32)
    assert np.array_equal(np.abs(d), s), "the encoder's d is the grid's step"
    err = np.abs(_dequantize_rows(L, gtype, out, x.shape[1]).reshape(nb, 32) - x.reshape(nb, 32))
    print(name, "largest error / |d|:", float((err / s).max()))
    assert (err <= (12.0 if gtype == BQ.IQ4_NL else 0.5) * s).all()


@pytest.mark.parametrize("name,gtype", TYPES)
def test_gguf_tensor_of_the_parameters_type_arrives_raw(sd, oracle, tmp_path, name, gtype):
    """wtype = the block type: the 256-wide Linear is declared in it, and the file's blocks (random fields no encoder would produce) decode to exactly the
    NumPy values — nothing was decoded and re-encoded on the way"""
    e = sd.Engine(model=sd.SD15_TINY, backend=oracle, wtype=gtype)
    n = "model.diffusion_model.input_blocks.4.1.transformer_blocks.0.ff.net.2.weight"   # [256, 64]
    ne, pty, _ = e.tensor_info(n)
    assert pty == gtype and int(ne[0]) == 256
    rng, nb = np.random.default_rng(7 + gtype), int(ne[1]) * 8
    d = (rng.integers(1, 64, nb) / 1024).astype(np.float16)
    f = d, d[::-1].copy(), rng.integers(0, BQ.QMAX[gtype] + 1, (nb, 32))
    _write_gguf(tmp_path / "b.gguf", [(n, gtype, [256, nb // 8], BQ.pack(gtype, *f).tobytes())])
    assert e.load_weights(tmp_path / "b.gguf")["loaded"] == 1
    assert np.array_equal(e.get_tensor(n).ravel(), BQ.dequant(gtype, *f).ravel())
