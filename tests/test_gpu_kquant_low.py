"""q2_K / q3_K Linear weights on the product backend (kernels/kquant.hip): the harness, routes and case table of tests/test_gpu_kquant.py with weights made from
raw super-blocks of tests/kquant_low_ref.py, bit for bit (K = 768: 252- / 330-byte rows, every 4- / 2-byte phase of a 16-byte granule).  Integer data: d = dmin in
{1/2, 1}, |w| <= 128 d, x in -4 .. 4, partial sums below linear_ref.EXACT_BOUND; behind SiLU / GEGLU linear_ref's transcendental bar."""
import os

import numpy as np
import pytest

import kquant_low_ref as KQ
import linear_ref as R
import test_gpu_kquant as G
from ggml_graph import Graph

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") == "1", reason="the CPU oracle has no K-quant MUL_MAT")]
TYPES = pytest.mark.parametrize("gtype", sorted(KQ.TYPES.values()), ids=sorted(KQ.TYPES))


@pytest.mark.parametrize("route", G.ROUTES)
@pytest.mark.parametrize("K", (256, 768))
@TYPES
def test_decode_one_hot(sd, gpu, gtype, K, route):
    """x = identity: the output transposed is w16 = f16(ggml's dequantised value) on every route; only the cached route keeps an image (160 rows padded to 256)"""
    rng, M = np.random.default_rng(K + gtype), 160
    nb = M * K // 256
    f = KQ.random_fields(rng, gtype, nb, (rng.integers(1, 64, nb) / 1024).astype(np.float16), (rng.integers(1, 64, nb) / 512).astype(np.float16))
    out, cached = G.run_linear(sd, gpu, gtype, KQ.pack(gtype, *f), M, K, np.eye(K, dtype=np.float32), *G.ROUTES[route])
    assert cached == (256 * K * 2 if route == "cached-image" else 0)
    want = KQ.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float32)
    bad = np.argwhere(out.T != want)
    assert len(bad) == 0, f"{len(bad)} weights differ; first (column, k) = {tuple(bad[0])}: got {out.T[tuple(bad[0])]!r}, w16 {want[tuple(bad[0])]!r}"


def integer_fields(rng, gtype, nb, one_per_row_of=None, small=False):
    """d = dmin in {1/2, 1} per super-block (small: 2^-9, scales <= 3: GEGLU pre-activations of a few units); one_per_row_of = K: a single weight 3 d per row"""
    d = (np.full(nb, 2.0 ** -9) if small else rng.choice([0.5, 1.0], nb)).astype(np.float16)
    if gtype == KQ.Q2_K:
        sc, mn, q = rng.integers(0, 4 if small else 16, (nb, 16)), rng.integers(0, 4 if small else 16, (nb, 16)), rng.integers(0, 4, (nb, 256))
    else:
        sc, mn, q = rng.integers(-3 if small else -32, 4 if small else 32, (nb, 16)), np.zeros((nb, 16), np.int64), rng.integers(-4, 4, (nb, 256))
    if one_per_row_of:
        sc, mn, q = np.ones_like(sc), np.zeros_like(mn), np.zeros_like(q)
        rows = np.arange(nb * 256 // one_per_row_of)
        pos = rows * one_per_row_of + (rows * 37) % one_per_row_of
        q[pos // 256, pos % 256] = 3
    return d, d, sc, mn, q


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c[0])
@TYPES
def test_integer_linear(sd, gpu, gtype, case):
    cid, rows, K, M, epi, opts, routes = case
    if cid in ("last-row-rb4", "last-row", "above-image"):   # the last row of the kernel's range (kq_gemm_supported); one row above it the image route
        rows += KQ.KERNEL_MAX_ROWS[gtype]
    if cid == "geglu-16-interleave" and sd.calibrate()["compute_units"] != 256:
        pytest.skip("the 16-column interleave is the default policy's choice for this shape on 256 CUs")
    rng, small, batch = np.random.default_rng(rows * 7 + K + gtype), epi == "geglu", 2 if epi == "gate" else 1
    f = integer_fields(rng, gtype, M * K // 256, one_per_row_of=K if epi == "presilu" else None, small=small)
    w = KQ.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float32)
    unit = 2.0 ** -10 if small else 0.5
    assert np.array_equal(w / unit, np.rint(w / unit)) and np.abs(w.reshape(-1, 256) / f[0].astype(np.float32)[:, None]).max() <= 128
    x = R.ints(rng, -1, 1, (rows, K)) if small else R.ints(rng, -4, 4, (rows, K))
    extra = {}
    if epi in ("bias", "bias+res", "gate", "geglu"):
        extra["bias"] = R.nonzero_ints(rng, -1 if small else -64, 1 if small else 64, (M,))
    if epi in ("bias+res", "gate"):
        extra["residual"] = R.ints(rng, -8, 8, (rows, M))
    if epi == "gate":
        extra["gate"] = R.nonzero_ints(rng, -2, 2, (batch, M))
    bound = (float(np.abs(x).max()) * float(np.abs(w).astype(np.float64).sum(axis=1).max()) + 2 * (64 + 8)) / unit
    assert epi == "presilu" or bound < R.EXACT_BOUND, f"partial sums up to {bound} units"
    out, _ = G.run_linear(sd, gpu, gtype, KQ.pack(gtype, *f), M, K, x, opts, routes, epi=epi, extra=extra, batch=batch)
    want, p = R.linear_ref(x, w, "f16", epi=epi, bias=extra.get("bias"), residual=extra.get("residual"), gate=extra.get("gate"), batches=batch, fast=rows > 1000)
    if epi == "presilu":
        col = np.abs(w).argmax(axis=1)
        bar = sum(R.transcendental_terms(R.silu64(p[:, col]), p[:, col], np.abs(w).max(axis=1)[None, :]))
    elif epi == "geglu":
        assert float(np.abs(want).max()) < R.F16_MAX / 2
        bar = sum(R.transcendental_terms(want, p[1], np.maximum(1.0, np.abs(p[0]))))
    else:
        want, bar = want.astype(np.float32), 0.0   # bit for bit
    err = np.abs(out.astype(np.float64) - want)
    print(f"{cid}: largest |error| = {float(err.max())!r}, largest bar = {float(np.max(bar))!r}")
    assert (err <= bar).all(), f"{int((err > bar).sum())} of {err.size} outside the bar; first (row, column) = {tuple(np.argwhere(err > bar)[0])}"


@TYPES
def test_supports_op(sd, gpu, gtype):
    """K = 256 is claimed; refused with mfma_gemm = 0 and at a hand-set ne0 = 320: the existing test's body, on the two types"""
    G.test_supports_op(sd, gpu, None, gtype)


@TYPES
def test_weight_outside_a_weights_buffer_fails_the_graph(sd, gpu, gtype):
    """supports_op cannot see the buffer: a typed MUL_MAT operand that is not a static weight never reaches the generic matmul, the plan fails loudly"""
    L, before = sd.lib(), sd.backend_stats()["generic_matmul"]
    with Graph(gpu) as g:
        w = L.ggml_new_tensor_2d(g.ctx, gtype, 256, 8)
        L.ggml_set_input(w)
        g._inputs.append((w, bytes(8 * KQ.BLOCK_BYTES[gtype])))
        with pytest.raises(AssertionError, match="graph_compute status"):
            g.run(L.ggml_mul_mat(g.ctx, w, g.input(np.ones((2, 256), np.float32))))
    assert sd.backend_stats()["generic_matmul"] == before


@TYPES
def test_engine_unet_forward(sd, gpu, gtype):
    """SD15_TINY with wtype = the type: its 256-wide Linears run on the K-quant routes; correctness rests on the Linear-level tests above"""
    rng, before = np.random.default_rng(gtype), sd.backend_stats()["kquant_linears"]
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, wtype=gtype)
    out = e.unet_forward(rng.standard_normal((1, 4, 16, 16)).astype(np.float32), np.array([500.0], np.float32), rng.standard_normal((1, 77, 64)).astype(np.float32))
    assert np.isfinite(out).all() and sd.backend_stats()["kquant_linears"] > before
