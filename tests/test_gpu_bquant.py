"""q4_1 / q5_0 / q5_1 / iq4_nl Linear weights on the product backend (kernels/bquant.hip): ONE Linear through the C ABI per test, its weight tensor created in the
block type from raw blocks (tests/bquant_ref.py), bit for bit.  Decode: x is the identity, so the output transposed must equal w16 = f16(ggml's dequantised value) on
random blocks, on every route; M = 8 rows of 22 / 18 bytes (K = 32) start at all eight even 16-byte phases.  Integer data: d in {1/2, 1}, m a multiple of d, x in
-4 .. 4, partial sums asserted below 2^24 units.  Behind SiLU / GEGLU: linear_ref's transcendental bar.  The lin_bq_* counters move as the case says, lin_kq_* /
lin_qgemv* / lin_qgemm16* / lin_wswz_q not at all (not asserted under SDCPP_BACKEND_OPTS; the CPU oracle has no MUL_MAT over these types)."""
import os

import numpy as np
import pytest

import bquant_ref as BQ
import linear_ref as R
from ggml_graph import F16, F32, Graph, tensor_struct

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") == "1", reason="the CPU oracle has no MUL_MAT over these block types")]
TYPES = sorted(BQ.TYPES.items())
DEFAULTS = {"qgemm16": 1, "jit_qimages": 4096}
WATCHED = ("lin_bq", "bquant_linears", "lin_kq", "kquant_linears", "lin_geglu", "lin_qgemv", "lin_qgemm16", "lin_wswz_q", "fused_presilu", "jit_images", "generic_matmul")
MAX_ROWS = 512   # k_bq_gemm's range (bq_gemm_max_rows); one row above it the image route


def run_linear(sd, gpu, gtype, blocks, M, K, x, opts, routes, epi="none", extra=None, batch=1):
    """blocks: uint8 [M * K / 32, block bytes]; x [rows, K]; -> out [rows, columns]; asserts the counters"""
    L, e = sd.lib(), extra or {}
    try:
        for k, v in opts.items():
            sd.backend_set_option(k, v)
        before = sd.backend_stats()
        with Graph(gpu) as g:
            w = L.ggml_new_tensor_2d(g.wctx, gtype, K, M)
            g._weights.append((w, blocks.tobytes()))
            rows = x.shape[0]
            xi = g.input(x.reshape(batch, rows // batch, K) if batch > 1 else x)
            shp = lambda a: a.reshape(batch, rows // batch, -1) if batch > 1 else a
            if epi == "presilu":
                xi = L.ggml_silu(g.ctx, xi)
            y = L.ggml_mul_mat(g.ctx, w, xi)
            if "bias" in e:
                y = L.ggml_add_inplace(g.ctx, y, g.weight(e["bias"], F32))
            if epi == "bias+res":
                y = L.ggml_add(g.ctx, y, g.input(shp(e["residual"])))
            elif epi == "gate":
                y = L.ggml_add(g.ctx, g.input(shp(e["residual"])), L.ggml_mul(g.ctx, y, g.input(e["gate"].reshape(batch, 1, M))))
            elif epi == "geglu":
                s = tensor_struct(y)
                ne, nb = [int(s.ne[i]) for i in range(4)], [int(s.nb[i]) for i in range(4)]
                lo = L.ggml_view_4d(g.ctx, y, M // 2, ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], 0)
                hi = L.ggml_view_4d(g.ctx, y, M // 2, ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], M // 2 * 4)
                h = L.ggml_mul(g.ctx, lo, L.ggml_gelu_inplace(g.ctx, L.ggml_cont(g.ctx, hi)))
                y = L.ggml_mul_mat(g.ctx, g.weight(np.eye(M // 2, dtype=np.float32), F16), h)
            out = g.run(y).reshape(rows, -1)
        after = sd.backend_stats()
    finally:
        for k in opts:
            sd.backend_set_option(k, DEFAULTS[k])
    if not os.environ.get("SDCPP_BACKEND_OPTS"):
        moved = {f: after[f] - before[f] for f in after if f.startswith(WATCHED) and after[f] != before[f]}
        assert moved == {**routes, "bquant_linears": 1}, f"counters moved {moved}, expected {routes}"
    return out, after["swizzled_weight_bytes"] - before["swizzled_weight_bytes"]


ROUTES = {"kernel": ({}, None), "cached-image": ({"qgemm16": 0}, {"lin_bq_image": 1}), "jit-image": ({"qgemm16": 0, "jit_qimages": 1}, {"lin_bq_image": 1, "jit_images": 1})}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("K", (32, 288))   # one short segment alone (32 rows: 32-row tiles); a full segment and a one-block tail (288 rows: 64-row tiles)
@pytest.mark.parametrize("name,gtype", TYPES)
def test_decode_one_hot(sd, gpu, name, gtype, K, route):
    rng, M = np.random.default_rng(K + gtype), 8
    nb = M * K // 32
    f = (rng.integers(1, 64, nb) / 1024).astype(np.float16), (rng.integers(-63, 64, nb) / 1024).astype(np.float16), rng.integers(0, BQ.QMAX[gtype] + 1, (nb, 32))
    opts, routes = ROUTES[route]
    out, cached = run_linear(sd, gpu, gtype, BQ.pack(gtype, *f), M, K, np.eye(K, dtype=np.float32), opts, routes or {"lin_bq_gemm_rb1" if K == 32 else "lin_bq_gemm_rb2": 1})
    assert cached == (128 * ((K + 63) // 64 * 64) * 2 if route == "cached-image" else 0), "only the cached route keeps an image (8 rows padded to 128, K to 64)"
    want = BQ.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float32)
    assert np.isfinite(want).all()
    bad = np.argwhere(out.T != want)
    assert len(bad) == 0, f"{len(bad)} weights differ; first (column, k) = {tuple(bad[0])}: got {out.T[tuple(bad[0])]!r}, w16 {want[tuple(bad[0])]!r}"


def integer_fields(rng, gtype, M, K, small=False, one_block_per_row=False):
    """d in {1/2, 1} per block (small: 2^-9, GEGLU pre-activations of a few units), m = d * (-8 .. 8); one_block_per_row: d = m = 0 in every other block"""
    nb = M * K // 32
    d = (np.full(nb, 2.0 ** -9) if small else rng.choice([0.5, 1.0], nb)).astype(np.float16)
    if not small:
        d[:2] = 1.0, 0.5
    if one_block_per_row:
        live = np.arange(M) * (K // 32) + (np.arange(M) * 5) % (K // 32)
        keep = np.zeros(nb, bool)
        keep[live] = True
        d[~keep] = 0
    m = (d * rng.integers(-8, 9, nb)).astype(np.float16) if gtype in (BQ.Q4_1, BQ.Q5_1) else np.zeros(nb, np.float16)
    return d, m, rng.integers(0, BQ.QMAX[gtype] + 1, (nb, 32))


# (id, rows, K, M, epilogue, lin_bq_* moves).  Tiles: 32 rows (1 .. 32) / 64 rows; 128 columns, 4 waves x 32 (M = 8: a partial tile, three waves with no column);
# segments of 256 k (288 = a full one and a one-block tail); 1 .. 4 rows are staged from f32, 5 and more come from the f16 operand image; the K slices are
# min(512 / tiles, segments / 2) >= 2: K = 768 (3 segments) does not split, K = 800 (4) is the smallest that does
CASES = [("1-row", 1, 288, 8, "none", {"lin_bq_gemm_rb1": 1}), ("2-rows", 2, 288, 160, "none", {"lin_bq_gemm_rb1": 1}),
         ("4-rows", 4, 320, 160, "none", {"lin_bq_gemm_rb1": 1}), ("5-rows", 5, 320, 160, "none", {"lin_bq_gemm_rb1": 1}),
         ("32-rows", 32, 32, 160, "none", {"lin_bq_gemm_rb1": 1}), ("33-rows", 33, 288, 160, "none", {"lin_bq_gemm_rb2": 1}),
         ("last-row", MAX_ROWS, 288, 8, "none", {"lin_bq_gemm_rb2": 1}), ("above-image", MAX_ROWS + 1, 32, 160, "none", {"lin_bq_image": 1}),
         ("no-split", 2, 768, 8, "bias", {"lin_bq_gemm_rb1": 1}), ("split-k", 2, 800, 8, "bias", {"lin_bq_gemm_rb1": 1, "lin_bq_gemm_reduce": 1}),
         ("bias+res", 33, 288, 160, "bias+res", {"lin_bq_gemm_rb2": 1}), ("gate", 66, 96, 160, "gate", {"lin_bq_gemm_rb2": 1}),
         ("presilu", 1, 288, 160, "presilu", {"lin_bq_gemm_rb1": 1, "fused_presilu": 1}),   # SiLU applied by k_bq_gemm while it stages the row
         ("geglu-pairs", 64, 288, 256, "geglu", {"lin_bq_image": 1, "lin_geglu_pair": 1})]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("name,gtype", TYPES)
def test_integer_linear(sd, gpu, name, gtype, case):
    """presilu: iq4_nl has no zero code, so a row's weights are one live BLOCK (d = 0 elsewhere) and the bar is linear_ref's, summed: every image value
    silu(x_k) carries transcendental_terms(silu(x_k), x_k), its exact product |w_k| times that, and the f32 sum of the <= 32 products adds at most
    32 * 2^-24 * sum |w_k silu(x_k)|."""
    cid, rows, K, M, epi, routes = case
    rng = np.random.default_rng(rows * 7 + K + gtype)
    small = epi == "geglu"
    f = integer_fields(rng, gtype, M, K, small=small, one_block_per_row=epi == "presilu")
    w = BQ.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float32)
    unit = 2.0 ** -9 if small else 0.5
    assert np.array_equal(w / unit, np.rint(w / unit)) and np.abs(w / unit).max() < R.F16_EXACT
    x = R.ints(rng, -1, 1, (rows, K)) if small else R.ints(rng, -4, 4, (rows, K))
    batch = 2 if epi == "gate" else 1
    extra = {}
    if epi in ("bias", "bias+res", "gate", "geglu"):
        extra["bias"] = R.nonzero_ints(rng, -1 if small else -64, 1 if small else 64, (M,))
    if epi in ("bias+res", "gate"):
        extra["residual"] = R.ints(rng, -8, 8, (rows, M))
    if epi == "gate":
        extra["gate"] = R.nonzero_ints(rng, -2, 2, (batch, M))
    bound = (float(np.abs(x).max()) * float(np.abs(w).astype(np.float64).sum(axis=1).max()) + 2 * (64 + 8)) / unit
    assert epi == "presilu" or bound < R.EXACT_BOUND, f"partial sums up to {bound} units"
    out, _ = run_linear(sd, gpu, gtype, BQ.pack(gtype, *f), M, K, x, {}, routes, epi=epi, extra=extra, batch=batch)
    want, p = R.linear_ref(x, w, "f16", epi=epi, bias=extra.get("bias"), residual=extra.get("residual"), gate=extra.get("gate"), batches=batch)
    if epi in ("presilu", "geglu"):
        if epi == "presilu":
            aw = np.abs(w).astype(np.float64).T
            bar = sum(R.transcendental_terms(R.silu64(p), p)) @ aw + 32 * 2.0 ** -24 * (np.abs(R.silu64(p)) @ aw)
        else:
            assert float(np.abs(want).max()) < R.F16_MAX / 2
            bar = sum(R.transcendental_terms(want, p[1], np.maximum(1.0, np.abs(p[0]))))
        err = np.abs(out.astype(np.float64) - want)
        print(f"{name} {cid}: largest |error| / bar = {float((err / bar).max()):.3f}")
        assert (err <= bar).all()
    else:
        w32 = want.astype(np.float32)
        bad = np.argwhere(out != w32)
        assert len(bad) == 0, f"{len(bad)} of {w32.size} differ; first (row, column) = {tuple(bad[0])}: got {out[tuple(bad[0])]!r}, reference {w32[tuple(bad[0])]!r}"


@pytest.mark.parametrize("name,gtype", TYPES)
def test_supports_op(sd, gpu, name, gtype):
    """whole blocks per row only: K = 32 is claimed, K = 48 (ne0 of a hand-made tensor: the front-end would not build it) is refused"""
    L = sd.lib()
    with Graph(gpu) as g:
        node = L.ggml_mul_mat(g.ctx, L.ggml_new_tensor_2d(g.wctx, gtype, 32, 8), g.input(np.zeros((2, 32), np.float32)))
        assert g.supports(node)
        sd.backend_set_option("mfma_gemm", 0)   # the Linear path is off: there is no other kernel for these blocks
        try:
            assert not g.supports(node)
        finally:
            sd.backend_set_option("mfma_gemm", 1)
        tensor_struct(tensor_struct(node).src[0]).ne[0] = 48
        tensor_struct(tensor_struct(node).src[1]).ne[0] = 48
        assert not g.supports(node)


@pytest.mark.parametrize("name,gtype", TYPES)
def test_weight_outside_a_weights_buffer_fails_the_graph(sd, gpu, name, gtype):
    """supports_op cannot see the buffer: a MUL_MAT operand of these types that is not a static weight never reaches the generic matmul, the plan fails loudly"""
    L = sd.lib()
    with Graph(gpu) as g:
        w = L.ggml_new_tensor_2d(g.ctx, gtype, 32, 8)
        L.ggml_set_input(w)
        g._inputs.append((w, bytes(8 * BQ.BLOCK_BYTES[gtype])))
        with pytest.raises(AssertionError, match="graph_compute status"):
            g.run(L.ggml_mul_mat(g.ctx, w, g.input(np.ones((2, 32), np.float32))))
