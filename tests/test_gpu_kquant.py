"""q4_K / q5_K / q6_K Linear weights on the product backend (kernels/kquant.hip): ONE Linear through the C ABI per test, its weight tensor created in the K
type from raw super-blocks (tests/kquant_ref.py), bit for bit.  Decode: x is the identity, so the output transposed must equal w16 = f16(ggml's dequantised value)
on random blocks, on every route (K = 768: 630-byte q6_K rows).  Integer data: d = dmin a power of two per super-block, |w| <= 2016 units, x in -4 .. 4, partial sums
asserted below 2^24 units.  Behind SiLU / GEGLU: linear_ref's transcendental bar.  The lin_kq_* counters move as the case says, lin_qgemv* / lin_qgemm16* /
lin_wswz_q not at all (not asserted under SDCPP_BACKEND_OPTS; the CPU oracle has no K-quant kernels)."""
import os

import numpy as np
import pytest

import kquant_ref as KQ
import linear_ref as R
from ggml_graph import F16, F32, Graph, tensor_struct

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") == "1", reason="the CPU oracle has no K-quant MUL_MAT")]
TYPES = sorted(KQ.TYPES.items())
DEFAULTS = {"qgemm16": 1, "jit_qimages": 4096, "qgemm16_rb": 3, "qgemm16_max_rows": 512}
WATCHED = ("lin_kq", "kquant_linears", "lin_geglu", "lin_qgemv", "lin_qgemm16", "lin_wswz_q", "fused_presilu", "jit_images", "generic_matmul")


def run_linear(sd, gpu, gtype, blocks, M, K, x, opts, routes, epi="none", extra=None, batch=1):
    """blocks: uint8 [M * K / 256, block bytes]; x [rows, K]; -> out [rows, columns]; asserts the counters"""
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
        assert moved == {**routes, "kquant_linears": 1}, f"counters moved {moved}, expected {routes}"
    return out, after["swizzled_weight_bytes"] - before["swizzled_weight_bytes"]


ROUTES = {"kernel-1": ({"qgemm16_max_rows": 1536}, {"lin_kq_gemm_rb2": 1}), "cached-image": ({"qgemm16": 0}, {"lin_kq_image": 1}),
          "jit-image": ({"qgemm16": 0, "jit_qimages": 1}, {"lin_kq_image": 1, "jit_images": 1})}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("K", (256, 768))
@pytest.mark.parametrize("name,gtype", TYPES)
def test_decode_one_hot(sd, gpu, name, gtype, K, route):
    rng, M = np.random.default_rng(K + gtype), 160
    nb = M * K // 256
    d, dmin = (rng.integers(1, 64, nb) / 1024).astype(np.float16), (rng.integers(1, 64, nb) / 512).astype(np.float16)
    f = KQ.random_fields(rng, gtype, nb, d, dmin)
    opts, routes = ROUTES[route]
    out, cached = run_linear(sd, gpu, gtype, KQ.pack(gtype, *f), M, K, np.eye(K, dtype=np.float32), opts, routes)
    assert cached == (256 * K * 2 if route == "cached-image" else 0), "only the cached route keeps an image (160 rows padded to 256)"
    want = KQ.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float32)
    bad = np.argwhere(out.T != want)
    assert len(bad) == 0, f"{len(bad)} weights differ; first (column, k) = {tuple(bad[0])}: got {out.T[tuple(bad[0])]!r}, w16 {want[tuple(bad[0])]!r}"


def integer_fields(rng, gtype, nb, one_per_row_of=None, small=False):
    """d = dmin in {1/2, 1} per super-block (small: 2^-9, scales <= 3: GEGLU pre-activations of a few units); one_per_row_of = K: a single weight 3 d per row"""
    d = (np.full(nb, 2.0 ** -9) if small else rng.choice([0.5, 1.0], nb)).astype(np.float16)
    d[: min(nb, 2)] = (2.0 ** -9 if small else 1.0), (2.0 ** -10 if small else 0.5)
    hi = 3 if small else 63
    if gtype == KQ.Q6_K:
        sc, mn, q = rng.integers(-hi, hi + 1, (nb, 16)), np.zeros((nb, 8), np.int64), rng.integers(-32, 32, (nb, 256))
    else:
        sc, mn, q = rng.integers(0, hi + 1, (nb, 8)), rng.integers(0, hi + 1, (nb, 8)), rng.integers(0, KQ.QMAX[gtype] + 1, (nb, 256))
    if one_per_row_of:
        per = one_per_row_of // 256
        sc, mn, q = np.ones_like(sc), np.zeros_like(mn), np.zeros_like(q)
        rows = np.arange(nb // per)
        pos = (rows * 37) % one_per_row_of
        q[rows * per + pos // 256, pos % 256] = 3
    return d[:nb], d[:nb], sc, mn, q


# (id, rows, K, M, epilogue, options, lin_kq_* moves); M = 8: a partial column tile and a wave with no column; split-k: 1 tile, S = min(512, nseg / 2) = 2
CASES = [("1-row", 1, 256, 8, "none", {}, {"lin_kq_gemm_rb1": 1}), ("2-rows", 2, 768, 160, "none", {}, {"lin_kq_gemm_rb1": 1}),
         ("33-rows", 33, 256, 160, "none", {}, {"lin_kq_gemm_rb2": 1}), ("130-rows", 130, 768, 8, "none", {}, {"lin_kq_gemm_rb2": 1}),
         ("last-row-rb4", 0, 256, 160, "none", {"qgemm16_rb": 4}, {"lin_kq_gemm_rb4": 1}), ("last-row", 0, 768, 8, "none", {}, {"lin_kq_gemm_rb2": 1}),
         ("split-k", 2, 1024, 8, "bias", {}, {"lin_kq_gemm_rb1": 1, "lin_kq_gemm_reduce": 1}), ("above-image", 1, 256, 160, "none", {}, {"lin_kq_image": 1}),
         ("bias+res", 33, 768, 160, "bias+res", {}, {"lin_kq_gemm_rb2": 1}), ("gate", 130, 256, 160, "gate", {}, {"lin_kq_gemm_rb2": 1}),
         ("presilu", 1, 768, 160, "presilu", {}, {"lin_kq_gemm_rb1": 1, "fused_presilu": 1}),   # SiLU applied by k_kq_gemm while it stages the row
         ("geglu-pairs", 64, 256, 256, "geglu", {}, {"lin_kq_image": 1, "lin_geglu_pair": 1}),
         ("geglu-16-interleave", 2048, 1280, 10240, "geglu", {}, {"lin_kq_image": 1, "lin_geglu16": 1})]   # (the shape at which the default policy takes that image order)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("name,gtype", TYPES)
def test_integer_linear(sd, gpu, name, gtype, case):
    cid, rows, K, M, epi, opts, routes = case
    if cid in ("last-row-rb4", "last-row", "above-image"):   # kernel 1's range (kq_gemm_supported): 512 rows, q6_K 256; one row above it the image route
        rows += 256 if gtype == KQ.Q6_K else 512
    if cid == "geglu-16-interleave" and sd.calibrate()["compute_units"] != 256:
        pytest.skip("the 16-column interleave is the default policy's choice for this shape on 256 CUs")
    rng = np.random.default_rng(rows * 7 + K + gtype)
    small = epi == "geglu"
    f = integer_fields(rng, gtype, M * K // 256, one_per_row_of=K if epi == "presilu" else None, small=small)
    w = KQ.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float32)
    unit = 2.0 ** -10 if small else 0.5
    assert np.array_equal(w / unit, np.rint(w / unit)) and np.abs(w.reshape(-1, 256) / f[0].astype(np.float32)[:, None]).max() <= 2016
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
    out, _ = run_linear(sd, gpu, gtype, KQ.pack(gtype, *f), M, K, x, opts, routes, epi=epi, extra=extra, batch=batch)
    want, p = R.linear_ref(x, w, "f16", epi=epi, bias=extra.get("bias"), residual=extra.get("residual"), gate=extra.get("gate"), batches=batch, fast=rows > 1000)
    if epi in ("presilu", "geglu"):
        if epi == "presilu":
            col = np.abs(w).argmax(axis=1)
            t1, t2 = R.transcendental_terms(R.silu64(p[:, col]), p[:, col], np.abs(w).max(axis=1)[None, :])
        else:
            assert float(np.abs(want).max()) < R.F16_MAX / 2
            t1, t2 = R.transcendental_terms(want, p[1], np.maximum(1.0, np.abs(p[0])))
        err = np.abs(out.astype(np.float64) - want)
        print(f"{name} {cid}: largest |error| / bar = {float((err / (t1 + t2)).max()):.3f}")
        assert (err <= t1 + t2).all()
    else:
        w32 = want.astype(np.float32)
        bad = np.argwhere(out != w32)
        assert len(bad) == 0, f"{len(bad)} of {w32.size} differ; first (row, column) = {tuple(bad[0])}: got {out[tuple(bad[0])]!r}, reference {w32[tuple(bad[0])]!r}"


@pytest.mark.parametrize("name,gtype", TYPES)
def test_supports_op(sd, gpu, name, gtype):
    """whole super-blocks per row only: K = 256 is claimed, K = 320 (ne0 of a hand-made tensor: the front-end would not build it) is refused"""
    L = sd.lib()
    with Graph(gpu) as g:
        node = L.ggml_mul_mat(g.ctx, L.ggml_new_tensor_2d(g.wctx, gtype, 256, 8), g.input(np.zeros((2, 256), np.float32)))
        assert g.supports(node)
        sd.backend_set_option("mfma_gemm", 0)   # the Linear path is off: there is no other kernel for super-blocks
        try:
            assert not g.supports(node)
        finally:
            sd.backend_set_option("mfma_gemm", 1)
        tensor_struct(tensor_struct(node).src[0]).ne[0] = 320
        tensor_struct(tensor_struct(node).src[1]).ne[0] = 320
        assert not g.supports(node)


@pytest.mark.parametrize("name,gtype", TYPES)
def test_weight_outside_a_weights_buffer_fails_the_graph(sd, gpu, name, gtype):
    """supports_op cannot see the buffer: a K-typed MUL_MAT operand that is not a static weight never reaches the generic matmul, the plan fails loudly"""
    L = sd.lib()
    with Graph(gpu) as g:
        w = L.ggml_new_tensor_2d(g.ctx, gtype, 256, 8)
        L.ggml_set_input(w)
        g._inputs.append((w, bytes(8 * KQ.BLOCK_BYTES[gtype])))
        with pytest.raises(AssertionError, match="graph_compute status"):
            g.run(L.ggml_mul_mat(g.ctx, w, g.input(np.ones((2, 256), np.float32))))
