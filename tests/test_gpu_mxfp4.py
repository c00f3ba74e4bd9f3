"""MXFP4 Linear weights on the product backend (kernels/bquant.hip, mxfp4_decode.h): ONE Linear through the C ABI per test, its weight tensor created in type 39
from raw blocks (tests/mxfp4_ref.py), bit for bit; the harness and the counter check are test_gpu_bquant's.  Decode: x is the identity, so the output transposed
must equal w16 = f16(ggml's value) on every route; M = 16 rows of 17 bytes (K = 32) start at all sixteen byte phases of a 16-byte granule.  Integer data: e = 127 /
128 (d = 1/2, 1), x in -4 .. 4, partial sums asserted below 2^24 units.  Behind SiLU / GEGLU: linear_ref's transcendental bar."""
import numpy as np
import pytest

import linear_ref as R
import mxfp4_ref as MX
from test_gpu_bquant import MAX_ROWS, ROUTES, pytestmark, run_linear   # noqa: F401 (pytestmark: gpu, not on the CPU oracle)

# e - 128 per block: "normal" = every w16 finite and normal or zero (2^-14 <= 2^n, 12 * 2^n <= 65504); "subnormal" = -28 .. -14: w16 down to one ulp (12 * 2^-28
# rounds up to 2^-24), zero below, ties at k = 3, 6, 12.  The matrix unit keeps subnormal f16 operands, so the NumPy w16 is the expected value
SPANS = {"normal": (-14, 12), "subnormal": (-28, -14)}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("K", (32, 288))   # one short segment alone; a full 8-block segment and a one-block tail
@pytest.mark.parametrize("span", SPANS)
def test_decode_one_hot(sd, gpu, span, K, route):
    rng, M = np.random.default_rng(K + len(span)), 16
    nb, (lo, hi) = M * K // 32, SPANS[span]
    e, q = 128 + rng.integers(lo, hi + 1, nb), rng.integers(0, 16, (nb, 32))
    e[:2], q[0, :16] = (128 + lo, 128 + hi), np.arange(16)   # both ends of the span, every code
    opts, routes = ROUTES[route]
    out, cached = run_linear(sd, gpu, MX.MXFP4, MX.pack(e, q), M, K, np.eye(K, dtype=np.float32), opts, routes or {"lin_bq_gemm_rb1" if K == 32 else "lin_bq_gemm_rb2": 1})
    assert cached == (128 * ((K + 63) // 64 * 64) * 2 if route == "cached-image" else 0), "only the cached route keeps an image (16 rows padded to 128, K to 64)"
    want = MX.dequant(e, q).astype(np.float16).reshape(M, K).astype(np.float32)
    assert np.isfinite(want).all() and (span == "normal") == (np.abs(want[want != 0]).min() >= 2.0 ** -14)
    bad = np.argwhere(out.T != want)
    assert len(bad) == 0, f"{len(bad)} weights differ; first (column, k) = {tuple(bad[0])}: got {out.T[tuple(bad[0])]!r}, w16 {want[tuple(bad[0])]!r}"


# (id, rows, K, M, epilogue, lin_bq_* moves).  Tiles: 32 rows (1 .. 32) / 64 rows; 128 columns, 4 waves x 32 (M = 8: three waves with no column; M = 136: a full
# tile and a partial one); segments of 256 k; 1 .. 4 rows are staged from f32, 5 and more come from the f16 operand image; K = 800 is the smallest K that splits
RB1, RB2 = {"lin_bq_gemm_rb1": 1}, {"lin_bq_gemm_rb2": 1}
CASES = [("1-row", 1, 288, 8, "none", RB1), ("4-rows", 4, 320, 136, "none", RB1), ("4-rows-presilu", 4, 288, 136, "presilu", {**RB1, "fused_presilu": 1}),
         ("5-rows", 5, 320, 136, "bias", RB1), ("33-rows", 33, 288, 136, "bias+res", RB2), ("last-row", MAX_ROWS, 288, 8, "none", RB2),
         ("above-image", MAX_ROWS + 1, 32, 136, "none", {"lin_bq_image": 1}), ("split-k", 2, 800, 8, "bias", {**RB1, "lin_bq_gemm_reduce": 1}),
         ("gate", 66, 96, 136, "gate", RB2), ("geglu-pairs", 64, 288, 256, "geglu", {"lin_bq_image": 1, "lin_geglu_pair": 1})]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_integer_linear(sd, gpu, case):
    """presilu: a row's weights are one live block (code 0 elsewhere) and the bar is linear_ref's, summed as in test_gpu_bquant: every image value silu(x_k)
    carries transcendental_terms(silu(x_k), x_k) times |w_k|, and the f32 sum of the <= 32 products adds at most 32 * 2^-24 * sum |w_k silu(x_k)|."""
    cid, rows, K, M, epi, routes = case
    rng, small, nb = np.random.default_rng(rows * 7 + K), epi == "geglu", M * K // 32
    e, q = (np.full(nb, 119) if small else rng.choice([127, 128], nb)), rng.integers(0, 16, (nb, 32))   # small: d = 2^-9, GEGLU pre-activations of a few units
    if epi == "presilu":
        live = np.zeros(nb, bool)
        live[np.arange(M) * (K // 32) + (np.arange(M) * 5) % (K // 32)] = True
        q[~live] = 0
    w = MX.dequant(e, q).astype(np.float16).reshape(M, K).astype(np.float32)
    unit = 2.0 ** -9 if small else 0.5
    assert np.array_equal(w / unit, np.rint(w / unit))
    x = R.ints(rng, -1, 1, (rows, K)) if small else R.ints(rng, -4, 4, (rows, K))
    batch, extra = (2 if epi == "gate" else 1), {}
    if epi in ("bias", "bias+res", "gate", "geglu"):
        extra["bias"] = R.nonzero_ints(rng, -1 if small else -64, 1 if small else 64, (M,))
    if epi in ("bias+res", "gate"):
        extra["residual"] = R.ints(rng, -8, 8, (rows, M))
    if epi == "gate":
        extra["gate"] = R.nonzero_ints(rng, -2, 2, (batch, M))
    bound = (float(np.abs(x).max()) * float(np.abs(w).astype(np.float64).sum(axis=1).max()) + 2 * (64 + 8)) / unit
    assert epi == "presilu" or bound < R.EXACT_BOUND, f"partial sums up to {bound} units"
    out, _ = run_linear(sd, gpu, MX.MXFP4, MX.pack(e, q), M, K, x, {}, routes, epi=epi, extra=extra, batch=batch)
    want, p = R.linear_ref(x, w, "f16", epi=epi, bias=extra.get("bias"), residual=extra.get("residual"), gate=extra.get("gate"), batches=batch)
    if epi == "presilu":
        aw = np.abs(w).astype(np.float64).T
        bar = sum(R.transcendental_terms(R.silu64(p), p)) @ aw + 32 * 2.0 ** -24 * (np.abs(R.silu64(p)) @ aw)
    elif epi == "geglu":
        assert float(np.abs(want).max()) < R.F16_MAX / 2
        bar = sum(R.transcendental_terms(want, p[1], np.maximum(1.0, np.abs(p[0]))))
    else:
        bar = 0.0   # bit for bit
    err = np.abs(out.astype(np.float64) - want)
    assert (err <= bar).all(), f"{cid}: {int((err > bar).sum())} of {err.size} beyond the bar; largest |error| {float(err.max())!r}"

