"""k_kq_gemv (kernels/kquant.hip): the hoisted modulation and embedding groups of q2_K .. q6_K Linears in ONE weight-streaming launch, bit for bit against plain
NumPy float64 over w16 = f16(dequant) and f16(SiLU(x)).  Both groups put a SiLU in front: x is drawn from {0} + {18 .. 32} + {-32}, where x * rcp(1 + exp(-x)) is x
(exp(-x) < 2^-25), 0 or a value that rounds to -0 in f16 — asserted on the float32 restatement below.  Weights are integer multiples of 1/2 (d = dmin in {1/2, 1},
sub-block scales <= 3), so every product and partial sum is exact in f32 (asserted against linear_ref.EXACT_BOUND) whatever the order of the sums."""
import os

import numpy as np
import pytest

import kquant_low_ref as KQL
import kquant_ref as KQ
import linear_ref as R
from ggml_graph import F32, Graph

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") == "1", reason="the CPU oracle has no K-quant MUL_MAT")]
TYPES = pytest.mark.parametrize("gtype", sorted({**KQL.TYPES, **KQ.TYPES}.values()), ids=sorted({**KQL.TYPES, **KQ.TYPES}))
MS = (8, 100, 52)   # 8: a partial workgroup and waves with no column; unequal sizes: the member lookup
WATCHED = ("lin_kq", "lin_qgemv", "lin_qgemm16", "kquant_linears", "qgemv_linears", "hoisted_", "fused_presilu")


def ref_of(gtype):
    return KQL if gtype in KQL.TYPES.values() else KQ


def integer_fields(rng, gtype, nb):
    d = rng.choice([0.5, 1.0], nb).astype(np.float16)
    if gtype in (KQL.Q3_K, KQ.Q6_K):
        q = rng.integers(-4, 4, (nb, 256)) if gtype == KQL.Q3_K else rng.integers(-32, 32, (nb, 256))
        return d, d, rng.integers(-3, 4, (nb, 16)), np.zeros((nb, 16 if gtype == KQL.Q3_K else 8), np.int64), q
    ns = 16 if gtype == KQL.Q2_K else 8
    return d, d, rng.integers(0, 4, (nb, ns)), rng.integers(0, 4, (nb, ns)), rng.integers(0, 4 if gtype == KQL.Q2_K else KQ.QMAX[gtype] + 1, (nb, 256))


def exact_silu_x(rng, shape):
    """-> x, f16(SiLU(x)) as float64; the float32 restatement of the device formula must be exact on it"""
    x = rng.choice(np.array([0, -32] + list(range(18, 33)), np.float32), shape)
    s = (x * (np.float32(1) / (np.float32(1) + np.exp(-x, dtype=np.float32)))).astype(np.float16)
    assert np.array_equal(s, np.where(x >= 18, x, 0).astype(np.float16))
    return x, s.astype(np.float64)


def members(rng, gtype, K, integer, ms=MS):
    """-> [(packed blocks, w16 float64 [M, K], bias [M])] for the three members"""
    out, Q = [], ref_of(gtype)
    for M in ms:
        nb = M * K // 256
        f = integer_fields(rng, gtype, nb) if integer else Q.random_fields(rng, gtype, nb, (rng.integers(1, 64, nb) / 1024).astype(np.float16),
                                                                           (rng.integers(1, 64, nb) / 512).astype(np.float16))
        out.append((Q.pack(gtype, *f), Q.dequant(gtype, *f).astype(np.float16).reshape(M, K).astype(np.float64), R.nonzero_ints(rng, -64, 64, (M,))))
    return out


def run_group(sd, gpu, gtype, K, x, mem, add_to=None):
    """the three chains SiLU -> MUL_MAT -> ADD(bias, in place) [-> RESHAPE -> ADD(add_to[i], .)] on one input; -> outputs, counters that moved"""
    L, before = sd.lib(), sd.backend_stats()
    with Graph(gpu) as g:
        xi, outs = g.input(x), []
        for i, (blocks, w, bias) in enumerate(mem):
            wt = L.ggml_new_tensor_2d(g.wctx, gtype, K, len(w))
            g._weights.append((wt, blocks.tobytes()))
            y = L.ggml_add_inplace(g.ctx, L.ggml_mul_mat(g.ctx, wt, L.ggml_silu(g.ctx, xi)), g.weight(bias, F32))
            if add_to is not None:
                y = L.ggml_add(g.ctx, g.input(add_to[i]), L.ggml_reshape_4d(g.ctx, y, 1, 1, len(w), len(x)))
            outs.append(y)
        res = g.run(*outs)
    after = sd.backend_stats()
    return res, {f: after[f] - before[f] for f in after if f.startswith(WATCHED) and after[f] != before[f]}


def check_moved(moved, want):
    if not os.environ.get("SDCPP_BACKEND_OPTS"):
        assert moved == want, f"counters moved {moved}, expected {want}"


@pytest.mark.parametrize("rows", (1, 2))
# K: one super-block (idle lanes) / three: 252- / 330- / 630-byte rows at changing 4- / 2-byte phases / nine: a wave step is 4 (q4_K, q5_K) or 8 super-blocks of a row,
# so 3 or 2 steps (the refill of the row registers, the phase of a later step) with ONE super-block in the last
@pytest.mark.parametrize("K", (256, 768, 2304))
@TYPES
def test_modulation_group(sd, gpu, gtype, K, rows):
    rng = np.random.default_rng(1000 * gtype + K + rows)
    mem = members(rng, gtype, K, integer=True)
    x, s = exact_silu_x(rng, (rows, K))
    bound = (32 * max(float(np.abs(w).sum(axis=1).max()) for _, w, _ in mem) + 64) / 0.5
    assert bound < R.EXACT_BOUND and all(np.array_equal(w * 2, np.rint(w * 2)) for _, w, _ in mem), f"partial sums up to {bound} units"
    out, moved = run_group(sd, gpu, gtype, K, x, mem)
    check_moved(moved, {"lin_kq_gemv": 1, "hoisted_mod_linears": 3, "kquant_linears": 3, "fused_presilu": 3})
    for o, (_, w, bias) in zip(out, mem):
        assert np.array_equal(o.reshape(rows, -1), (s @ w.T + bias).astype(np.float32))
    try:   # the same graph as three k_kq_gemm launches: the same values
        sd.backend_set_option("qgemv", 0)
        single, moved = run_group(sd, gpu, gtype, K, x, mem)
    finally:
        sd.backend_set_option("qgemv", 1)
    split = {"lin_kq_gemm_reduce": 3} if K >= 1024 else {}   # k_kq_gemm cuts K into slices of at least two super-blocks (kq_gemm_grid): from four on
    check_moved(moved, {"lin_kq_gemm_rb1": 3, "kquant_linears": 3, "fused_presilu": 3, **split})
    assert all(np.array_equal(a, b) for a, b in zip(out, single))


# member sizes that are no multiple of a wave's 4 rows (plan_hoisted_emb does not ask for it: the single-weight launch clamps its last group); 32880 columns: two
# column groups per wave (gpw = 2 from 32768 columns on)
@pytest.mark.parametrize("K,ms", ((768, MS), (768, (6, 101, 53)), (256, (8, 100, 32772))), ids=("3x", "odd-members", "two-groups-per-wave"))
@pytest.mark.parametrize("N", (2, 4))   # R = 2 and R = 4 activation rows in registers
@TYPES
def test_embedding_group(sd, gpu, gtype, N, K, ms):
    rng = np.random.default_rng(100 * gtype + N + K + ms[0])
    mem = members(rng, gtype, K, integer=True, ms=ms)
    x, s = exact_silu_x(rng, (N, K))
    assert (32 * max(float(np.abs(w).sum(axis=1).max()) for _, w, _ in mem) + 64 + 8) / 0.5 < R.EXACT_BOUND
    add_to = [R.ints(rng, -8, 8, (N, M, 2, 2)) for M in ms]
    out, moved = run_group(sd, gpu, gtype, K, x, mem, add_to)
    check_moved(moved, {"lin_kq_gemv": 1, "hoisted_emb_linears": 3, "kquant_linears": 3, "fused_presilu": 3})
    for o, a, (_, w, bias) in zip(out, add_to, mem):
        assert np.array_equal(o, (a + (s @ w.T + bias)[:, :, None, None]).astype(np.float32))


@TYPES
def test_real_valued_decode(sd, gpu, gtype):
    """random super-blocks: f32 sums of exact products in any order, plus the one rounded bias add"""
    rng, K = np.random.default_rng(gtype), 768
    mem = members(rng, gtype, K, integer=False)
    x, s = exact_silu_x(rng, (2, K))
    out, moved = run_group(sd, gpu, gtype, K, x, mem)
    check_moved(moved, {"lin_kq_gemv": 1, "hoisted_mod_linears": 3, "kquant_linears": 3, "fused_presilu": 3})
    for o, (_, w, bias) in zip(out, mem):
        ref = s @ w.T + bias
        err, bar = np.abs(o.reshape(2, -1) - ref), K * 2.0 ** -24 * (np.abs(s) @ np.abs(w).T) + 2.0 ** -24 * np.abs(ref)
        print(f"largest |error| / bar = {float((err / bar).max()):.3g}")
        assert (err <= bar).all()

