"""Attention kernels on scores that MOVE the running max (tests/attn_scores.py), and SOFT_MAX with its mask / scale arguments.

Every other attention test draws standard-normal Q / K: k_flash_attn's deferred max then never moves after the first key tile, so the accumulator
rescale (`__shfl(alpha, row)`), `l_run *= alpha`, the max-slot rewrite, the rescale of the ones column and the split vote never meet a non-zero
accumulator (tests/test_kernel_logic.py proves both statements on the model).  Here each family runs through the smallest shape that reaches each
kernel variant, and the variant is ASSERTED through the flash_*_launches statistics.

Bars (per case, printed before they are asserted):
  * rel-L2 against the float64 softmax on the f16-rounded K and V < max(B, 3 s): B the bar the path's existing test uses (2e-3 flash node / manual
    chain / 77-key kernel, 4e-3 head dims > 160), s the rel-L2 of the path's operand-rounding MODEL against the same exact result, computed here: the
    margin comes from the two references, not from the kernel; the factor 3 covers f32 summation order and v_exp_f32;
  * FLASH_ATTN_EXT node: rel-L2 against the oracle < max(1e-2, 2 rel_l2(oracle, exact)) — the oracle accumulates V in f16, the larger term;
  * two runs are bit-equal;
  * spike_last: per query row, max-abs <= 3e-3 max(1, |ref row|max) — an aggregate norm can hide a handful of mis-scaled rows."""
import os

import numpy as np
import pytest

import attn_scores as AS
from ggml_graph import F16, F32, Graph

pytestmark = pytest.mark.gpu

ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
VARIANT_STATS = ("flash_short_launches", "flash_qb2_launches", "flash_mslot_launches", "flash_generic_launches")


def _counting():
    return ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")


def _inputs(kind, d, Lq, Lk, HN):
    rng = np.random.default_rng([d, Lq, Lk, AS.KINDS.index(kind)])
    q, k, v = AS.make_heads(kind, Lq, Lk, d, HN, rng)
    return q, k, v, 1.0 / np.sqrt(d)


def _run_twice(sd, gpu, build, expect=None, extra=None):
    """the graph on the device under test, twice (bit-equal); `expect` = the flash variant statistic that must count (None: none of the four)"""
    before = sd.backend_stats() if _counting() else None
    outs = []
    for _ in range(2):
        with Graph(gpu) as g:
            node = build(g, sd.lib())
            assert g.supports(node)
            outs.append(g.run(node))
    np.testing.assert_array_equal(outs[0], outs[1])
    if before is not None:
        after = sd.backend_stats()
        for name in VARIANT_STATS:
            delta = after[name] - before[name]
            assert (delta >= 1) if name == expect else (delta == 0), (name, delta, expect)
        for name, least in (extra or {}).items():
            assert after[name] - before[name] >= least, name
    return outs[0]


def _check(tag, out, exact, model, B, kind):
    """out, exact, model: [HN, Lq, d]"""
    assert np.isfinite(out).all()
    s = AS.rel_l2(model, exact)
    err = AS.rel_l2(out, exact)
    bar = max(B, 3.0 * s) if ON_GPU else max(1e-2, 3.0 * s)   # self-check mode: the oracle's flash node accumulates V in f16
    row_err = np.abs(out - exact).max(-1)
    row_bar = 3e-3 * np.maximum(1.0, np.abs(exact).max(-1))
    print(f"[attn-scores] {tag} {kind}: rel-L2 vs exact {err:.3e} (bar {bar:.1e}, model {s:.3e}); worst row max-abs / bar {float((row_err / row_bar).max()):.3f}")
    assert err < bar
    if kind == "spike_last" and ON_GPU:
        bad = np.argwhere(row_err > row_bar)
        assert bad.size == 0, f"{len(bad)} rows beyond 3e-3: first (head, row) {bad[:4].tolist()}"


def _flash_variant(d, Lq, Lk, HN):
    if d % 8 != 0:
        return "flash_generic_launches"
    if d <= 64 and 64 < Lk <= 96:
        return "flash_short_launches"
    if d == 40:
        qb2 = (Lk + 63) // 64 >= 4 and Lq >= 192 and (Lq + 255) // 256 * HN >= 512
        return "flash_qb2_launches" if qb2 else "flash_mslot_launches"
    return None


def _flash_node_case(sd, oracle, gpu, d, Lq, Lk, HN, kind, tag, k0=None):
    q, k, v, scale = _inputs(kind, d, Lq, Lk, HN)
    if k0 is not None:
        k[:, :, 0] = k0

    def build(g, L):
        out = L.ggml_flash_attn_ext(g.ctx, g.input(q), g.input(k, F16), g.input(v, F16), None, scale, 0.0, 0.0)
        L.ggml_flash_attn_ext_set_prec(out, 10)
        return out

    expect = _flash_variant(d, Lq, Lk, HN)
    out = _run_twice(sd, gpu, build, expect)
    with Graph(oracle) as g:
        ref = g.run(build(g, sd.lib()))
    assert out.shape == ref.shape == (1, Lq, HN, d)
    out, ref = out[0].transpose(1, 0, 2), ref[0].transpose(1, 0, 2)
    k16, v16 = AS.f16r(k), AS.f16r(v)
    exact = AS.exact(q, k16, v16, scale)
    if expect == "flash_short_launches":
        model = AS.onepass_model(q, k16, v16, scale)
    else:
        model, moves, split, pmax = AS.deferred_model(q, k16, v16, scale, mslot=AS.uses_max_slot(d, Lk))
        assert np.isfinite(pmax)
        if kind in AS.MOVING and AS.ramp_can_move(kind, Lk):
            assert moves >= 2 and split >= 1
    o_err, o_own = AS.rel_l2(out, ref), AS.rel_l2(ref, exact)
    print(f"[attn-scores] {tag} d={d} Lq={Lq} Lk={Lk} HN={HN} {kind}: rel-L2 vs oracle {o_err:.3e} (oracle vs exact {o_own:.3e})")
    _check(f"{tag} d={d} Lq={Lq} Lk={Lk} HN={HN}", out, exact, model, 2e-3, kind)
    assert o_err < max(1e-2, 2.0 * o_own)


@pytest.mark.parametrize("kind", AS.KINDS)
@pytest.mark.parametrize("d,Lq,Lk,HN", AS.FLASH_NODE_CASES)
def test_flash_node_scores_move_the_max(sd, oracle, gpu, d, Lq, Lk, HN, kind):
    """FLASH_ATTN_EXT (f16 K / V): the max-slot kernels with one and two query blocks per wave, the select-free staging (d = 64 / 128), the 48-wide tile
    without the slot, the ones column on the 3-block accumulator (d = 80), d = 96 / 160 and the generic staging (d = 20)."""
    _flash_node_case(sd, oracle, gpu, d, Lq, Lk, HN, kind, "flash-node")


@pytest.mark.parametrize("d,Lq,Lk,HN", AS.FLASH_NODE_CASES[:2])
def test_flash_max_slot_first_tile_below_f32_exp_range(sd, oracle, gpu, d, Lq, Lk, HN):
    """offset_neg with the key channel at -50: every score sits near -144 log2 units (operands still far inside f16).  The max-slot kernels moved the
    max from 0 to the first tile's max with alpha = 2^144 = inf on the zero accumulators and returned NaN rows (found through the block test's
    offset_neg case, where the projections' noise pushes some rows below -128); the first tile takes alpha = 1 now.  Both copies of the move: one and
    two query blocks per wave."""
    _flash_node_case(sd, oracle, gpu, d, Lq, Lk, HN, "offset_neg", "flash-node k0=-50", k0=-50.0)


@pytest.mark.parametrize("kind", AS.KINDS)
@pytest.mark.parametrize("d,Lq,Lk,HN", AS.SHORT_CASES)
def test_flash_short_scores(sd, oracle, gpu, d, Lq, Lk, HN, kind):
    """k_flash_short (65 .. 96 keys in registers): one-pass softmax and the -inf accumulator start of the padded key block on scores up to ~120 log2
    units; spike_mid puts its keys at 64 (first of the masked block) and Lk // 2, spike_last at Lk - 1 (its last valid key)."""
    _flash_node_case(sd, oracle, gpu, d, Lq, Lk, HN, kind, "flash-short")


@pytest.mark.parametrize("kind", AS.KINDS)
@pytest.mark.parametrize("d,Lq,Lk,HN", AS.MANUAL_CASES + AS.GEMM_CASES)
def test_manual_chain_scores_move_the_max(sd, oracle, gpu, d, Lq, Lk, HN, kind):
    """MUL_MAT(k, q) -> SCALE -> SOFT_MAX -> MUL_MAT(vT, kq) with f32 K / V^T: the !FAST kernel (its own has_ones / l_run split), and beyond d = 160 the
    composition from MFMA GEMMs and k_soft_max_rows_f16 (statistic gemm_attention)."""
    q, k, v, scale = _inputs(kind, d, Lq, Lk, HN)
    vt = np.ascontiguousarray(v.transpose(0, 2, 1))

    def build(g, L):
        kq = L.ggml_mul_mat(g.ctx, g.input(k), g.input(q))
        kq = L.ggml_scale_inplace(g.ctx, kq, scale)
        kq = L.ggml_soft_max_inplace(g.ctx, kq)
        return L.ggml_mul_mat(g.ctx, g.input(vt), kq)

    gemm = d > 160
    out = _run_twice(sd, gpu, build, None if gemm else "flash_generic_launches", {"gemm_attention": 1} if gemm else {"fused_attention": 1})
    assert out.shape == (1, HN, Lq, d)
    k16, v16 = AS.f16r(k), AS.f16r(v)
    exact = AS.exact(q, k16, v16, scale)
    if gemm:
        model = AS.gemm_model(q, k16, v16, scale)
    else:
        model, moves, split, pmax = AS.deferred_model(q, k16, v16, scale)
        assert np.isfinite(pmax)
        if kind in AS.MOVING and AS.ramp_can_move(kind, Lk):
            assert moves >= 2 and split >= 1
    tag = f"{'gemm-attn' if gemm else 'manual'} d={d} Lq={Lq} Lk={Lk} HN={HN}"
    if ON_GPU:
        _check(tag, out[0], exact, model, 4e-3 if gemm else 2e-3, kind)
    else:   # self-check mode: the oracle runs this chain in f32 on the UNROUNDED K / V
        full = AS.exact(q, k, v, scale)
        print(f"[attn-scores] {tag} {kind}: oracle vs exact f32 chain {AS.rel_l2(out[0], full):.3e}")
        assert np.isfinite(out).all() and AS.rel_l2(out[0], full) < 1e-4


# ---- SOFT_MAX with mask and scale (ggml_soft_max_ext): claimed by supports_op for f16 / f32 masks broadcast over ne[2] and ne[3]

def _soft_max_rows(ncols, nrows, rng):
    """rows spanning +-80, rows with a common offset of +-1e4, and plain standard-normal rows, in turn"""
    x = rng.standard_normal((nrows, ncols)).astype(np.float32)
    for r in range(nrows):
        if r % 4 == 0:
            x[r] = rng.uniform(-80.0, 80.0, ncols)
        elif r % 4 == 1:
            x[r] += 1e4
        elif r % 4 == 2:
            x[r] -= 1e4
    return x


def _soft_max_exact(logits32):
    z = logits32.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    p = np.exp(z)
    return p / p.sum(-1, keepdims=True)


@pytest.mark.parametrize("ncols", [5, 77, 256, 257, 1000])
@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("mtype", [F32, F16])
def test_soft_max_ext_mask_and_scale(sd, oracle, gpu, ncols, scale, mtype):
    """softmax(x * scale + mask) against float64 on the f32 logits the op defines (x * scale is exact for these scales; the mask holds 0, -inf and
    multiples of 1/4, exact in f16, and is zero on the +-1e4 rows' kept entries so that their sum stays exact).  Causal -inf mask: every row keeps at
    least one finite entry; masked entries must come out as exact zeros; rows sum to 1."""
    rng = np.random.default_rng([ncols, int(scale * 1000), mtype])
    rows, H, N = 12, 3, 2
    x = np.stack([_soft_max_rows(ncols, rows, rng) for _ in range(H * N)]).reshape(N, H, rows, ncols)
    r_ = np.arange(rows)
    keep = np.where(r_ % 3 == 0, ncols, 1 + (r_ * 37) % ncols)                  # row r keeps its first keep[r] columns (causal shape, >= 1)
    mask = np.where(np.arange(ncols)[None, :] < keep[:, None], 0.0, -np.inf).astype(np.float32)
    bias = (rng.integers(-8, 9, (rows, ncols)) / 4.0).astype(np.float32)
    bias[np.arange(rows) % 4 != 0] = 0.0
    mask = mask + bias                                                          # -inf stays -inf

    def build(g, L):
        return L.ggml_soft_max_ext(g.ctx, g.input(x), g.input(mask, mtype), scale, 0.0)

    outs = []
    for dev in (oracle, gpu):
        with Graph(dev) as g:
            node = build(g, sd.lib())
            assert g.supports(node)
            outs.append(g.run(node))
    ref, out = outs
    exact = _soft_max_exact(x * np.float32(scale) + mask[None, None])
    err = float(np.abs(out - exact).max())
    print(f"[soft-max-ext] ncols={ncols} scale={scale} mask={'f16' if mtype == F16 else 'f32'}: max-abs vs float64 {err:.3e}, vs oracle {float(np.abs(out - ref).max()):.3e}")
    assert np.isfinite(out).all()
    assert (out[..., ~np.isfinite(mask)] == 0.0).all()
    assert np.abs(out.astype(np.float64).sum(-1) - 1.0).max() < 1e-6
    assert err <= 2e-6
    assert np.abs(out - ref).max() <= 2e-6


@pytest.mark.parametrize("ncols", [5, 77, 256, 257, 1000])
def test_soft_max_inplace_wide_rows(sd, oracle, gpu, ncols):
    """the unmasked in-place form on the same rows (spans of +-80, common offsets of +-1e4)"""
    rng = np.random.default_rng(ncols)
    x = _soft_max_rows(ncols, 12, rng).reshape(1, 2, 6, ncols)

    def build(g, L):
        return L.ggml_soft_max_inplace(g.ctx, L.ggml_scale(g.ctx, g.input(x), 1.0))

    with Graph(gpu) as g:
        out = g.run(build(g, sd.lib()))
    exact = _soft_max_exact(x)
    err = float(np.abs(out - exact).max())
    print(f"[soft-max] in place, ncols={ncols}: max-abs vs float64 {err:.3e}")
    assert np.isfinite(out).all() and np.abs(out.astype(np.float64).sum(-1) - 1.0).max() < 1e-6
    assert err <= 2e-6
