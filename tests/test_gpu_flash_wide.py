"""FLASH_ATTN_EXT at head dims 192 .. 512 (k_flash_wide, kernels/flash_wide.hip) against the float64 softmax, on the score families of tests/attn_scores.py.

The kernel's tiles are 32 keys x 32 queries (not the 64 keys of k_flash_attn), so next to the shapes written for 64-key tiles — which here reach one tile + a tail (40),
exactly two tiles (64), 4 / 6 / 10 tiles + a tail (132 / 200 / 330), a partial query block (33), the head stride (HN 2 / 3) and several workgroups per head (257) —
two more reach less than one key tile (20 keys, 5 queries) and exactly one tile of each (32 x 32).

Bars (tests/test_gpu_attention_scores.py `_check`): rel-L2 against AS.exact on the f16-rounded K / V < max(4e-3, 3 s), 4e-3 the bar head dims > 160 already have and s the
rel-L2 of AS.deferred_model (Q, K, P, V rounded where this kernel rounds them, the max deferred by the same FA_THR) against the same exact result; spike_last also per
row, max-abs <= 3e-3 max(1, |ref row|max).  Two runs are bit-equal, and a head computes the same bits alone and as head 0 of a 3-head launch."""
import os

import numpy as np
import pytest

import attn_scores as AS
from ggml_graph import F16, Graph

pytestmark = pytest.mark.gpu

CASES = [(192, 33, 40, 2), (512, 32, 64, 1), (512, 100, 132, 1), (256, 70, 200, 3), (512, 257, 330, 2), (256, 5, 20, 1), (512, 32, 32, 1)]
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"   # (harness self-check on a CPU-only box: both sides run the oracle)
OLDER = ("gemm_attention", "flash_short_launches", "flash_qb2_launches", "flash_mslot_launches", "flash_generic_launches")


def _inputs(kind, d, Lq, Lk, HN):
    rng = np.random.default_rng([d, Lq, Lk, AS.KINDS.index(kind)])
    return (*AS.make_heads(kind, Lq, Lk, d, HN, rng), 1.0 / np.sqrt(d))


def _run(sd, gpu, q, k, v, scale):
    """the node on the device: claimed, and counted under flash_wide_launches alone -> [HN, Lq, d]"""
    counting = ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")
    before = sd.backend_stats() if counting else None
    with Graph(gpu) as g:
        L = sd.lib()
        node = L.ggml_flash_attn_ext(g.ctx, g.input(q), g.input(k, F16), g.input(v, F16), None, scale, 0.0, 0.0)
        L.ggml_flash_attn_ext_set_prec(node, 10)
        assert g.supports(node)
        out = g.run(node)
    if counting:
        after = sd.backend_stats()
        assert after["flash_wide_launches"] - before["flash_wide_launches"] >= 1
        assert all(after[n] == before[n] for n in OLDER), {n: after[n] - before[n] for n in OLDER}
    assert out.shape == (1, q.shape[1], q.shape[0], q.shape[2])
    return out[0].transpose(1, 0, 2)


@pytest.mark.parametrize("kind", AS.KINDS)
@pytest.mark.parametrize("d,Lq,Lk,HN", CASES)
def test_flash_wide_node_vs_float64_softmax(sd, gpu, d, Lq, Lk, HN, kind):
    q, k, v, scale = _inputs(kind, d, Lq, Lk, HN)
    out = _run(sd, gpu, q, k, v, scale)
    np.testing.assert_array_equal(out, _run(sd, gpu, q, k, v, scale))
    assert np.isfinite(out).all()
    k16, v16 = AS.f16r(k), AS.f16r(v)
    exact = AS.exact(q, k16, v16, scale)
    s = AS.rel_l2(AS.deferred_model(q, k16, v16, scale)[0], exact)
    err, bar = AS.rel_l2(out, exact), max(4e-3 if ON_GPU else 1e-2, 3.0 * s)   # (the oracle's flash node accumulates V in f16)
    row_err, row_bar = np.abs(out - exact).max(-1), 3e-3 * np.maximum(1.0, np.abs(exact).max(-1))
    print(f"[flash-wide] d={d} Lq={Lq} Lk={Lk} HN={HN} {kind}: rel-L2 vs exact {err:.3e} (bar {bar:.1e}, model {s:.3e}); worst row / bar {float((row_err / row_bar).max()):.3f}")
    assert err < bar
    if kind == "spike_last" and ON_GPU:
        assert (row_err <= row_bar).all(), np.argwhere(row_err > row_bar)[:4].tolist()


@pytest.mark.parametrize("kind", ["ramp12", "spike_mid", "offset_neg"])
def test_flash_wide_head_is_independent_of_the_launch(sd, gpu, kind):
    """(512, 100, 132): head 0 of a 3-head launch equals its single-head run bit for bit"""
    q, k, v, scale = _inputs(kind, 512, 100, 132, 3)
    np.testing.assert_array_equal(_run(sd, gpu, q, k, v, scale)[0], _run(sd, gpu, q[:1], k[:1], v[:1], scale)[0])
