"""FLASH_ATTN_EXT with an f16 mask at head dims 64 / 128 (k_flash_mask, kernels/flash_mask.hip) against the float64 softmax(scale q k^T + m) v on the f16-rounded
K, V and mask: -inf keys excluded, a row with no live key defined as zeros (the convention of the CPU kernel restated in oracle/ggml_cpu_ref.cpp).

Cases (d, Lq, Lk, HN, Hm) for 64-key tiles and 128-query workgroups: CLIP's 77 x 77 (odd Lk: 2-byte aligned mask rows, a full tile + a 13-key tail), less than a tile of
each, exact tiles with HN = 2 Hm, a one-key tail tile with a partial query block and per-head planes, and two workgroups per head over four key tiles with a mask of
160 > Lq rows (the padding rows hold 3e4: read as data they would swamp the row).  Mask kinds: `causal` (Lq == Lk), `bias` N(0, 2), `keypad` (the last third of the
keys -inf: at Lk = 200 a whole trailing tile), `lead` (the first 64 keys -inf, or the first half: the running max is still -inf when the first live key arrives),
`deadrows` (bias, every 5th row all -inf), `floor` (keypad with f16's -65504).  Scores: the two families of tests/attn_scores.py that move the deferred max late.

Bars: rel-L2 < 4e-3 (tests/test_gpu_flash_wide.py, tests/test_gpu_attention_scores.py for f16 operands); per row max-abs <= 3e-3 max(1, |ref row|max); dead rows
exactly 0.0; two runs bit-equal; head 0 of a 3-head launch equals its single-head run on plane 0 bit for bit."""
import os

import numpy as np
import pytest

import attn_scores as AS
from ggml_graph import F16, Graph

pytestmark = pytest.mark.gpu

CASES = [(64, 77, 77, 2, 1), (64, 5, 20, 1, 1), (64, 64, 64, 4, 2), (128, 33, 129, 3, 3), (128, 130, 200, 2, 1)]
MASKS = ("causal", "bias", "keypad", "lead", "deadrows", "floor")
SCORES = ("ramp12", "spike_last")
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"   # (harness self-check on a CPU-only box: both sides run the oracle)
OTHERS = ("gemm_attention", "flash_short_launches", "flash_qb2_launches", "flash_mslot_launches", "flash_generic_launches", "flash_short_ip_launches", "flash_wide_launches")


def _mask(kind, Lq, Lk, Hm, rng):
    """f32 [Hm, Lqm, Lk]; Lqm = 160 at Lq = 130 (rows beyond Lq are padding), else Lq"""
    Lqm = 160 if Lq == 130 else Lq
    m = np.zeros((Hm, Lqm, Lk), np.float32)
    if kind in ("bias", "deadrows"):
        m = rng.normal(0.0, 2.0, m.shape).astype(np.float32)
    if kind == "causal":
        m[:, np.arange(Lk)[None, :] > np.arange(Lqm)[:, None]] = -np.inf
    elif kind in ("keypad", "floor"):
        m[:, :, Lk - (Lk + 2) // 3:] = -np.inf if kind == "keypad" else -65504.0
    elif kind == "lead":
        m[:, :, :64 if Lk > 64 else Lk // 2] = -np.inf
    elif kind == "deadrows":
        m[:, ::5] = -np.inf
    m[:, Lq:] = 3e4
    return m


def _inputs(d, Lq, Lk, HN, Hm, mkind, skind):
    rng = np.random.default_rng([d, Lq, Lk, MASKS.index(mkind), SCORES.index(skind)])
    return (*AS.make_heads(skind, Lq, Lk, d, HN, rng), _mask(mkind, Lq, Lk, Hm, rng), 1.0 / np.sqrt(d))


def _ref(q, k, v, m, scale):
    k16, v16, m16 = AS.f16r(k), AS.f16r(v), AS.f16r(m)
    out = np.zeros(q.shape[:2] + (v.shape[-1],))
    for h in range(q.shape[0]):
        s = (q[h].astype(np.float64) @ k16[h].T) * scale + m16[h % m.shape[0], :q.shape[1]]
        top = s.max(-1, keepdims=True)
        p = np.exp(s - np.where(np.isfinite(top), top, 0.0))           # a dead row: exp(-inf) = 0 everywhere
        l = p.sum(-1, keepdims=True)
        out[h] = np.where(l > 0, (p @ v16[h]) / np.where(l > 0, l, 1.0), 0.0)
    return out


def _run(sd, gpu, q, k, v, m, scale):
    """the node on the device: claimed, and counted under flash_mask_launches alone -> [HN, Lq, d]"""
    counting = ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")
    before = sd.backend_stats() if counting else None
    with Graph(gpu) as g:
        L = sd.lib()
        node = L.ggml_flash_attn_ext(g.ctx, g.input(q), g.input(k, F16), g.input(v, F16), g.input(m, F16), scale, 0.0, 0.0)
        L.ggml_flash_attn_ext_set_prec(node, 10)
        assert g.supports(node)
        out = g.run(node)
    if counting:
        after = sd.backend_stats()
        assert after["flash_mask_launches"] - before["flash_mask_launches"] >= 1
        assert all(after[n] == before[n] for n in OTHERS), {n: after[n] - before[n] for n in OTHERS}
    assert out.shape == (1, q.shape[1], q.shape[0], q.shape[2])
    return out[0].transpose(1, 0, 2)


@pytest.mark.parametrize("skind", SCORES)
@pytest.mark.parametrize("d,Lq,Lk,HN,Hm,mkind", [(*c, mk) for c in CASES for mk in MASKS if mk != "causal" or c[1] == c[2]])
def test_flash_mask_node_vs_float64_softmax(sd, gpu, d, Lq, Lk, HN, Hm, mkind, skind):
    q, k, v, m, scale = _inputs(d, Lq, Lk, HN, Hm, mkind, skind)
    out = _run(sd, gpu, q, k, v, m, scale)
    np.testing.assert_array_equal(out, _run(sd, gpu, q, k, v, m, scale))
    assert np.isfinite(out).all()
    ref = _ref(q, k, v, m, scale)
    dead = ~np.isfinite(AS.f16r(m)[:, :Lq].max(-1))[np.arange(HN) % Hm]      # [HN, Lq]
    err, bar = AS.rel_l2(out, ref), 4e-3 if ON_GPU else 1e-2                   # (the oracle's flash node accumulates V in f16)
    row_err, row_bar = np.abs(out - ref).max(-1), 3e-3 * np.maximum(1.0, np.abs(ref).max(-1))
    print(f"[flash-mask] d={d} Lq={Lq} Lk={Lk} HN={HN} Hm={Hm} {mkind} {skind}: rel-L2 {err:.3e} (bar {bar:.1e}); worst row / bar {float((row_err / row_bar).max()):.3f}; dead rows {int(dead.sum())}")
    assert (out[dead] == 0.0).all()
    assert err < bar
    if ON_GPU:
        assert (row_err <= row_bar).all(), np.argwhere(row_err > row_bar)[:4].tolist()


@pytest.mark.parametrize("mkind", ["bias", "lead"])
def test_flash_mask_head_is_independent_of_the_launch(sd, gpu, mkind):
    """(128, 33, 129): head 0 of a 3-head launch with Hm = 3 equals its single-head run with Hm = 1 and plane 0, bit for bit"""
    q, k, v, m, scale = _inputs(128, 33, 129, 3, 3, mkind, "ramp12")
    np.testing.assert_array_equal(_run(sd, gpu, q, k, v, m, scale)[0], _run(sd, gpu, q[:1], k[:1], v[:1], m[:1], scale)[0])
