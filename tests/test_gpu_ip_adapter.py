"""IP-Adapter on the MI355X: k_flash_short_ip (text keys + image keys of the same q, SCALE and ADD in one launch) through the planner pattern on raw graphs
(tests/ggml_graph.py), its nearest misses through the plain nodes, operand placement (recycled blocks, hoisted K / V), the tiny UNets with image tokens
against the oracle backend and against fuse_ip_attn=0, and trajectories with the token state of sd_set_ip_adapter: device sampler and host loop against the oracle,
strength 0, replay of the captured step graph with other tokens, an armed step cache with previews, the three-branch inpaint variant.

Bars.  Kernel level, the bar of tests/test_gpu_attention_scores.py: rel-L2 against the float64 result on the f16-rounded K / V below max(2e-3, 3 s), s the rel-L2
of the kernel's operand-rounding MODEL (tests/ip_adapter_ref.py) against the same exact result, computed here and printed before it is asserted; on the spike
kinds also per query row max-abs <= 3e-3 max(1, |ref row|max); two runs bit-equal.  Where a Linear stands behind the ADD (the f16 operand image route) the model
also rounds the attention output to f16, as the image does.  Model level, the bar of tests/test_gpu_concat_cfg.py: one forward rel-L2 < 5e-3 against the oracle.
A masked FLASH_ATTN_EXT is not a near miss that can run: the backend's supports_op refuses the node (the host then builds the manual chain), asserted below.
The counter assertions are skipped under SDCPP_BACKEND_OPTS and with SDCPP_GPU_TESTS_ON_ORACLE=1."""
import os

import numpy as np
import pytest

import attn_scores as AS
import ip_adapter_ref as IP
from ggml_graph import F16, F32, Graph, tensor_struct

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
STATS = ("fused_ip_attn", "flash_short_ip_launches", "flash_short_launches", "flash_out_alias", "fused_q16")


def _counting():
    return ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")


def _make(d, H, N, Lq, Lk, Li, kind):
    """q [HN, Lq, d] (f16-representable: an identity projection in front reproduces it exactly), k / v [HN, Lk, d], k_ip / v_ip [HN, Li, d]; the kind's key profile
    (spikes included) sits on the image keys too"""
    rng = np.random.default_rng([d, H * N, Lq, Lk, Li, AS.KINDS.index(kind)])
    q, k, v = AS.make_heads(kind, Lq, Lk, d, H * N, rng)
    _, ki, vi = AS.make_heads(kind, Lq, Li, d, H * N, rng)
    return AS.f16r(q).astype(np.float32), k, v, ki, vi


def _tokens(a, H):
    """[N * H, L, d] -> [N, L, H * d]"""
    return np.ascontiguousarray(IP.heads_to_tokens(a, H)).astype(np.float32)


def _attn_tail(g, L, fa, d, H, Lq, N):
    ts = tensor_struct(fa)
    vw = L.ggml_view_4d(g.ctx, fa, d, H, Lq, N, ts.nb[1], ts.nb[2], ts.nb[1] * H, 0)
    ct = L.ggml_cont(g.ctx, vw)
    return ct, L.ggml_reshape_3d(g.ctx, ct, d * H, Lq, N)


def _heads(g, L, x, d, H, Lq, N):
    """[C, Lq, N] -> [d, Lq, H * N] as ggml_ext_attention_ext splits the heads"""
    x = L.ggml_reshape_4d(g.ctx, x, d, H, Lq, N)
    x = L.ggml_cont(g.ctx, L.ggml_permute(g.ctx, x, 0, 2, 1, 3))
    return L.ggml_reshape_3d(g.ctx, x, d, Lq, H * N)


def _build(g, L, data, d, H, N, ip_scale, *, qproj=False, out16=False, w_out=None, computed=False, variant=None):
    """the graph of block.hpp:380-389 on caller tensors.  qproj: q through an (identity) to_q Linear and one head split per attention, as the model emits it;
    out16: a Linear behind the ADD; computed: every operand is a graph node (its block can be recycled); variant: one of the near misses"""
    q, k, v, ki, vi = data
    Lq = q.shape[1]
    scale = 1.0 / np.sqrt(d)
    C = d * H
    if qproj:
        tx = g.input(_tokens(q, H))
        ql = L.ggml_mul_mat(g.ctx, g.weight(np.eye(C, dtype=np.float32), F16), tx)
        qa, qb = _heads(g, L, ql, d, H, Lq, N), _heads(g, L, ql, d, H, Lq, N)
    else:
        qa = g.input(q)
        if computed:
            qa = L.ggml_scale(g.ctx, qa, 1.0)
        qb = qa
        if variant == "other_q":
            qb = g.input(q.copy())
    if computed:
        tk, tv, tki, tvi = (L.ggml_cast(g.ctx, g.input(a), F16) for a in (k, v, ki, vi))
    else:
        tk, tv, tki, tvi = (g.input(a, F16) for a in (k, v, ki, vi))
    fa = L.ggml_flash_attn_ext(g.ctx, qa, tk, tv, None, scale, 0.0, 0.0)
    L.ggml_flash_attn_ext_set_prec(fa, 10)
    ca, ra = _attn_tail(g, L, fa, d, H, Lq, N)
    fb = L.ggml_flash_attn_ext(g.ctx, qb, tki, tvi, None, scale, 0.0, 0.0)
    L.ggml_flash_attn_ext_set_prec(fb, 10)
    cb, rb = _attn_tail(g, L, fb, d, H, Lq, N)
    sc = L.ggml_scale(g.ctx, rb, ip_scale)
    add = L.ggml_add(g.ctx, sc, ra) if variant == "swapped" else L.ggml_add(g.ctx, ra, sc)
    outs = [L.ggml_mul_mat(g.ctx, g.weight(w_out, F16), add) if out16 else L.ggml_dup(g.ctx, add)]
    if variant == "scale_reader":
        outs.append(L.ggml_dup(g.ctx, sc))
    elif variant == "cont_reader":
        outs.append(L.ggml_dup(g.ctx, ca))
    elif variant == "flash_reader":
        outs.append(L.ggml_dup(g.ctx, fb))
    elif variant == "scale_output":
        outs.append(sc)
    return outs


def _reference(data, d, H, ip_scale, out16, w_out):
    q, k, v, ki, vi = data
    scale = 1.0 / np.sqrt(d)
    k16, v16, ki16, vi16 = (AS.f16r(a) for a in (k, v, ki, vi))
    exact = IP.heads_to_tokens(IP.exact(q, k16, v16, ki16, vi16, scale, ip_scale), H)
    fused = IP.heads_to_tokens(IP.fused_model(q, k16, v16, ki16, vi16, scale, ip_scale), H)
    plain = IP.heads_to_tokens(IP.plain_model(q, k16, v16, ki16, vi16, scale, ip_scale), H)
    if out16:
        w = AS.f16r(w_out).T
        exact, fused, plain = exact @ w, AS.f16r(fused) @ w, AS.f16r(plain) @ w
    return exact, fused, plain


def _check(tag, out, exact, model, kind):
    assert np.isfinite(out).all()
    s, err = AS.rel_l2(model, exact), AS.rel_l2(out, exact)
    bar = max(2e-3, 3.0 * s) if ON_GPU else max(1e-2, 3.0 * s)   # self-check mode: the oracle's flash node accumulates V in f16
    row_err = np.abs(out - exact).max(-1)
    row_bar = 3e-3 * np.maximum(1.0, np.abs(exact).max(-1))
    print(f"[ip-adapter] {tag} {kind}: rel-L2 vs exact {err:.3e} (bar {bar:.1e}, model s {s:.3e}); worst row max-abs / bar {float((row_err / row_bar).max()):.3f}")
    assert err < bar
    if kind.startswith("spike") and ON_GPU:
        bad = np.argwhere(row_err > row_bar)
        assert bad.size == 0, f"{len(bad)} rows beyond 3e-3: first {bad[:4].tolist()}"


def _run(sd, gpu, build, runs=2):
    """the graph `runs` times on fresh backends; returns (outputs of run 0, per-run statistic deltas or None)"""
    outs, deltas = [], []
    for _ in range(runs):
        s0 = sd.backend_stats() if _counting() else None
        with Graph(gpu) as g:
            nodes = build(g, sd.lib())
            assert all(g.supports(n) for n in nodes)
            res = g.run(*nodes)
            outs.append(res if isinstance(res, list) else [res])
        if s0 is not None:
            s1 = sd.backend_stats()
            deltas.append({f: s1[f] - s0[f] for f in STATS})
    for a, b in zip(outs[0], outs[-1]):
        np.testing.assert_array_equal(a, b)
    return outs[0], (deltas if deltas else None)


# (d, H, N, Lq, Lk, Lk_ip, ip_scale, kind, q through to_q (f16 image), Linear behind the ADD (f16 operand image)): every value of every axis, and the corners
CASES = [
    (8, 2, 1, 1, 65, 1, 1.0, "ramp3", False, False),          # the smallest of everything; one query, one image key
    (40, 2, 2, 31, 77, 4, 0.35, "spike_last", False, True),   # ragged single block; spike on image key 3 (lane half 0's last of its first four)
    (64, 2, 1, 33, 96, 16, -0.5, "spike_mid", True, False),   # two blocks, the second with one row; negative scale; spike on image key 8
    (64, 2, 2, 129, 77, 32, 2.0, "ramp12", True, True),       # five blocks over two workgroups; every image key valid; both images
    (40, 8, 1, 129, 96, 32, 1.0, "offset_pos", True, True),   # SD1.5's 320-wide level: 8 heads of 40
    (8, 64, 64, 33, 65, 4, 0.35, "descend", False, False),    # ceil(33 / 32) * 4096 = 8192 blocks: two query blocks per wave (qi = 2), the second past the end
    (64, 1, 1, 33, 65, 1, 2.0, "offset_neg", False, True),    # one image key: P_ip = ip_scale on every row
    (8, 2, 1, 129, 96, 16, -0.5, "spike_last", True, False),  # spike on image key 15: the last key of the first P V step
    (64, 2, 1, 129, 96, 32, 1.0, "spike_mid", False, False),  # the f32-Q d = 64 instantiation (the widest register set) at every limit
    (40, 2, 1, 33, 77, 31, 1.0, "spike_last", False, False),  # 31 image keys: one masked key, in lane half 1's last register
]


@pytest.mark.parametrize("d,H,N,Lq,Lk,Li,ip_scale,kind,qproj,out16", CASES)
def test_fused_kernel(sd, gpu, d, H, N, Lq, Lk, Li, ip_scale, kind, qproj, out16):
    data = _make(d, H, N, Lq, Lk, Li, kind)
    w_out = np.random.default_rng(d + Lq).standard_normal((d * H, d * H)).astype(np.float32) / np.sqrt(d * H) if out16 else None
    exact, fused, plain = _reference(data, d, H, ip_scale, out16, w_out)
    tag = f"fused d={d} H={H} N={N} Lq={Lq} Lk={Lk} Lk_ip={Li} s={ip_scale} q16={int(qproj)} out16={int(out16)}"
    s_f, s_p = AS.rel_l2(fused, exact), AS.rel_l2(plain, exact)
    print(f"[ip-adapter] {tag}: model fused {s_f:.3e}, model plain {s_p:.3e}")
    assert s_p < max(2e-3, 3.0 * s_f)   # (CPU) the plain-node route, modelled the same way, stays inside the bar on these inputs
    (out,), deltas = _run(sd, gpu, lambda g, L: _build(g, L, data, d, H, N, ip_scale, qproj=qproj, out16=out16, w_out=w_out))
    assert out.shape[-3:] == (N, Lq, d * H)
    _check(tag, out.reshape(N, Lq, d * H), exact, fused, kind)
    if deltas:
        for dl in deltas:
            assert dl["fused_ip_attn"] == 1 and dl["flash_short_ip_launches"] == 1 and dl["flash_short_launches"] == 0 and dl["flash_out_alias"] == 0, dl
            assert dl["fused_q16"] == (1 if qproj and Lq >= 32 else 0), dl   # Q stays an f16 image: one, read by the one launch


MISSES = [
    ("Lk=64", dict(Lk=64), None), ("Lk=97", dict(Lk=97), None), ("Lk_ip=33", dict(Li=33), None), ("d=72", dict(d=72), None),
    ("other q node", {}, "other_q"), ("ADD(B, A)", {}, "swapped"), ("SCALE read twice", {}, "scale_reader"), ("A's CONT read twice", {}, "cont_reader"),
    ("second flash node read twice", {}, "flash_reader"), ("SCALE is an output", {}, "scale_output"), ("fuse_ip_attn=0", {}, "option"),
]


@pytest.mark.parametrize("name,shape,variant", MISSES, ids=[m[0] for m in MISSES])
def test_nearest_misses_run_as_plain_nodes(sd, gpu, name, shape, variant):
    p = dict(d=40, H=2, N=1, Lq=33, Lk=77, Li=4)
    p.update(shape)
    d, H, N, Lq, Lk, Li = (p[k] for k in ("d", "H", "N", "Lq", "Lk", "Li"))
    data = _make(d, H, N, Lq, Lk, Li, "spike_last")
    exact, fused, plain = _reference(data, d, H, 0.35, False, None)
    if variant == "option" and ON_GPU:
        sd.backend_set_option("fuse_ip_attn", 0)
    try:
        outs, deltas = _run(sd, gpu, lambda g, L: _build(g, L, data, d, H, N, 0.35, variant=None if variant == "option" else variant))
    finally:
        if variant == "option" and ON_GPU:
            sd.backend_set_option("fuse_ip_attn", 1)
    model = plain   # (ip_adapter_ref.plain_model states the kernel each node takes at these shapes)
    _check(f"miss [{name}]", outs[0].reshape(N, Lq, d * H), exact, model, "spike_last")
    if deltas:
        for dl in deltas:
            assert dl["fused_ip_attn"] == 0 and dl["flash_short_ip_launches"] == 0 and dl["flash_out_alias"] == 0, (name, dl)


def test_masked_flash_node_is_not_claimed(sd, gpu):
    """the mask form of the near miss: supports_op refuses a masked FLASH_ATTN_EXT, so such a pair never reaches the planner"""
    if not ON_GPU:
        pytest.skip("the oracle backend takes masked flash nodes")
    q, k, v, _, _ = _make(40, 2, 1, 32, 77, 4, "ramp3")
    with Graph(gpu) as g:
        L = sd.lib()
        mask = g.input(np.zeros((1, 1, 32, 77), np.float32), F16)
        node = L.ggml_flash_attn_ext(g.ctx, g.input(q), g.input(k, F16), g.input(v, F16), mask, 1.0 / np.sqrt(40), 0.0, 0.0)
        assert not g.supports(node)


@pytest.mark.parametrize("N", [1, 2, 3, 4])
@pytest.mark.parametrize("Lq,Li", [(33, 4), (16, 32), (64, 16)])
def test_recycled_operand_blocks(sd, gpu, N, Lq, Li):
    """every operand a graph NODE (q a SCALE, K / V casts), so the allocator may hand a dead operand's block to the ADD — Lq = Lk_ip / 2 makes the image K / V casts
    exactly the ADD's size, and q always is.  Whatever it does: the pair is either fused, or refused and counted in flash_out_alias (the statistic of the
    existing FLASH_ATTN_EXT -> CONT guard, which this guard extends to five operands and to the nodes between the two attentions), never both or neither, and the result is the plain nodes' within the bar."""
    d, H, Lk = 40, 2, 77
    data = _make(d, H, N, Lq, Lk, Li, "spike_last")
    exact, fused, plain = _reference(data, d, H, 0.35, False, None)
    build = lambda g, L: _build(g, L, data, d, H, N, 0.35, computed=True)
    (out,), deltas = _run(sd, gpu, build)
    _check(f"recycled N={N} Lq={Lq} Lk_ip={Li}", out.reshape(N, Lq, d * H), exact, fused, "spike_last")
    if deltas:
        print(f"[ip-adapter] recycled N={N} Lq={Lq} Lk_ip={Li}: {deltas[0]}")
        for dl in deltas:
            # (a refused pair runs as two plain FLASH_ATTN_EXT -> CONT chains, whose own guard may count in the same statistic)
            assert (dl["fused_ip_attn"], dl["flash_out_alias"] == 0) in ((1, True), (0, False)) and dl["flash_short_ip_launches"] == dl["fused_ip_attn"], dl
    if ON_GPU:
        sd.backend_set_option("fuse_ip_attn", 0)
        try:
            (ref,), _ = _run(sd, gpu, build, runs=1)
        finally:
            sd.backend_set_option("fuse_ip_attn", 1)
        _check(f"recycled N={N} Lq={Lq} Lk_ip={Li} (plain)", ref.reshape(N, Lq, d * H), exact, plain, "spike_last")
        assert AS.rel_l2(out, ref) < 2 * max(2e-3, 3.0 * AS.rel_l2(fused, exact))


# ---------------------------------------------------------------------------------------------------------------- model level
IP_DIM, CLIP_DIM = 32, 48


@pytest.fixture(scope="module")
def engines(sd, gpu, oracle):
    made = {}

    def get(name, backend):
        if (name, backend) not in made:
            e = sd.Engine(model=getattr(sd, name), backend=backend, flash_attn=True)
            e.ip_adapter_init(IP_DIM, CLIP_DIM, 4, weight_seed=7)
            made[(name, backend)] = e
        return made[(name, backend)]

    return get


def _model_inputs(e, name, n=2):
    rng = np.random.default_rng(11)
    ctx_dim = next(e.tensor_info(t)[0][0] for t in e.tensor_names() if t.endswith("attn2.to_k.weight"))
    x = rng.standard_normal((n, 4, 16, 16)).astype(np.float32)
    t = np.full(n, 500.0, np.float32)
    c = rng.standard_normal((1, 77, ctx_dim)).astype(np.float32)
    y = None
    if name == "SDXL_TINY":
        adm = next(e.tensor_info(tn)[0][0] for tn in e.tensor_names() if tn.endswith("label_emb.0.0.weight"))
        y = rng.standard_normal((1, adm)).astype(np.float32)
    return x, t, c, y


@pytest.mark.parametrize("name", ["SD15_TINY", "SDXL_TINY"])
@pytest.mark.parametrize("n_ip", [4, 16])
@pytest.mark.parametrize("hoist", [1, 0])
def test_forward_with_tokens_against_oracle(sd, gpu, oracle, engines, name, n_ip, hoist):
    """one forward with image tokens: against the oracle (< 5e-3), fused against fuse_ip_attn=0 (each within 5e-3 of the oracle, so within 1e-2 of each other),
    bit-equal when repeated, with the K / V projections of the text and of the tokens hoisted (default) and in place (hoist_kv=0)."""
    e, r = engines(name, gpu), engines(name, oracle)
    x, t, c, y = _model_inputs(e, name)
    tok = np.random.default_rng(n_ip).standard_normal((1, n_ip, IP_DIM)).astype(np.float32)
    want = r.unet_forward(x, t, c, y, ip_context=tok, ip_scale=0.6)
    n_attn2 = sum(1 for n in e.tensor_names() if n.endswith("attn2.to_k.weight"))
    if ON_GPU:
        sd.backend_set_option("hoist_kv", hoist)
    try:
        s0 = sd.backend_stats() if _counting() else None
        got = e.unet_forward(x, t, c, y, ip_context=tok, ip_scale=0.6)
        s1 = sd.backend_stats() if _counting() else None
        again = e.unet_forward(x, t, c, y, ip_context=tok, ip_scale=0.6)
        np.testing.assert_array_equal(got, again)
        if ON_GPU:
            sd.backend_set_option("fuse_ip_attn", 0)
        plain = e.unet_forward(x, t, c, y, ip_context=tok, ip_scale=0.6)
    finally:
        if ON_GPU:
            sd.backend_set_option("fuse_ip_attn", 1)
            sd.backend_set_option("hoist_kv", 1)
    err, err_p = AS.rel_l2(got, want), AS.rel_l2(plain, want)
    print(f"[ip-adapter] {name} {n_ip} tokens hoist_kv={hoist}: rel-L2 vs oracle fused {err:.3e}, plain nodes {err_p:.3e}, fused vs plain {AS.rel_l2(got, plain):.3e}")
    assert np.isfinite(got).all() and err < 5e-3 and err_p < 5e-3
    if s0 is not None:
        fused, refused = s1["fused_ip_attn"] - s0["fused_ip_attn"], s1["flash_out_alias"] - s0["flash_out_alias"]
        print(f"[ip-adapter] {name}: {n_attn2} attn2, fused {fused}, refused for operand placement {refused}, q16 {s1['fused_q16'] - s0['fused_q16']}")
        if hoist:   # the text K / V sit in the arena: nothing stands in the way of any pair
            assert fused == n_attn2 and refused == 0
        else:       # K / V left in the graph buffer may not outlive the nodes between the two attentions: such a pair is refused, counted, and runs plain
            assert 0 <= fused <= n_attn2 and (fused == n_attn2 or refused >= 1)
        assert s1["flash_short_ip_launches"] - s0["flash_short_ip_launches"] == fused


@pytest.mark.parametrize("name", ["SD15_TINY", "SDXL_TINY"])
def test_zero_scale_and_no_tokens_are_the_plain_forward(sd, gpu, engines, name):
    e = engines(name, gpu)
    x, t, c, y = _model_inputs(e, name)
    tok = np.ones((1, 4, IP_DIM), np.float32)
    plain = sd.Engine(model=getattr(sd, name), backend=gpu, flash_attn=True)
    want = plain.unet_forward(x, t, c, y)
    s0 = sd.backend_stats() if _counting() else None
    np.testing.assert_array_equal(e.unet_forward(x, t, c, y), want)
    np.testing.assert_array_equal(e.unet_forward(x, t, c, y, ip_context=tok, ip_scale=0.0), want)
    if s0 is not None:
        assert sd.backend_stats()["fused_ip_attn"] == s0["fused_ip_attn"]


# ---------------------------------------------------------------------------------------------------------------- trajectories (sd_set_ip_adapter)
# Bars as in tests/test_gpu_concat_cfg.py: a three-step Euler-A trajectory < 3 x 5e-3 against the oracle — the per-forward error enters each update once, so it adds at
# most linearly over the steps.  Fused against fuse_ip_attn=0: each within that bar of the oracle.
def _ip_traj(sd, e, **over):
    rng = np.random.default_rng(5)
    ctx_dim = next(e.tensor_info(t)[0][0] for t in e.tensor_names() if t.endswith("attn2.to_k.weight"))
    cond, uncond = rng.standard_normal((1, 77, ctx_dim)).astype(np.float32), rng.standard_normal((1, 77, ctx_dim)).astype(np.float32)
    kw = dict(width=128, height=128, steps=3, cfg=7.5, seed=11, batch=2, method=sd.EULER_A, device_sampler=True, fuse_cfg=True)
    if any(n.endswith("label_emb.0.0.weight") for n in e.tensor_names()):
        adm = next(e.tensor_info(n)[0][0] for n in e.tensor_names() if n.endswith("label_emb.0.0.weight"))
        kw["cond_y"], kw["uncond_y"] = rng.standard_normal((1, adm)).astype(np.float32), rng.standard_normal((1, adm)).astype(np.float32)
    kw.update(over)
    return e.sample_latents(cond, uncond, **kw)


def _tokens_pair(seed, n=4):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, IP_DIM)).astype(np.float32), rng.standard_normal((n, IP_DIM)).astype(np.float32)


@pytest.mark.parametrize("name", ["SD15_TINY", "SDXL_TINY"])
@pytest.mark.parametrize("device", [True, False])
def test_trajectory_against_oracle_fused_and_plain(sd, gpu, oracle, engines, name, device):
    e, r = engines(name, gpu), engines(name, oracle)
    tok, un = _tokens_pair(3)
    try:
        for x in (e, r):
            x.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.6)
        want = _ip_traj(sd, r, device_sampler=device)
        s0 = sd.backend_stats() if _counting() else None
        got = _ip_traj(sd, e, device_sampler=device)
        fused = sd.backend_stats()["fused_ip_attn"] - s0["fused_ip_attn"] if s0 else None
        np.testing.assert_array_equal(_ip_traj(sd, e, device_sampler=device), got)
        if ON_GPU:
            sd.backend_set_option("fuse_ip_attn", 0)
        plain = _ip_traj(sd, e, device_sampler=device)
        e.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.0)
        off = _ip_traj(sd, e, device_sampler=device)
    finally:
        if ON_GPU:
            sd.backend_set_option("fuse_ip_attn", 1)
        for x in (e, r):
            x.set_ip_adapter()
    err, err_p = AS.rel_l2(got, want), AS.rel_l2(plain, want)
    print(f"[ip-adapter] {name} 3-step Euler-A, {'device sampler' if device else 'host loop'}: rel-L2 vs oracle fused {err:.3e}, plain nodes {err_p:.3e}; pairs fused {fused}")
    assert np.isfinite(got).all() and err < 3 * 5e-3 and err_p < 3 * 5e-3
    if fused is not None:
        assert fused >= 1
    np.testing.assert_array_equal(off, _ip_traj(sd, e, device_sampler=device))   # strength 0 == tokens cleared == no adapter
    if name == "SD15_TINY":
        bare = sd.Engine(model=getattr(sd, name), backend=gpu, flash_attn=True)
        np.testing.assert_array_equal(off, _ip_traj(sd, bare, device_sampler=device))


def test_replay_with_other_tokens_is_a_fresh_context(sd, gpu, engines):
    """the step graph is captured once (hipGraph) with the arena addresses of the f16 Q image and of the fused launches' operands; a second trajectory with OTHER
    tokens of the same shape replays it — and must give what a context that never saw the first tokens gives"""
    e = engines("SD15_TINY", gpu)
    a, b = _tokens_pair(7), _tokens_pair(8)
    fresh = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    fresh.ip_adapter_init(IP_DIM, CLIP_DIM, 4, weight_seed=7)
    try:
        e.set_ip_adapter(tokens=a[0], uncond_tokens=a[1], strength=0.6)
        first = _ip_traj(sd, e)
        s0 = sd.backend_stats() if _counting() else None
        e.set_ip_adapter(tokens=b[0], uncond_tokens=b[1], strength=0.6)
        second = _ip_traj(sd, e)
        if s0 is not None:
            s1 = sd.backend_stats()
            assert s1["plans_built"] == s0["plans_built"] and s1["graph_replays"] > s0["graph_replays"]
        fresh.set_ip_adapter(tokens=b[0], uncond_tokens=b[1], strength=0.6)
        np.testing.assert_array_equal(second, _ip_traj(sd, fresh))
        assert not np.array_equal(first, second)
    finally:
        e.set_ip_adapter()


def test_step_cache_and_previews_with_an_adapter(sd, gpu, engines):
    """an armed step cache (skip-step graphs run) and previews on: the final latents are those of the same run without previews, bit for bit"""
    e = engines("SD15_TINY", gpu)
    tok, un = _tokens_pair(9)
    frames = []
    try:
        e.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.6)
        e.set_step_cache(sd.CACHE_UCACHE, reuse_threshold=1.0)
        plain = _ip_traj(sd, e, steps=12, method=sd.EULER)
        assert any(r["skipped"] for r in e.step_cache_trace())
        e.set_preview(lambda step, fr, noisy, first: frames.append(step), interval=3)
        got = _ip_traj(sd, e, steps=12, method=sd.EULER)
        assert got.tobytes() == plain.tobytes() and len(frames) >= 4
        e.set_step_cache(None)
        no_cache = _ip_traj(sd, e, steps=12, method=sd.EULER)
        e.set_preview(None)
        np.testing.assert_array_equal(no_cache, _ip_traj(sd, e, steps=12, method=sd.EULER))
    finally:
        e.set_preview(None)
        e.set_step_cache(None)
        e.set_ip_adapter()


def test_inpaint_variant_three_branches(sd, gpu, oracle):
    """an inpaint UNet with image guidance: cond, uncond and img_uncond in one graph — the cond seat sees the tokens, the two others the uncond tokens — device sampler
    and host loop against the oracle (< 3 x 5e-3), and different from the run with the token sets swapped"""
    tok, un = _tokens_pair(13)
    cat = np.random.default_rng(61).standard_normal((1, 5, 16, 16)).astype(np.float32)
    cat[:, 0] = cat[:, 0] > 0
    eng = []
    for backend in (gpu, oracle):
        x = sd.Engine(model=sd.SD15_TINY, backend=backend, flash_attn=True, variant=sd.UNET_INPAINT)
        x.ip_adapter_init(IP_DIM, CLIP_DIM, 4, weight_seed=7)
        x.set_concat_condition(cat)
        x.set_img_cfg(1.5)
        x.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.6)
        eng.append(x)
    e, r = eng
    want = _ip_traj(sd, r)
    for device in (True, False):
        got = _ip_traj(sd, e, device_sampler=device)
        err = AS.rel_l2(got, want)
        print(f"[ip-adapter] inpaint, 3 branches, {'device sampler' if device else 'host loop'}: rel-L2 vs oracle {err:.3e}")
        assert np.isfinite(got).all() and err < 3 * 5e-3
    e.set_ip_adapter(tokens=un, uncond_tokens=tok, strength=0.6)
    assert AS.rel_l2(_ip_traj(sd, e), want) > 3 * 5e-3
