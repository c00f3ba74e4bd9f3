"""IP-Adapter on the oracle backend: the adapter's parameters, the graph every attn2 emits with image tokens (block.hpp:382-389, node for node), the graph without
them (unchanged, bit for bit), the image projection against the NumPy restatement, the refusals, and a lane-by-lane replay of k_flash_short_ip's index logic
(in the manner of tests/test_kernel_logic.py) with the rounding models of tests/ip_adapter_ref.py, attn2 composed from the no-IP forward, and the samplers'
token state (sd_set_ip_adapter): default uncond tokens, swapped sets, a Python-driven loop bit for bit, the refusals."""
import numpy as np
import pytest

import attn_scores as AS
import ip_adapter_ref as IP
from ref_graphs import engine_graph_description, split_description

IP_DIM, CLIP_DIM = 32, 48
MODELS = ("SD15_TINY", "SDXL_TINY")


def _op(line):
    return line.split()[2]


def _inputs(sd, name, n=2):
    rng = np.random.default_rng(11)
    ctx_dim = {"SD15_TINY": 64}.get(name)
    e = sd.Engine(model=getattr(sd, name), backend="CPU-oracle", flash_attn=True)
    if ctx_dim is None:
        ctx_dim = next(e.tensor_info(t)[0][0] for t in e.tensor_names() if t.endswith("attn2.to_k.weight"))
    x = rng.standard_normal((n, 4, 16, 16)).astype(np.float32)
    t = np.full(n, 500.0, np.float32)
    c = rng.standard_normal((1, 77, ctx_dim)).astype(np.float32)
    y = None
    if name == "SDXL_TINY":
        adm = next(e.tensor_info(tn)[0][0] for tn in e.tensor_names() if tn.endswith("label_emb.0.0.weight"))
        y = rng.standard_normal((1, adm)).astype(np.float32)
    return e, x, t, c, y


@pytest.fixture(scope="module")
def pairs(sd, oracle):
    """per model: (engine without the adapter, engine with it, inputs)"""
    made = {}

    def get(name):
        if name not in made:
            plain, x, t, c, y = _inputs(sd, name)
            ip, *_ = _inputs(sd, name)
            ip.ip_adapter_init(IP_DIM, CLIP_DIM, 4, weight_seed=7)
            made[name] = (plain, ip, (x, t, c, y))
        return made[name]

    return get


@pytest.mark.parametrize("name", MODELS)
def test_adapter_parameters(pairs, name):
    """to_k_ip / to_v_ip [ip_dim -> inner], no bias, on every attn2 and on no attn1; the image projection; nothing else is added and no resident weight moves"""
    plain, ip, _ = pairs(name)
    assert plain.ip_adapter_info() is None and ip.ip_adapter_info() == (IP_DIM, CLIP_DIM, 4)
    base, names = plain.tensor_names(), ip.tensor_names()
    assert names[:len(base)] == base
    extra = names[len(base):]
    attn2 = [n[:-len("to_k.weight")] for n in base if n.endswith("attn2.to_k.weight")]
    want = [p + s for p in attn2 for s in ("to_k_ip.weight", "to_v_ip.weight")] + ["ip_adapter.image_proj." + s for s in ("proj.weight", "proj.bias", "norm.weight", "norm.bias")]
    assert sorted(extra) == sorted(want)
    assert not any("attn1" in n for n in extra)
    for p in attn2:
        inner = plain.tensor_info(p + "to_k.weight")[0][1]
        for s in ("to_k_ip.weight", "to_v_ip.weight"):
            assert tuple(ip.tensor_info(p + s)[0][:2]) == (IP_DIM, inner)
    for n in base[:: max(1, len(base) // 16)]:
        np.testing.assert_array_equal(plain.get_tensor(n), ip.get_tensor(n))


@pytest.mark.parametrize("name", MODELS)
def test_no_tokens_or_zero_scale_is_the_graph_without_the_adapter(pairs, name):
    plain, ip, (x, t, c, y) = pairs(name)
    tok = np.random.default_rng(3).standard_normal((1, 4, IP_DIM)).astype(np.float32)
    want = plain.unet_forward(x, t, c, y)
    d0 = split_description(engine_graph_description(lambda: plain.unet_forward(x, t, c, y), compute=False))
    for kw in ({}, {"ip_context": tok, "ip_scale": 0.0}):
        np.testing.assert_array_equal(ip.unet_forward(x, t, c, y, **kw), want)
        d1 = split_description(engine_graph_description(lambda: ip.unet_forward(x, t, c, y, **kw), compute=False))
        assert d1 == d0   # leafs and nodes, line for line: no IP node, no IP leaf


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("n_ip,ip_n", [(4, 1), (16, 2)])
def test_graph_with_tokens(pairs, name, n_ip, ip_n):
    """per attn2: two MUL_MATs on the tokens, one more FLASH_ATTN_EXT -> VIEW -> CONT -> RESHAPE chain on the SAME q, SCALE(ip_scale), ADD(x, scaled), then to_out —
    in the reference's order; everything outside those insertions is the graph without the adapter"""
    plain, ip, (x, t, c, y) = pairs(name)
    tok = np.random.default_rng(5).standard_normal((ip_n, n_ip, IP_DIM)).astype(np.float32)
    _, n0 = split_description(engine_graph_description(lambda: plain.unet_forward(x, t, c, y), compute=False))
    _, n1 = split_description(engine_graph_description(lambda: ip.unet_forward(x, t, c, y, ip_context=tok, ip_scale=0.35), compute=False))
    n_attn2 = sum(1 for n in plain.tensor_names() if n.endswith("attn2.to_k.weight"))
    cnt = lambda nodes, op: sum(1 for l in nodes if _op(l) == op)
    assert cnt(n1, "MUL_MAT") - cnt(n0, "MUL_MAT") == 2 * n_attn2
    assert cnt(n1, "FLASH_ATTN_EXT") - cnt(n0, "FLASH_ATTN_EXT") == n_attn2
    assert cnt(n1, "SCALE") - cnt(n0, "SCALE") == n_attn2
    assert cnt(n1, "ADD") - cnt(n0, "ADD") == n_attn2
    assert cnt(n1, "REPEAT") - cnt(n0, "REPEAT") == (1 if ip_n != x.shape[0] else 0)
    ops = [_op(l) for l in n1]
    src = lambda l: [s.split(":")[1] for s in l.split(" s=")[1].split()[0].split(",")]
    scale_bits = str(int(np.float32(0.35).view(np.uint32)))
    seen = 0
    for i, l in enumerate(n1):
        if _op(l) != "SCALE" or f"p={scale_bits} " not in l:
            continue
        seen += 1
        # ... FLASH(q,k,v) VIEW CONT RESHAPE | k_ip, v_ip projections | FLASH(q,k_ip,v_ip) VIEW CONT RESHAPE SCALE ADD MUL_MAT(to_out)
        assert ops[i - 4:i + 3] == ["FLASH_ATTN_EXT", "VIEW", "CONT", "RESHAPE", "SCALE", "ADD", "MUL_MAT"]
        fb = n1[i - 4]
        between = []
        j = i - 5
        while _op(n1[j]) != "RESHAPE" or _op(n1[j - 1]) != "CONT" or _op(n1[j - 2]) != "VIEW" or _op(n1[j - 3]) != "FLASH_ATTN_EXT":
            between.append(_op(n1[j]))
            j -= 1
        fa = n1[j - 3]
        # the same q: ggml_ext_attention_ext splits the heads itself, so each attention reads its own RESHAPE <- CONT <- PERMUTE <- RESHAPE of the ONE to_q output
        by_id = {n.split()[1]: n for n in n1}
        def q_root(flash):
            node, ops_ = by_id[src(flash)[0][1:]], []
            for _ in range(4):
                ops_.append(_op(node))
                node = by_id[src(node)[0][1:]]
            return ops_, node
        (oa, qa), (ob, qb) = q_root(fa), q_root(fb)
        assert oa == ob == ["RESHAPE", "CONT", "PERMUTE", "RESHAPE"] and qa == qb and _op(qa) == "MUL_MAT"
        assert src(n1[i + 1]) == ["n" + n1[j].split()[1], "n" + l.split()[1]]      # ADD(x, scaled)
        mm = [k for k in between if k == "MUL_MAT"]
        assert len(mm) == 2 and between.count("CPY") == 2                # to_k_ip, to_v_ip and their f16 casts ...
        assert between.count("CONT") == 3                                # ... the head-major copies of q, k_ip and v_ip, nothing else that computes
        first = seen == 1 and ip_n != x.shape[0]                         # (the first attn2 also reaches the REPEAT of the shared tokens to the batch)
        assert set(between) <= {"MUL_MAT", "CPY", "RESHAPE", "PERMUTE", "CONT"} | ({"REPEAT"} if first else set())
    assert seen == n_attn2


@pytest.mark.parametrize("name", MODELS)
def test_forward_with_tokens(pairs, name):
    """finite, different from the forward without tokens, odd in nothing: +s and -s move the output in different directions; a batch of equal tokens equals one shared token set"""
    plain, ip, (x, t, c, y) = pairs(name)
    tok = np.random.default_rng(9).standard_normal((1, 4, IP_DIM)).astype(np.float32)
    base = plain.unet_forward(x, t, c, y)
    a = ip.unet_forward(x, t, c, y, ip_context=tok, ip_scale=1.0)
    b = ip.unet_forward(x, t, c, y, ip_context=tok, ip_scale=-1.0)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert AS.rel_l2(a, base) > 1e-3 and AS.rel_l2(b, base) > 1e-3 and AS.rel_l2(a, b) > 1e-3
    both = ip.unet_forward(x, t, c, y, ip_context=np.repeat(tok, x.shape[0], axis=0), ip_scale=1.0)
    np.testing.assert_array_equal(both, a)


def test_image_projection(pairs):
    """sd_ip_adapter_project against the NumPy ImageProjModel on the stored (f16-rounded) weights.  Bar: the embeddings are f16-representable, so every product is
    exact in f32 and what remains is f32 summation over clip_dim = 48 terms and the LayerNorm's own f32 steps: rel-L2 < 48 * 2^-24 * 4 = 1.2e-5."""
    _, ip, _ = pairs("SD15_TINY")
    rng = np.random.default_rng(21)
    emb = rng.standard_normal((3, CLIP_DIM)).astype(np.float16).astype(np.float32)
    got = ip.ip_adapter_project(emb)
    w = {s: ip.get_tensor("ip_adapter.image_proj." + s) for s in ("proj.weight", "proj.bias", "norm.weight", "norm.bias")}
    want = IP.image_proj(emb, w["proj.weight"].reshape(4 * IP_DIM, CLIP_DIM), w["proj.bias"], w["norm.weight"], w["norm.bias"], 4)
    err = AS.rel_l2(got, want)
    print(f"[ip-adapter] image projection rel-L2 vs float64 {err:.3e}")
    assert got.shape == (3, 4, IP_DIM) and err < 1.2e-5
    zero = ip.ip_adapter_project(np.zeros((1, CLIP_DIM), np.float32))
    assert np.abs(zero).max() > 0.0   # bias -> LayerNorm -> norm bias: the projection of an all-zero embedding is not zero


def test_refusals(sd, oracle, pairs):
    plain, ip, (x, t, c, y) = pairs("SD15_TINY")
    tok = np.zeros((1, 4, IP_DIM), np.float32)
    with pytest.raises(sd.EngineError, match="no IP-Adapter"):
        plain.unet_forward(x, t, c, y, ip_context=tok)
    with pytest.raises(sd.EngineError, match="no IP-Adapter"):
        plain.ip_adapter_project(np.zeros((1, CLIP_DIM), np.float32))
    with pytest.raises(sd.EngineError, match="ip_dim"):
        ip.unet_forward(x, t, c, y, ip_context=np.zeros((1, 4, IP_DIM + 8), np.float32))
    with pytest.raises(sd.EngineError, match="batch"):
        ip.unet_forward(np.repeat(x, 2, 0)[:3], np.repeat(t, 2)[:3], c, y, ip_context=np.zeros((2, 4, IP_DIM), np.float32))
    with pytest.raises(sd.EngineError, match="clip_dim"):
        ip.ip_adapter_project(np.zeros((1, CLIP_DIM + 1), np.float32))
    ip.ip_adapter_init(IP_DIM, CLIP_DIM, 4, weight_seed=99)   # the same dimensions again: nothing happens, the weights stay
    with pytest.raises(sd.EngineError, match="other dimensions"):
        ip.ip_adapter_init(IP_DIM * 2, CLIP_DIM, 4)
    dit = sd.Engine(model=sd.SD35_TINY, backend="CPU-oracle", flash_attn=True)
    with pytest.raises(sd.EngineError, match="UNet families"):
        dit.ip_adapter_init(IP_DIM, CLIP_DIM, 4)


# ---------------------------------------------------------------------------------------------------------------- kernel logic
@pytest.mark.parametrize("lk_ip", [1, 4, 16, 31, 32])
def test_ip_block_index_logic(lk_ip):
    """k_flash_short_ip's image block replayed lane by lane: which register holds which image score, what the accumulator's initial value masks, the two-half
    max / sum exchange, and that P's packing order meets V's rows in the P V k-steps — against the softmax written directly."""
    rng = np.random.default_rng(lk_ip)
    d = 16
    q = rng.standard_normal((32, d))
    k = rng.standard_normal((lk_ip, d))
    v = rng.standard_normal((lk_ip, d))
    kpad = np.zeros((32, d))
    kpad[:lk_ip] = k                                     # rows beyond Lk_ip are staged as zeros
    vpad = np.zeros((32, d))
    vpad[:lk_ip] = v
    st = kpad @ q.T                                      # S^T[key, query]
    owner = {}
    si = np.empty((64, 16))
    for lane in range(64):
        for r in range(16):
            key = IP.ip_key_of(lane, r)
            assert 0 <= key < 32
            owner.setdefault((lane & 31, key), []).append((lane, r))
            init = -np.inf if IP.ip_key_masked(lane, r, lk_ip) else 0.0
            assert IP.ip_key_masked(lane, r, lk_ip) == (key >= lk_ip)
            si[lane, r] = init + st[key, lane & 31]
    assert len(owner) == 32 * 32 and all(len(o) == 1 for o in owner.values())      # every (query, key) in exactly one register
    assert not IP.ip_key_masked(0, 0, lk_ip) and IP.ip_key_of(0, 0) == 0             # key 0: lane half 0, register 0, never masked
    m = si.max(1)
    m = np.maximum(m, m[np.arange(64) ^ 32])
    assert np.isfinite(m).all()                                                      # also for the half whose 16 keys are all masked (Lk_ip <= 4)
    p = np.exp2(si - m[:, None])
    ps = p.sum(1)
    ps = ps + ps[np.arange(64) ^ 32]
    assert (ps >= 1.0).all()
    p = p * (0.35 / ps)[:, None]
    out = np.zeros((32, d))
    for lane in range(64):
        hi = lane >> 5
        for r in range(16):
            t, j = IP.ip_pv_slot(lane, r)
            vrow = t * 16 + 4 * hi + (j & 3) + 8 * (j >> 2)                         # the V row element j of lane half hi's B fragment holds in k-step t
            assert vrow == IP.ip_key_of(lane, r)
            if t == 1 and lk_ip <= 16:
                assert p[lane, r] == 0.0                                            # the skipped second k-step carries no weight
                continue
            out[lane & 31] += p[lane, r] * vpad[vrow]
    s = q @ k.T
    w = np.exp2(s - s.max(1, keepdims=True))
    want = 0.35 * (w / w.sum(1, keepdims=True)) @ v
    np.testing.assert_allclose(out, want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("kind", AS.KINDS)
@pytest.mark.parametrize("ip_scale", [1.0, 0.35, -0.5, 2.0])
def test_plain_route_model_within_the_fused_bar(kind, ip_scale):
    """the bar the GPU test holds the fused launch to — max(2e-3, 3 s), s the fused rounding model's distance from float64 — also holds the plain-node route
    modelled the same way, on every data family and scale: the two routes are interchangeable at that bar"""
    rng = np.random.default_rng([AS.KINDS.index(kind), int(ip_scale * 100) + 100])
    d, Lq, Lk, Li, HN = 40, 33, 77, 16, 2
    q, k, v = AS.make_heads(kind, Lq, Lk, d, HN, rng)
    _, ki, vi = AS.make_heads(kind, Lq, Li, d, HN, rng)
    scale = 1.0 / np.sqrt(d)
    k16, v16, ki16, vi16 = (AS.f16r(a) for a in (k, v, ki, vi))
    ex = IP.exact(q, k16, v16, ki16, vi16, scale, ip_scale)
    s = AS.rel_l2(IP.fused_model(q, k16, v16, ki16, vi16, scale, ip_scale), ex)
    sp = AS.rel_l2(IP.plain_model(q, k16, v16, ki16, vi16, scale, ip_scale), ex)
    print(f"[ip-adapter] {kind} ip_scale={ip_scale}: fused model {s:.3e}, plain model {sp:.3e}")
    assert np.isfinite(s) and sp < max(2e-3, 3.0 * s)


# ---------------------------------------------------------------------------------------------------------------- composition, samplers
def test_attn2_composes_from_the_no_ip_pieces(sd, oracle):
    """numeric check of orientation and scale placement from the oracle's own no-IP forward: with to_k_ip = to_k, to_v_ip = to_v, the text context as the image
    tokens and ip_scale 1, every attn2 hands to_out x + 1 * x = 2 x (exact in f32); a context WITHOUT the adapter whose attn2 to_out weights are doubled (exact in
    f16) computes W (2 x) as (2 W) x: every product and partial sum doubles exactly, so the two forwards are bit-identical.  ip_scale 3 against weights times 4
    differs only by the rounding of 3 x: rel-L2 < 1e-5.  A transposed to_k_ip, tokens on the wrong projection or the scale on the wrong operand break both."""
    a, x, t, c, y = _inputs(sd, "SD15_TINY")
    b, *_ = _inputs(sd, "SD15_TINY")
    a.ip_adapter_init(c.shape[2], CLIP_DIM, 4)
    outs = [n for n in b.tensor_names() if n.endswith("attn2.to_out.0.weight")]
    for n in outs:
        p = n[:-len("to_out.0.weight")]
        a.set_tensor(p + "to_k_ip.weight", a.get_tensor(p + "to_k.weight"))
        a.set_tensor(p + "to_v_ip.weight", a.get_tensor(p + "to_v.weight"))
    base = {n: b.get_tensor(n) for n in outs}
    for n in outs:
        b.set_tensor(n, base[n] * 2.0)
    np.testing.assert_array_equal(a.unet_forward(x, t, c, y, ip_context=c, ip_scale=1.0), b.unet_forward(x, t, c, y))
    for n in outs:
        b.set_tensor(n, base[n] * 4.0)
    err = AS.rel_l2(a.unet_forward(x, t, c, y, ip_context=c, ip_scale=3.0), b.unet_forward(x, t, c, y))
    print(f"[ip-adapter] composition, ip_scale 3 vs to_out x 4: rel-L2 {err:.3e}")
    assert 0.0 < err < 1e-5 or err == 0.0


def _traj(sd, e, **over):
    rng = np.random.default_rng(5)
    cond, uncond = rng.standard_normal((1, 77, 64)).astype(np.float32), rng.standard_normal((1, 77, 64)).astype(np.float32)
    kw = dict(width=128, height=128, steps=2, cfg=5.0, seed=11, batch=2, method=sd.EULER)
    kw.update(over)
    return e.sample_latents(cond, uncond, **kw), cond, uncond, kw


def test_sampler_token_state(sd, oracle, pairs):
    """sd_set_ip_adapter through the host loop, its fused pair and the device-resident sampler (all three bit-equal on the oracle): the default uncond tokens ARE the
    projection of zeros (and not zeros); cond and uncond tokens swapped give another trajectory; strength 0 and cleared tokens give the trajectory of a context
    without the adapter; embeds = project + set"""
    plain, ip, _ = pairs("SD15_TINY")
    rng = np.random.default_rng(31)
    tok, un = (rng.standard_normal((4, IP_DIM)).astype(np.float32) for _ in range(2))
    zero_proj = ip.ip_adapter_project(np.zeros((1, CLIP_DIM), np.float32))[0]
    base, *_ = _traj(sd, plain)
    try:
        ip.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.7)
        a, *_ = _traj(sd, ip)
        np.testing.assert_array_equal(_traj(sd, ip, fuse_cfg=True)[0], a)
        np.testing.assert_array_equal(_traj(sd, ip, fuse_cfg=True, device_sampler=True)[0], a)
        assert AS.rel_l2(a, base) > 1e-3
        ip.set_ip_adapter(tokens=un, uncond_tokens=tok, strength=0.7)
        swapped, *_ = _traj(sd, ip)
        assert AS.rel_l2(swapped, a) > 1e-3
        ip.set_ip_adapter(tokens=tok, strength=0.7)
        dflt, *_ = _traj(sd, ip)
        ip.set_ip_adapter(tokens=tok, uncond_tokens=zero_proj, strength=0.7)
        np.testing.assert_array_equal(_traj(sd, ip)[0], dflt)
        ip.set_ip_adapter(tokens=tok, uncond_tokens=np.zeros_like(tok), strength=0.7)
        assert not np.array_equal(_traj(sd, ip)[0], dflt)
        emb = rng.standard_normal(CLIP_DIM).astype(np.float32)
        ip.set_ip_adapter(embeds=emb, strength=0.7)
        via_embeds, *_ = _traj(sd, ip)
        ip.set_ip_adapter(tokens=ip.ip_adapter_project(emb[None])[0], strength=0.7)
        np.testing.assert_array_equal(_traj(sd, ip)[0], via_embeds)
        ip.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.0)
        np.testing.assert_array_equal(_traj(sd, ip)[0], base)
        ip.set_ip_adapter()
        np.testing.assert_array_equal(_traj(sd, ip)[0], base)
        np.testing.assert_array_equal(_traj(sd, ip, fuse_cfg=True, device_sampler=True)[0], _traj(sd, plain, fuse_cfg=True, device_sampler=True)[0])
    finally:
        ip.set_ip_adapter()


def test_trajectory_equals_a_python_driven_loop(sd, oracle, pairs):
    """2 Euler steps with equal cond / uncond tokens and strength 0.6, bit for bit against a loop of unet_forward(ip_context=, ip_scale=) calls that restates the host
    loop's separately rounded f32 operations (CompVis scalings, guidance.cpp:171, denoiser.hpp:1582-1597) and the Philox start noise"""
    from test_host_logic import philox_randn_np

    _, ip, _ = pairs("SD15_TINY")
    tok = np.random.default_rng(41).standard_normal((4, IP_DIM)).astype(np.float32)
    f = np.float32
    try:
        ip.set_ip_adapter(tokens=tok, uncond_tokens=tok, strength=0.6)
        out, cond, uncond, kw = _traj(sd, ip, batch=1)
    finally:
        ip.set_ip_adapter()
    sig = sd.get_sigmas(kw["steps"])
    n = 4 * 16 * 16
    x = (philox_randn_np(kw["seed"], 0, n).astype(np.float32) * f(sig[0])).astype(np.float32).reshape(1, 4, 16, 16)
    for i in range(kw["steps"]):
        s, s_to = f(sig[i]), f(sig[i + 1])
        c_in = f(1.0) / np.sqrt(s * s + f(1.0), dtype=np.float32)
        t = np.array([sd.lib().sd_sigma_to_t(float(s))], dtype=np.float32)
        xin = (x * c_in).astype(np.float32)
        ec = ip.unet_forward(xin, t, cond, ip_context=tok[None], ip_scale=0.6)
        eu = ip.unet_forward(xin, t, uncond, ip_context=tok[None], ip_scale=0.6)
        g = eu + f(kw["cfg"]) * (ec - eu)
        den = g * (-s) + x * f(1.0)
        d = (x - den) / s
        x = x + d * (s_to - s)
    assert x.dtype == np.float32
    np.testing.assert_array_equal(out, x)


def test_sampler_refusals(sd, oracle, pairs):
    plain, ip, _ = pairs("SD15_TINY")
    tok = np.zeros((4, IP_DIM), np.float32)
    with pytest.raises(sd.EngineError, match="no IP-Adapter"):          # set before init
        plain.set_ip_adapter(tokens=tok)
    with pytest.raises(sd.EngineError, match="no IP-Adapter"):
        plain.set_ip_adapter(embeds=np.zeros(CLIP_DIM, np.float32))
    with pytest.raises(sd.EngineError, match="n_tokens mismatch"):      # the two token sets differ in count
        ip.set_ip_adapter(tokens=tok, uncond_tokens=np.zeros((16, IP_DIM), np.float32))
    with pytest.raises(sd.EngineError, match="ip_dim"):
        ip.set_ip_adapter(tokens=np.zeros((4, IP_DIM + 8), np.float32))
    with pytest.raises(sd.EngineError, match="uncond_tokens must be given"):   # 16 cond tokens, but the projection of zeros has 4
        ip.set_ip_adapter(tokens=np.zeros((16, IP_DIM), np.float32))
    with pytest.raises(sd.EngineError, match="clip_dim"):
        ip.set_ip_adapter(embeds=np.zeros(CLIP_DIM + 1, np.float32))
    plain.set_ip_adapter()                                               # clearing needs no adapter
