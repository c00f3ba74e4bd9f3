"""Inpaint / pix2pix UNets on the MI355X: the two glue kernels of the device-resident sampler (kernels/guidance.hip) through sd_guidance_kernels and as planner
patterns, bit for bit against the NumPy restatement (tests/concat_cfg_ref.py) and against the plain nodes; the forward with c_concat against the oracle backend;
trajectories with the fusions on and off, replayed, against the oracle backend, with a step cache, and next to a plain context.

Bars.  The kernels copy, multiply once, or evaluate six separately rounded operations: bit for bit.  One forward: rel-L2 < 5e-3, the per-forward bar of
tests/test_gpu_model.py.  A three-step trajectory: 3 x 5e-3 — the per-forward error enters each Euler update once, so it adds at most linearly over the steps.
Measured on the MI355X: forwards 1.2e-3 .. 1.5e-3 (the first conv with K = 81 / 72 runs on g16_conv_t128n64 at these widths), trajectories 4.1e-3 (K = 2) and
3.9e-3 (K = 3).
The counter assertions are skipped under SDCPP_BACKEND_OPTS and with SDCPP_GPU_TESTS_ON_ORACLE=1."""
import os

import numpy as np
import pytest

import concat_cfg_ref as ref
from ggml_graph import F16, F32, Graph, tensor_struct

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"


def _counting():
    return ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def engines(sd, gpu, oracle):
    made = {}

    def get(name, variant, backend=None):
        key = (name, variant, backend or gpu)
        if key not in made:
            made[key] = sd.Engine(model=getattr(sd, name), backend=key[2], variant=variant)
        return made[key]

    return get


def _find_contraction_pair():
    """scale pairs on which a contracted multiply-add changes the last bit of some element: found by search, and asserted, so the case cannot go vacuous"""
    c, u, iu = ref.special_vectors(1027 * 3, seed=23)
    found = []
    for txt, img in ((7.5, 1.5), (1.0, 1.5), (3.3, 0.7), (11.0, 2.25), (5.1, 1.9)):
        if not ref.same_bits(ref.cfg_combine3_contracted(c, u, iu, txt, img), ref.cfg_combine3(c, u, iu, txt, img)):
            found.append((txt, img))
    return c, u, iu, found


G3_C, G3_U, G3_IU, G3_PAIRS = _find_contraction_pair()
assert len(G3_PAIRS) >= 2, "no scale pair shows a contracted multiply-add on this data"


# ---------------------------------------------------------------------------------------------------------------- k_model_input
@pytest.mark.parametrize("w,h,c,cc,route", [(8, 8, 4, 5, "v4"), (5, 3, 4, 5, "v1"), (6, 2, 4, 4, "v4"), (2, 2, 4, 5, "v4"), (1, 1, 4, 5, "v1")])
def test_model_input_kernel(sd, engines, w, h, c, cc, route):
    e = engines("SD15_TINY", sd.UNET_PLAIN)   # (the entry needs a context for its backend only)
    rng = np.random.default_rng(w * 100 + h)
    for k in (1, 2, 3):
        for nb in (1, 3):
            for per_image in (False, True):
                for c_in in (1.0, 0.37):
                    x = rng.standard_normal((nb, c, h, w)).astype(np.float32)
                    cat = rng.standard_normal((k * nb if per_image else k, cc, h, w)).astype(np.float32)
                    s0 = sd.backend_stats() if _counting() else None
                    xin, _ = e.guidance_kernels(x=x, c_in=c_in, concat=cat, k=k, concat_per_image=per_image)   # (the output buffer starts as NaN)
                    assert ref.same_bits(xin, ref.model_input(x, c_in, cat, k, per_image)), (k, nb, per_image, c_in)
                    if s0 is not None:
                        s1 = sd.backend_stats()
                        moved = {f: s1[f] - s0[f] for f in ("fused_model_input", "ew_model_input_v4", "ew_model_input_v1") if s1[f] != s0[f]}
                        assert moved == {"fused_model_input": 1, "ew_model_input_" + route: 1}, (k, nb, per_image, c_in, moved)


# ---------------------------------------------------------------------------------------------------------------- k_guidance3
@pytest.mark.parametrize("per", [1, 60, 256, 1027])
def test_guidance3_kernel(sd, engines, per):
    e = engines("SD15_TINY", sd.UNET_PLAIN)
    for nb in (1, 3):
        n = per * nb
        e3 = np.stack([G3_C[:n].reshape(nb, per), G3_U[:n].reshape(nb, per), G3_IU[:n].reshape(nb, per)], axis=1)   # [nb, 3, per]
        for txt, img in G3_PAIRS + [(7.0, 1.0), (3.0, 3.0)]:
            s0 = sd.backend_stats() if _counting() else None
            _, got = e.guidance_kernels(e3=e3, txt_cfg=txt, img_cfg=img)
            want = ref.cfg_combine3(e3[:, 0], e3[:, 1], e3[:, 2], txt, img)
            assert ref.same_bits(got, want), (per, nb, txt, img)
            assert ref.same_bits(got, sd.cfg_combine3(e3[:, 0], e3[:, 1], e3[:, 2], txt, img))
            if s0 is not None:
                assert sd.backend_stats()["fused_guidance3"] - s0["fused_guidance3"] == 1


# ---------------------------------------------------------------------------------------------------------------- planner patterns
def _model_input_graph(g, L, x, c_in, cat, k, *, rep_reader=False, mul_reader=False, concat_output=False, f16_cat=False):
    """the sampler's chain on caller tensors; the CONCAT feeds a DUP so that it is no graph output unless asked"""
    nb, c, h, w = x.shape
    per = c * h * w
    tx, ts, tc = g.input(x), g.input(np.array([c_in], np.float32)), g.input(cat)
    noised = L.ggml_mul(g.ctx, tx, ts)
    xk, rep = noised, None
    if k > 1:
        flat = L.ggml_reshape_3d(g.ctx, noised, per, 1, nb)
        rep = L.ggml_repeat(g.ctx, flat, L.ggml_new_tensor_3d(g.ctx, F32, per, k, nb))
        xk = L.ggml_reshape_4d(g.ctx, rep, w, h, c, k * nb)
    cc_all = tc
    if cat.shape[0] != k * nb:
        cc_all = L.ggml_repeat(g.ctx, tc, L.ggml_new_tensor_4d(g.ctx, F32, w, h, cat.shape[1], k * nb))
    node = L.ggml_concat(g.ctx, xk, cc_all, 2)
    if f16_cat:
        tensor_struct(node).src[1] = g.input(np.broadcast_to(cat, (k * nb,) + cat.shape[1:]).copy(), F16)
        return node
    outs = [node if concat_output else L.ggml_dup(g.ctx, node)]
    if rep_reader:
        outs.append(L.ggml_dup(g.ctx, rep))
    if mul_reader:
        outs.append(L.ggml_dup(g.ctx, noised))
    return outs


def _run_model_input(sd, gpu, option, **kw):
    rng = np.random.default_rng(77)
    x = rng.standard_normal((3, 4, 6, 8)).astype(np.float32)
    cat = rng.standard_normal((2, 5, 6, 8)).astype(np.float32)
    if ON_GPU:
        sd.backend_set_option("fuse_model_input", option)
    try:
        s0 = sd.backend_stats() if _counting() else None
        with Graph(gpu) as g:
            outs = g.run(*_model_input_graph(g, sd.lib(), x, 0.37, cat, 2, **kw))
        fused = sd.backend_stats()["fused_model_input"] - s0["fused_model_input"] if s0 is not None else None
    finally:
        if ON_GPU:
            sd.backend_set_option("fuse_model_input", 1)
    outs = outs if isinstance(outs, list) else [outs]
    want = ref.model_input(x, 0.37, cat, 2, False)
    assert ref.same_bits(outs[0], want)
    return outs, fused, x


def test_model_input_pattern_on_off_and_refusals(sd, gpu):
    on, fused_on, _ = _run_model_input(sd, gpu, 1)
    off, fused_off, _ = _run_model_input(sd, gpu, 0)
    assert ref.same_bits(on[0], off[0])
    if fused_on is not None:
        assert (fused_on, fused_off) == (1, 0)
    # an extra reader of the REPEAT: the intermediate must exist — plain nodes, right results
    outs, fused, x = _run_model_input(sd, gpu, 1, rep_reader=True)
    assert fused in (None, 0)
    assert ref.same_bits(outs[1].reshape(3, 2, -1), np.repeat((x * np.float32(0.37)).reshape(3, 1, -1), 2, axis=1))
    # the CONCAT flagged as a graph output
    outs, fused, _ = _run_model_input(sd, gpu, 1, concat_output=True)
    assert fused in (None, 0)
    # the MUL with a second reader is still written; the rest of the chain fuses behind it (the recording variant of the step cache)
    outs, fused, x = _run_model_input(sd, gpu, 1, mul_reader=True)
    assert fused in (None, 1)
    assert ref.same_bits(outs[1], x * np.float32(0.37))


@pytest.mark.skipif(not ON_GPU, reason="planner_supports_op is the product backend's predicate")
def test_model_input_pattern_refuses_an_f16_concat_operand(sd, gpu):
    """the backend's concat kernels read both sources as f32, and so does k_model_input: a foreign graph with an f16 second source is refused at supports_op, the
    pattern never sees it (the counter stays put because nothing is planned)"""
    rng = np.random.default_rng(78)
    x = rng.standard_normal((1, 4, 4, 4)).astype(np.float32)
    cat = rng.standard_normal((2, 5, 4, 4)).astype(np.float32)
    s0 = sd.backend_stats()
    with Graph(gpu) as g:
        node = _model_input_graph(g, sd.lib(), x, 0.5, cat, 2, f16_cat=True)
        assert not g.supports(node)
    assert sd.backend_stats()["fused_model_input"] == s0["fused_model_input"]


def test_guidance3_pattern_on_off_and_refusal(sd, gpu):
    per, nb = 60, 3
    n = per * nb
    e3 = np.stack([G3_C[:n].reshape(nb, per), G3_U[:n].reshape(nb, per), G3_IU[:n].reshape(nb, per)], axis=1)
    txt, img = G3_PAIRS[0]
    res = {}
    for label, option, reader in (("on", 1, False), ("off", 0, False), ("reader", 1, True)):
        if ON_GPU:
            sd.backend_set_option("fuse_guidance3", option)
        try:
            s0 = sd.backend_stats() if _counting() else None
            with Graph(gpu) as g:
                L = sd.lib()
                t3, ts = g.input(e3), g.input(np.array([0.0, txt, 0, 0, 0, 0, 0, 1, img], np.float32))
                S = lambda j: L.ggml_view_1d(g.ctx, ts, 1, 4 * j)
                row = lambda j: L.ggml_view_3d(g.ctx, t3, per, 1, nb, 4 * per, 12 * per, 4 * per * j)
                ec, eu, ei = row(0), row(1), row(2)
                a1 = L.ggml_add(g.ctx, ei, L.ggml_mul(g.ctx, L.ggml_sub(g.ctx, eu, ei), S(8)))
                out = L.ggml_add(g.ctx, a1, L.ggml_mul(g.ctx, L.ggml_sub(g.ctx, ec, eu), S(1)))
                outs = g.run(out, L.ggml_dup(g.ctx, a1)) if reader else [g.run(out)]
            res[label] = (outs, sd.backend_stats()["fused_guidance3"] - s0["fused_guidance3"] if s0 is not None else None)
        finally:
            if ON_GPU:
                sd.backend_set_option("fuse_guidance3", 1)
    want = ref.cfg_combine3(e3[:, 0], e3[:, 1], e3[:, 2], txt, img)
    for label in res:
        assert ref.same_bits(res[label][0][0].reshape(nb, per), want), label
    if res["on"][1] is not None:
        assert (res["on"][1], res["off"][1], res["reader"][1]) == (1, 0, 0)
    a1_want = e3[:, 2] + np.float32(img) * (e3[:, 1] - e3[:, 2])
    assert ref.same_bits(res["reader"][0][1].reshape(nb, per), a1_want)


# ---------------------------------------------------------------------------------------------------------------- forward parity
@pytest.mark.parametrize("name,variant", [("SD15_TINY", 1), ("SD15_TINY", 2), ("SDXL_TINY", 1)])
def test_forward_with_concat_vs_oracle(sd, engines, oracle, name, variant):
    e, o = engines(name, variant), engines(name, variant, oracle)
    cc = e.concat_channels()
    rng = np.random.default_rng(12)
    ctx = rng.standard_normal((1, 77, 64)).astype(np.float32)
    y = rng.standard_normal((1, 96)).astype(np.float32) if "XL" in name else None
    for n, s in ((2, 32), (3, 8)):   # 8 x 8 latents: 1 x 1 feature maps at the deepest level
        x = rng.standard_normal((n, 4, s, s)).astype(np.float32)
        cat = rng.standard_normal((1, cc, s, s)).astype(np.float32)
        t = np.linspace(900.0, 30.0, n).astype(np.float32)
        s0 = sd.backend_stats() if _counting() else None
        a = e.unet_forward(x, t, ctx, y, c_concat=cat)
        if s0 is not None:   # the first conv runs with K = 81 / 72 for the first time: which conv route took it
            s1 = sd.backend_stats()
            print(name, variant, (n, s), "conv routes moved:", {k: s1[k] - s0[k] for k in s1 if (k.startswith("g16_conv_") or k.startswith("c3w_")) and s1[k] != s0[k]})
        err = rel_l2(a, o.unet_forward(x, t, ctx, y, c_concat=cat))
        print(f"{name} variant {variant} n={n} {s}x{s}: rel-L2 vs oracle {err:.3e}")
        assert np.isfinite(a).all() and err < 5e-3
        np.testing.assert_array_equal(e.unet_forward(x, t, ctx, y, c_concat=cat), a)   # the cached plan


# ---------------------------------------------------------------------------------------------------------------- trajectories
def _cond(seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((1, 77, 64)).astype(np.float32), rng.standard_normal((1, 77, 64)).astype(np.float32)


def _traj(sd, e, k, **over):
    cond, uncond = _cond()
    e.set_img_cfg(1.5 if k == 3 else float("inf"))
    kw = dict(width=128, height=128, steps=3, cfg=7.5, seed=11, batch=2, method=sd.EULER_A, device_sampler=True, fuse_cfg=True)
    kw.update(over)
    return e.sample_latents(cond, uncond, **kw)


def _concat(n=1):
    rng = np.random.default_rng(60 + n)
    cat = rng.standard_normal((n, 5, 16, 16)).astype(np.float32)
    cat[:, 0] = cat[:, 0] > 0
    return cat


@pytest.mark.parametrize("k", [2, 3])
def test_trajectory_fusions_on_off_replay_and_oracle(sd, engines, oracle, k):
    e, o = engines("SD15_TINY", sd.UNET_INPAINT), engines("SD15_TINY", sd.UNET_INPAINT, oracle)
    cat = _concat()
    try:
        e.set_concat_condition(cat)
        o.set_concat_condition(cat)
        s0 = sd.backend_stats() if _counting() else None
        on = _traj(sd, e, k)
        if s0 is not None:
            s1 = sd.backend_stats()
            moved = {f: s1[f] - s0[f] for f in ("fused_model_input", "fused_guidance3", "ew_model_input_v4")}
            print(f"K = {k}: {moved}")
            assert moved["fused_model_input"] >= 1 and moved["ew_model_input_v4"] >= 1 and (moved["fused_guidance3"] >= 1) == (k == 3)
        np.testing.assert_array_equal(_traj(sd, e, k), on)   # the second trajectory replays the captured graph
        if ON_GPU:
            sd.backend_set_option("fuse_model_input", 0)
            sd.backend_set_option("fuse_guidance3", 0)
        try:
            off = _traj(sd, e, k)
        finally:
            if ON_GPU:
                sd.backend_set_option("fuse_model_input", 1)
                sd.backend_set_option("fuse_guidance3", 1)
        np.testing.assert_array_equal(off, on)
        err = rel_l2(on, _traj(sd, o, k))
        print(f"K = {k}: 3-step Euler-A trajectory, MI355X vs oracle rel-L2 {err:.3e} (bar {3 * 5e-3:.1e})")
        assert np.isfinite(on).all() and err < 3 * 5e-3
    finally:
        for x in (e, o):
            x.set_concat_condition(None)
            x.set_img_cfg()


def test_two_branch_concat_trajectory_with_ucache(sd, engines):
    """decides like the host loop, the idiom of tests/test_gpu_step_cache.py::test_device_sampler_decides_like_the_host_loop"""
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    over = dict(steps=16, batch=1, method=sd.EULER, width=64, height=64)
    cat = _concat()[:, :, :8, :8].copy()
    decisions = lambda tr: [(r["step"], r["active"], r["skipped"]) for r in tr]
    try:
        e.set_concat_condition(cat)
        e.set_step_cache(sd.CACHE_UCACHE, reuse_threshold=0.0)
        _traj(sd, e, 2, device_sampler=False, fuse_cfg=False, **over)
        rates = [r["rate"] for r in e.step_cache_trace() if r["rate"] > 0]
        assert len(rates) >= 4
        e.set_step_cache(sd.CACHE_UCACHE, reuse_threshold=float(1.5 * np.median(rates)))
        host = _traj(sd, e, 2, device_sampler=False, fuse_cfg=False, **over)
        t_host = e.step_cache_trace()
        decided = [r for r in t_host if r["threshold"] > 0]
        assert sum(r["skipped"] for r in t_host) > 0 and len(decided) >= 4
        for r in decided:
            assert abs(r["accumulated"] - r["threshold"]) > 1e-3 * r["threshold"], f"step {r['step']} decides within 1e-3 of its threshold: choose another seed"
        dev = _traj(sd, e, 2, **over)
        assert decisions(e.step_cache_trace()) == decisions(t_host)
        print(f"UCache with c_concat: {sum(r['skipped'] for r in t_host)} steps skipped, device vs host max |diff| {float(np.abs(dev - host).max()):.3e}")
        assert np.isfinite(dev).all()
    finally:
        e.set_step_cache(None)
        e.set_concat_condition(None)
        e.set_img_cfg()


def test_plain_context_is_untouched_by_a_variant_trajectory(sd, engines):
    plain, inp = engines("SD15_TINY", sd.UNET_PLAIN), engines("SD15_TINY", sd.UNET_INPAINT)
    before = _traj(sd, plain, 2)
    try:
        inp.set_concat_condition(_concat(2))
        assert np.isfinite(_traj(sd, inp, 3)).all()
    finally:
        inp.set_concat_condition(None)
        inp.set_img_cfg()
    np.testing.assert_array_equal(_traj(sd, plain, 2), before)
