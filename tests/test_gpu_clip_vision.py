"""GPU suite: k_clip_preprocess, k_patch_embed and its planner pattern, the GELU_ERF unary, the CLIP vision tower, the Resampler, and image tokens from a picture end to
end (csrc/kernels/clip_vision.hip, csrc/backend/planner.cpp plan_patch_embed, csrc/host/clip_vision.hpp).  References: tests/clip_vision_ref.py."""
import os

import numpy as np
import pytest

import clip_vision_ref as CV
from ggml_graph import F16, F32, Graph

pytestmark = pytest.mark.gpu

ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"  # harness self-check mode: the 'gpu' fixture is the CPU oracle (no kernels, no counters, no GELU_ERF)
needs_kernels = pytest.mark.skipif(not ON_GPU, reason="self-check mode on the CPU oracle: the MI355X kernels and counters do not exist there")


def _stats(sd):
    return sd.backend_stats() if ON_GPU else None


def _delta(sd, s0, key):
    return sd.backend_stats()[key] - s0[key]


# ---------------------------------------------------------------------------------------------------- k_clip_preprocess
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("w,h,S", [(37, 23, 28), (23, 37, 28), (224, 224, 224), (640, 480, 224), (1, 1, 28)])
def test_clip_preprocess_kernel_bit_for_bit(sd, gpu, w, h, S, n):
    img = np.random.default_rng(w * 7 + h + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    img[0, 0, 0] = (0, 255, 128)
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    got = e.clip_preprocess(img, size=S)
    ref = CV.clip_preprocess(img, S)
    assert got.shape == ref.shape == (n, 3, S, S)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"max abs diff {np.abs(got - ref).max()}"


# ---------------------------------------------------------------------------------------------------- k_patch_embed
def _embed_graph(g, L, px, w, cls, pos, P, stride=None, bias=None, second_reader=False):
    """CLIPVisionEmbeddings::forward (clip.hpp:224-235) through the C ggml API; returns the output nodes"""
    N, _, S, _ = px.shape
    E = w.shape[0]
    s = stride or P
    x = g.input(px)
    wt = g.weight(w, F16)
    conv = L.ggml_conv_2d(g.ctx, wt, x, s, s, 0, 0, 1, 1)
    if bias is not None:
        conv = L.ggml_add_inplace(g.ctx, conv, L.ggml_reshape_4d(g.ctx, g.weight(bias, F32), 1, 1, E, 1))
    G = (S - P) // s + 1
    np_ = G * G
    pe = L.ggml_reshape_3d(g.ctx, conv, np_, E, N)
    pe = L.ggml_cont(g.ctx, L.ggml_permute(g.ctx, pe, 1, 0, 2, 3))
    pe = L.ggml_reshape_4d(g.ctx, pe, 1, E, np_, N)
    c = L.ggml_repeat(g.ctx, g.weight(cls, F32), L.ggml_new_tensor_2d(g.ctx, F32, E, N))
    c = L.ggml_reshape_4d(g.ctx, c, 1, E, 1, N)
    y = L.ggml_concat(g.ctx, c, pe, 2)
    y = L.ggml_reshape_3d(g.ctx, y, E, np_ + 1, N)
    y = L.ggml_add(g.ctx, y, g.weight(pos, F32))
    outs = [y]
    if second_reader:
        outs.append(L.ggml_scale(g.ctx, conv, 2.0))
    return outs


def _embed_data(seed, N, S, P, E, tail_only=False):
    rng = np.random.default_rng(seed)
    px = rng.integers(-2, 3, (N, 3, S, S)).astype(np.float32)
    w = rng.integers(-1, 2, (E, 3, P, P)).astype(np.float32)
    if tail_only:  # weights and pixels nonzero only in the last 12 of the K = 3 P P entries (c = 2, ky = P - 1, kx >= P - 12): a dropped or mis-padded K tail shows
        wm = np.zeros_like(w)
        wm[:, 2, P - 1, P - 12:] = rng.integers(1, 2, (E, 12)) * rng.choice([-1, 1], (E, 12))
        w = wm
        pm = np.zeros_like(px)
        G = S // P
        for gy in range(G):
            for gx in range(G):
                v = px[:, 2, gy * P + P - 1, gx * P + P - 12: gx * P + P]
                pm[:, 2, gy * P + P - 1, gx * P + P - 12: gx * P + P] = np.where(v == 0, 1.0, v)
        px = pm
    cls = rng.integers(-3, 4, (E,)).astype(np.float32)
    pos = rng.integers(-4, 5, ((S // P) ** 2 + 1, E)).astype(np.float32)
    return px, w, cls, pos


EMBED_CASES = [
    ("smallest", 1, 28, 14, 64, False),
    ("embed_80", 2, 28, 14, 80, False),          # embed no multiple of the 64-column tile
    ("full_patch_count_n1", 1, 224, 14, 128, False),
    ("full_patch_count_n3", 3, 224, 14, 128, False),  # 768 patch rows: 12 row tiles, images straddle none; class rows of 3 images
    ("k12", 2, 12, 2, 96, False),                # K = 12, under one MFMA K step; 36 patches
    ("k_tail", 2, 42, 14, 72, True),             # only the last 12 of 588 K entries carry data; 9 patches per image (a partial row tile)
]


@needs_kernels
@pytest.mark.parametrize("name,N,S,P,E,tail", EMBED_CASES, ids=[c[0] for c in EMBED_CASES])
def test_patch_embed_kernel_bit_for_bit(sd, gpu, name, N, S, P, E, tail):
    px, w, cls, pos = _embed_data(len(name) * 31 + E, N, S, P, E, tail)
    ref = CV.patch_embed(px, w, cls, pos, P)
    assert np.abs(ref).max() < 2 ** 20  # integers: exact in f16 x f16 -> f32
    if tail:
        assert np.abs(ref[:, 1:] - pos[1:]).max() > 0
    outs = {}
    for fuse in (1, 0):
        sd.backend_set_option("fuse_patch_embed", fuse)
        try:
            s0 = sd.backend_stats()
            with Graph(gpu) as g:
                outs[fuse] = g.run(*_embed_graph(g, sd.lib(), px, w, cls, pos, P))
            assert _delta(sd, s0, "fused_patch_embed") == fuse and _delta(sd, s0, "patch_embed_launches") == fuse
        finally:
            sd.backend_set_option("fuse_patch_embed", 0)  # the default
    outs = {k: v.reshape(v.shape[-3:]) for k, v in outs.items()}  # (Graph.fetch returns all four ggml dimensions)
    assert outs[1].shape == ref.shape
    assert np.array_equal(outs[1], ref.astype(np.float32)), f"{name}: fused vs NumPy, {np.count_nonzero(outs[1] != ref)} cells differ"
    assert np.array_equal(outs[0], outs[1]), f"{name}: fused vs plain nodes"


@needs_kernels
@pytest.mark.parametrize("miss", ["stride", "bias", "second_reader"])
def test_patch_embed_nearest_misses_run_as_plain_nodes(sd, gpu, oracle, miss):
    N, S, P, E = 2, 28, 14, 64
    stride = 7 if miss == "stride" else None
    G = (S - P) // (stride or P) + 1
    rng = np.random.default_rng(5)
    px = rng.integers(-2, 3, (N, 3, S, S)).astype(np.float32)
    w = rng.integers(-1, 2, (E, 3, P, P)).astype(np.float32)
    cls = rng.integers(-3, 4, (E,)).astype(np.float32)
    pos = rng.integers(-4, 5, (G * G + 1, E)).astype(np.float32)
    bias = rng.integers(-2, 3, (E,)).astype(np.float32) if miss == "bias" else None
    kw = dict(stride=stride, bias=bias, second_reader=miss == "second_reader")
    sd.backend_set_option("fuse_patch_embed", 1)  # (the default is 0: the misses are misses of the pattern, not of the option)
    try:
        s0 = sd.backend_stats()
        with Graph(gpu) as g:
            got = g.run(*_embed_graph(g, sd.lib(), px, w, cls, pos, P, **kw))
        assert _delta(sd, s0, "fused_patch_embed") == 0 and _delta(sd, s0, "patch_embed_launches") == 0
        if miss == "bias":  # the same graph without the bias does match: the option is on
            with Graph(gpu) as g:
                g.run(*_embed_graph(g, sd.lib(), px, w, cls, pos, P))
            assert _delta(sd, s0, "fused_patch_embed") == 1
    finally:
        sd.backend_set_option("fuse_patch_embed", 0)
    with Graph(oracle) as g:
        ref = g.run(*_embed_graph(g, sd.lib(), px, w, cls, pos, P, **kw))
    got, ref = (got, ref) if isinstance(got, list) else ([got], [ref])
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)  # integer data: exact on both backends


# ---------------------------------------------------------------------------------------------------- GELU_ERF
def _unary_grid():
    return np.concatenate([np.linspace(-8, 8, 4001), [0.0, 1e-6, -1e-6, 1e-3, -1e-3, 6.0, -6.0, 40.0, -40.0]]).astype(np.float32)


def _floor_rel(out, ref):
    """max over the grid of |out - ref| / max(1, |ref|): f32 results carry a relative rounding error above 1 and an absolute one below"""
    ref = np.asarray(ref, np.float64)
    return float((np.abs(np.asarray(out, np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


@needs_kernels
def test_gelu_erf_unary_against_torch_erf(sd, gpu):
    """GELU_ERF (out of place and in place) against 0.5 x (1 + erf(x / sqrt 2)) in float64 on a grid with 0, +-1e-6, +-1e-3, +-6, +-40 and 4001 points of [-8, 8].
    Bound: twice the error of the existing GELU (tanh) route against its own float64 formula on the same grid, same metric (|err| / max(1, |ref|)).
    Measured on MI355X: GELU_ERF 1.224e-07 (in place the same bits), GELU (tanh) 2.918e-07, so the bound is 5.836e-07."""
    x = _unary_grid()
    L = sd.lib()
    with Graph(gpu) as g:
        tanh_out = g.run(L.ggml_gelu(g.ctx, g.input(x))).ravel()
    with Graph(gpu) as g:
        erf_out = g.run(L.ggml_gelu_erf(g.ctx, g.input(x))).ravel()
    with Graph(gpu) as g:
        erf_in = g.run(L.ggml_gelu_erf_inplace(g.ctx, L.ggml_scale(g.ctx, g.input(x), 1.0))).ravel()
    e_tanh = _floor_rel(tanh_out, CV.gelu_tanh(x))
    e_erf = _floor_rel(erf_out, CV.gelu_erf(x))
    e_in = _floor_rel(erf_in, CV.gelu_erf(x))
    print(f"[gelu_erf] error vs fp64: GELU_ERF {e_erf:.3e}, in place {e_in:.3e}; GELU (tanh) vs its own formula {e_tanh:.3e}; bound {2 * e_tanh:.3e}")
    assert np.isfinite(erf_out).all() and erf_out[x == 0][0] == 0 and erf_out[x == 40][0] == 40 and erf_out[x == -40][0] == 0
    assert np.array_equal(erf_in, erf_out)
    assert e_erf <= 2 * e_tanh and e_in <= 2 * e_tanh


# ---------------------------------------------------------------------------------------------------- tower
TOWERS = [("d64", 128, 2, 2, 28), ("d80", 160, 2, 2, 28), ("keys257", 128, 2, 1, 224)]  # keys257: the hidden-state leg uses clip_skip 1, so its one layer (257 keys) runs


@pytest.mark.parametrize("name,hidden,heads,layers,size", TOWERS, ids=[t[0] for t in TOWERS])
@pytest.mark.parametrize("N", [1, 2])
def test_tower_against_torch_float64(sd, gpu, name, hidden, heads, layers, size, N):
    """Pooled output and hidden state at clip_skip 2 against PyTorch float64 on the engine's own parameters.  Tolerance: the error of the same graph with fusion = 0 against
    the same reference, times 1.5 (the fused kernels change the summation order, not the operand formats); both printed."""
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    e.clip_vision_init(hidden=hidden, heads=heads, layers=layers, image_size=size, patch_size=14, proj=48, weight_seed=5)
    info = e.clip_vision_info()
    img = np.random.default_rng(hidden + N).integers(0, 256, (N, 50, 41, 3), dtype=np.uint8)
    px = e.clip_preprocess(img)
    for pooled, skip in ((True, -1), (False, 2 if layers > 1 else 1)):
        ref = CV.tower(e, px, pooled, skip)
        if ON_GPU:
            sd.backend_set_option("fuse_patch_embed", 1)  # (default 0, profiles/clip_vision_probe.txt: the tower is checked with the kernel in it)
        s0 = _stats(sd)
        try:
            got = e.clip_vision_encode(px, pooled, skip)
        finally:
            if ON_GPU:
                sd.backend_set_option("fuse_patch_embed", 0)
        if ON_GPU:
            run = CV.layers_run(layers, skip)
            assert _delta(sd, s0, "fused_patch_embed") == 1
            assert _delta(sd, s0, "fused_gelu") == (run if info["use_gelu"] else 0)
            sd.backend_set_option("fusion", 0)
        try:
            plain = e.clip_vision_encode(px, pooled, skip)
        finally:
            if ON_GPU:
                sd.backend_set_option("fusion", 1)
        err, err_plain = CV.rel_l2(got, ref), CV.rel_l2(plain, ref)
        print(f"[tower {name} N {N} pooled {pooled} clip_skip {skip}] rel-L2 vs torch fp64: fused {err:.3e}, fusion = 0 {err_plain:.3e}, bound {1.5 * err_plain:.3e}")
        assert got.shape == ref.shape and np.isfinite(got).all()
        assert err <= 1.5 * err_plain


@needs_kernels
def test_tower_gelu_epilogue_still_fuses(sd, gpu):
    """hidden 1024 is the width at which the reference's rule picks tanh-GELU (clip.hpp:21-25): fc1 -> GELU -> fc2 must still take the GEMM's GELU epilogue,
    one per layer run (1 layer, image 28: 5 tokens)"""
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    e.clip_vision_init(hidden=1024, heads=16, layers=1, image_size=28, patch_size=14, proj=32, weight_seed=2)
    assert e.clip_vision_info()["use_gelu"] == 1
    px = np.random.default_rng(1).standard_normal((1, 3, 28, 28)).astype(np.float32)
    s0 = sd.backend_stats()
    got = e.clip_vision_encode(px, True, -1)
    assert _delta(sd, s0, "fused_gelu") == 1
    ref = CV.tower(e, px, True, -1)
    sd.backend_set_option("fusion", 0)
    try:
        plain = e.clip_vision_encode(px, True, -1)
    finally:
        sd.backend_set_option("fusion", 1)
    err, err_plain = CV.rel_l2(got, ref), CV.rel_l2(plain, ref)
    print(f"[tower hidden 1024] rel-L2 vs torch fp64: fused {err:.3e}, fusion = 0 {err_plain:.3e}")
    assert err <= 1.5 * err_plain


# ---------------------------------------------------------------------------------------------------- Resampler
@needs_kernels
@pytest.mark.parametrize("n_tok", [5, 257])
@pytest.mark.parametrize("N", [1, 2])
def test_resampler_against_torch_float64(sd, gpu, n_tok, N):
    """dim 128, depth 2, 16 queries, embed_dim 160, output_dim 64, ff_inner 256; 5 tokens and 257 (273 keys against 16 queries).  Tolerance as for the tower."""
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    e.ip_adapter_init_plus(64, 128, 2, 16, 160, 256, 9)
    emb = np.random.default_rng(n_tok + N).standard_normal((N, n_tok, 160)).astype(np.float32)
    ref = CV.resampler(e, emb, 2)
    got = e.ip_adapter_project(emb)
    sd.backend_set_option("fusion", 0)
    try:
        plain = e.ip_adapter_project(emb)
    finally:
        sd.backend_set_option("fusion", 1)
    err, err_plain = CV.rel_l2(got, ref), CV.rel_l2(plain, ref)
    print(f"[resampler n_tok {n_tok} N {N}] rel-L2 vs torch fp64: fused {err:.3e}, fusion = 0 {err_plain:.3e}, bound {1.5 * err_plain:.3e}")
    assert got.shape == ref.shape == (N, 16, 64) and np.isfinite(got).all()
    assert err <= 1.5 * err_plain
    # all-zero hidden states: what set_ip_adapter(image=...) installs as uncond tokens, against the float64 Resampler under the same rule
    zero = np.zeros_like(emb)
    zref = CV.resampler(e, zero, 2)
    zgot = e.ip_adapter_project(zero)
    sd.backend_set_option("fusion", 0)
    try:
        zplain = e.ip_adapter_project(zero)
    finally:
        sd.backend_set_option("fusion", 1)
    zerr, zerr_plain = CV.rel_l2(zgot, zref), CV.rel_l2(zplain, zref)
    print(f"[resampler zeros n_tok {n_tok} N {N}] rel-L2 vs torch fp64: fused {zerr:.3e}, fusion = 0 {zerr_plain:.3e}, bound {1.5 * zerr_plain:.3e}")
    assert np.abs(zref).max() > 0 and zerr <= 1.5 * zerr_plain
    for b in range(1, N):
        assert np.array_equal(zgot[b], zgot[0])


# ---------------------------------------------------------------------------------------------------- end to end
def _traj(sd, e, device):
    rng = np.random.default_rng(5)
    cond, uncond = rng.standard_normal((1, 77, 64)).astype(np.float32), rng.standard_normal((1, 77, 64)).astype(np.float32)
    return e.sample_latents(cond, uncond, width=128, height=128, steps=3, cfg=7.5, seed=11, batch=2, method=sd.EULER_A, device_sampler=device, fuse_cfg=True)


def _adapter_engine(sd, gpu, plus):
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    if plus:
        e.ip_adapter_init_plus(64, 128, 2, 16, 160, 256, 9)
        e.clip_vision_init(hidden=160, heads=2, layers=3, image_size=28, patch_size=14, proj=48, weight_seed=5)
    else:
        e.ip_adapter_init(64, 48, 4, 9)
        e.clip_vision_init(hidden=128, heads=2, layers=2, image_size=28, patch_size=14, proj=48, weight_seed=5)
    return e


@pytest.mark.parametrize("plus", [False, True], ids=["plain", "plus"])
@pytest.mark.parametrize("device", [False, True], ids=["host_loop", "device_sampler"])
def test_image_tokens_end_to_end(sd, gpu, plus, device):
    if plus and not ON_GPU:
        pytest.skip("self-check mode on the CPU oracle: no GELU_ERF there")
    e = _adapter_engine(sd, gpu, plus)
    img = np.random.default_rng(8).integers(0, 256, (45, 60, 3), dtype=np.uint8)
    bare = _traj(sd, sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True), device)
    assert np.array_equal(_traj(sd, e, device), bare)  # adapter and tower initialised, nothing set: the graphs of a context without them
    e.set_ip_adapter(image=img, strength=0.6)
    a = _traj(sd, e, device)
    # the same by hand: preprocess -> encode -> project -> set_ip_adapter(tokens, uncond from zeros)
    px = e.clip_preprocess(img)
    emb = e.clip_vision_encode(px, False, 2) if plus else e.clip_vision_encode(px, True, -1)
    tok = e.ip_adapter_project(emb)[0]
    un = e.ip_adapter_project(np.zeros_like(emb))[0]
    e.set_ip_adapter(tokens=tok, uncond_tokens=un, strength=0.6)
    b = _traj(sd, e, device)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    assert not np.array_equal(a, bare)
    if plus:  # all-zero hidden states give the uncond tokens set_ip_adapter(image=...) installs: leaving uncond to the default gives the same trajectory
        e.set_ip_adapter(tokens=tok, strength=0.6)
        assert np.array_equal(_traj(sd, e, device), a)
    e.set_ip_adapter(image=img, strength=0.0)
    assert np.array_equal(_traj(sd, e, device), bare)
    e.set_ip_adapter()
    assert np.array_equal(_traj(sd, e, device), bare)


def test_mismatched_tower_and_adapter_is_an_error(sd, gpu):
    img = np.zeros((30, 30, 3), np.uint8)
    e = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    e.ip_adapter_init(64, 32, 4, 1)  # reads 32-wide embeddings
    with pytest.raises(sd.EngineError, match="no vision tower"):
        e.set_ip_adapter(image=img)
    e.clip_vision_init(hidden=128, heads=2, layers=1, image_size=28, patch_size=14, proj=48, weight_seed=5)  # projects to 48
    with pytest.raises(sd.EngineError, match="expects"):
        e.set_ip_adapter(image=img)
    p = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    p.ip_adapter_init_plus(64, 128, 1, 16, 160, 256, 1)  # reads 160-wide hidden states
    p.clip_vision_init(hidden=128, heads=2, layers=2, image_size=28, patch_size=14, proj=160, weight_seed=5)  # hidden 128 (the projection width does not matter for plus)
    with pytest.raises(sd.EngineError, match="expects"):
        p.set_ip_adapter(image=img)
    t = sd.Engine(model=sd.SD15_TINY, backend=gpu, flash_attn=True)
    t.clip_vision_init(hidden=128, heads=2, layers=1, image_size=28, patch_size=14, proj=48, weight_seed=5)
    with pytest.raises(sd.EngineError, match="no IP-Adapter"):
        t.set_ip_adapter(image=img)
