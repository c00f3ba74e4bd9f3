"""Inpaint / pix2pix UNets on the oracle backend: variant contexts, the forward with c_concat against the PyTorch restatement, the three-conditioning guidance
combine bit for bit against the reference's guidance.cpp (oracle/_ref, when it is here) and the NumPy restatement (concat_cfg_ref.py), the mask stages against
hand-written expectations, the host loop / fused branches / device-resident sampler against each other bit for bit, the refusals, the checkpoint probe and the
condition made from pixels."""
import ctypes as C
import json
import struct
from pathlib import Path

import numpy as np
import pytest

import concat_cfg_ref as ref
from oracle import torch_ref
from ref_graphs import engine_graph_description, split_description

ROOT = Path(__file__).resolve().parent.parent
W0 = "model.diffusion_model.input_blocks.0.0.weight"
SCALE_PAIRS = ((7.5, 1.5), (1.0, 1.5), (3.0, 3.0), (7.0, 1.0))   # (txt_cfg, img_cfg)
RULE = {(7.5, 1.5): (True, True), (1.0, 1.5): (True, True), (3.0, 3.0): (False, True), (7.0, 1.0): (True, False)}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.fixture(scope="module")
def engines(sd, oracle):
    made = {}

    def get(name, variant):
        if (name, variant) not in made:
            made[(name, variant)] = sd.Engine(model=getattr(sd, name), backend=oracle, variant=variant)
        return made[(name, variant)]

    return get


# ---------------------------------------------------------------------------------------------------------------- guidance combine
def test_cfg_combine3_bit_exact(sd):
    """all three forms x the four scale pairs, on vectors with signed zeros, subnormals and 1e30-scale values: engine == NumPy restatement == the reference's own
    ClassifierFreeGuidance::forward compiled into oracle/_ref (live when that library is here, like tests/test_host_logic.py)"""
    ref_so = ROOT / "oracle" / "_ref" / "libref_guidance.so"
    R = None
    if ref_so.exists():
        R = C.CDLL(str(ref_so))
        R.ref_cfg_combine.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_float, C.c_void_p]
        R.ref_cfg_combine.restype = C.c_int
    c, u, iu = ref.special_vectors(20011, seed=17)
    for txt, img in SCALE_PAIRS:
        assert ref.branch_rule(txt, img) == RULE[(txt, img)]
        for uu, ii in ((u, iu), (None, iu), (u, None), (None, None)):
            want = ref.cfg_combine3(c, uu, ii, txt, img)
            got = sd.cfg_combine3(c, uu, ii, txt, img)
            assert ref.same_bits(got, want), (txt, img, uu is None, ii is None)
            if R is not None:
                o = np.empty_like(c)
                assert R.ref_cfg_combine(c.ctypes.data, None if uu is None else uu.ctypes.data, None if ii is None else ii.ctypes.data, c.size, txt, img, o.ctypes.data) == 0
                assert ref.same_bits(o, want), (txt, img, uu is None, ii is None)
    # the two-prediction form is the existing combine
    assert ref.same_bits(sd.cfg_combine3(c, u, None, 7.0, 1.0), sd.cfg_combine(c, u, 7.0))
    # and a contracted multiply-add would show: the restatement is not vacuous
    assert not ref.same_bits(ref.cfg_combine3_contracted(c, u, iu, 7.5, 1.5), ref.cfg_combine3(c, u, iu, 7.5, 1.5))


# ---------------------------------------------------------------------------------------------------------------- mask stages
def test_mask_stages_known_answers(sd):
    m = np.zeros((16, 24), np.float32)   # [H, W] = 16 x 24 pixels -> 2 x 3 latent cells
    m[7, 8] = 1.0                        # the last row of block row 0, the first column of block column 1
    want = np.zeros((2, 3), np.float32)
    want[0, 1] = 1.0
    np.testing.assert_array_equal(sd.latent_mask(m), want)
    np.testing.assert_array_equal(ref.latent_mask(m), want)
    # sd::ops::round is std::round (src/core/tensor.hpp:1089-1092): halves go away from zero, so 0.5 counts as masked and 0.49 does not
    h = np.zeros((16, 24), np.float32)
    h[15, 23] = 0.5
    h[0, 0] = 0.49
    want = np.zeros((2, 3), np.float32)
    want[1, 2] = 1.0
    np.testing.assert_array_equal(sd.latent_mask(h), want)
    np.testing.assert_array_equal(ref.latent_mask(h), want)
    np.testing.assert_array_equal(sd.latent_mask(np.zeros((16, 24), np.float32)), np.zeros((2, 3), np.float32))
    # max-pool at the four borders: a corner cell, one cell on each remaining edge
    for (y, x), cells in {(0, 0): [(0, 0), (0, 1), (1, 0), (1, 1)],
                          (0, 3): [(0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4)],
                          (3, 0): [(2, 0), (3, 0), (2, 1), (3, 1)],
                          (2, 4): [(1, 3), (1, 4), (2, 3), (2, 4), (3, 3), (3, 4)]}.items():
        a = np.zeros((4, 5), np.float32)
        a[y, x] = 1.0
        want = np.zeros((4, 5), np.float32)
        for cy, cx in cells:
            want[cy, cx] = 1.0
        np.testing.assert_array_equal(sd.mask_max_pool3(a), want)
        np.testing.assert_array_equal(ref.max_pool3(a), want)
    neg = -np.ones((3, 3), np.float32)   # cells outside the map do not take part: no zero padding shows
    np.testing.assert_array_equal(sd.mask_max_pool3(neg), neg)


# ---------------------------------------------------------------------------------------------------------------- variant contexts
def test_variant_contexts(sd, oracle, engines):
    for name, mc in (("SD15_TINY", 32), ("SDXL_TINY", 32)):
        for variant, ic, cc in ((sd.UNET_INPAINT, 9, 5), (sd.UNET_PIX2PIX, 8, 4)):
            e = engines(name, variant)
            assert e.tensor_info(W0)[0] == [3, 3, ic, mc] and e.concat_channels() == cc and e.unet_variant() == variant
    plain = engines("SD15_TINY", sd.UNET_PLAIN)
    assert plain.tensor_info(W0)[0] == [3, 3, 4, 32] and plain.concat_channels() == 0
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 4, 8, 8)).astype(np.float32)
    t = np.array([300.0], np.float32)
    ctx = rng.standard_normal((1, 77, 64)).astype(np.float32)
    with pytest.raises(sd.EngineError, match="model needs c_concat"):
        e.unet_forward(x, t, ctx)
    with pytest.raises(sd.EngineError, match="the model takes 5"):
        e.unet_forward(x, t, ctx, c_concat=np.zeros((1, 4, 8, 8), np.float32))
    with pytest.raises(sd.EngineError, match="takes no c_concat"):
        plain.unet_forward(x, t, ctx, c_concat=np.zeros((1, 5, 8, 8), np.float32))
    with pytest.raises(sd.EngineError, match="UNet families"):
        sd.Engine(model=sd.SD35_TINY, backend=oracle, variant=sd.UNET_INPAINT)
    with pytest.raises(sd.EngineError, match="UNet families"):
        sd.Engine(model=sd.FLUX_TINY, backend=oracle, variant=sd.UNET_PIX2PIX)


@pytest.mark.parametrize("name,variant", [("SD15_TINY", 1), ("SD15_TINY", 2), ("SDXL_TINY", 1)])
def test_forward_with_concat_vs_torch(sd, engines, name, variant):
    """the bound of tests/test_model_cpu.py::test_unet_graph_vs_torch for these two models; torch reads the engine's weights by name and takes the 9- / 8-wide input"""
    e = engines(name, variant)
    cc = e.concat_channels()
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 4, 16, 16)).astype(np.float32)
    ctx = rng.standard_normal((1, 77, 64)).astype(np.float32)
    y = rng.standard_normal((1, 96)).astype(np.float32) if "XL" in name else None
    t = np.array([500.0, 37.5], dtype=np.float32)
    cat1 = rng.standard_normal((1, cc, 16, 16)).astype(np.float32)
    catn = rng.standard_normal((2, cc, 16, 16)).astype(np.float32)
    for cat in (cat1, catn):
        a = e.unet_forward(x, t, ctx, y, c_concat=cat)
        full = np.concatenate([x, np.broadcast_to(cat, (2,) + cat.shape[1:])], 1)
        assert rel_l2(a, torch_ref.unet_forward(e, name, full, t, ctx, y)) < 3e-3
    np.testing.assert_array_equal(e.unet_forward(x, t, ctx, y, c_concat=cat1), e.unet_forward(x, t, ctx, y, c_concat=np.repeat(cat1, 2, 0)))


def test_graph_shape(sd, engines):
    """[REPEAT,] CONCAT(dim 2) feed the first conv and nothing else changed against the plain context's graph"""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 4, 8, 8)).astype(np.float32)
    t = np.array([500.0, 20.0], np.float32)
    ctx = rng.standard_normal((1, 77, 64)).astype(np.float32)
    plain, inp = engines("SD15_TINY", sd.UNET_PLAIN), engines("SD15_TINY", sd.UNET_INPAINT)
    ops = lambda desc: [ln.split()[2] for ln in split_description(desc)[1]]
    base = ops(engine_graph_description(lambda: plain.unet_forward(x, t, ctx)))
    for cat, extra in ((np.zeros((1, 5, 8, 8), np.float32), ["REPEAT", "CONCAT"]), (np.zeros((2, 5, 8, 8), np.float32), ["CONCAT"])):
        desc = engine_graph_description(lambda: inp.unet_forward(x, t, ctx, c_concat=cat))
        got = ops(desc)
        assert len(got) == len(base) + len(extra)
        nodes = split_description(desc)[1]
        first_im2col = min(i for i, ln in enumerate(nodes) if ln.split()[2] == "IM2COL")
        ic = first_im2col - 1
        field = lambda ln, key: next(tok[len(key):] for tok in ln.split() if tok.startswith(key))
        assert got[ic] == "CONCAT" and f"1:n{ic}" in field(nodes[first_im2col], "s=").split(","), "the first conv reads the CONCAT: " + nodes[first_im2col]
        assert field(nodes[ic], "p=") == "2" and field(nodes[ic], "ne=") == "8,8,9,2", "CONCAT along dim 2: " + nodes[ic]
        if extra[0] == "REPEAT":
            assert got[ic - 1] == "REPEAT" and f"1:n{ic - 1}" in field(nodes[ic], "s=").split(",")
        assert got[:ic + 1 - len(extra)] + got[ic + 1:] == base


# ---------------------------------------------------------------------------------------------------------------- trajectories
def _cond(seed=5):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((1, 77, 64)).astype(np.float32), rng.standard_normal((1, 77, 64)).astype(np.float32)


def _sample(sd, e, k, method, **over):
    """k = 1: no guidance pair; 2: cond / uncond; 3: + img_uncond"""
    cond, uncond = _cond()
    e.set_img_cfg(1.5 if k == 3 else float("inf"))
    kw = dict(width=128, height=128, steps=3, cfg=1.0 if k == 1 else 7.5, seed=11, batch=2, method=method)
    kw.update(over)
    return e.sample_latents(cond, None if k == 1 else uncond, **kw)


@pytest.mark.parametrize("method", ["EULER", "EULER_A"])
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("concat_n", [1, 2])
def test_device_sampler_equals_host_loop(sd, engines, method, k, concat_n):
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    m = getattr(sd, method)
    rng = np.random.default_rng(40 + concat_n)
    cat = rng.standard_normal((concat_n, 5, 16, 16)).astype(np.float32)
    cat[:, 0] = (cat[:, 0] > 0)
    try:
        e.set_concat_condition(cat)
        host = _sample(sd, e, k, m)
        assert np.isfinite(host).all()
        np.testing.assert_array_equal(_sample(sd, e, k, m, fuse_cfg=True), host)
        np.testing.assert_array_equal(_sample(sd, e, k, m, fuse_cfg=True, device_sampler=True), host)
        np.testing.assert_array_equal(_sample(sd, e, k, m, device_sampler=True, device_batch=1), host)   # device groups take their slice of a per-image concat
        if k == 3:   # the third branch does something: another img_uncond concat, another result
            e.set_concat_condition(cat, np.zeros_like(cat))
            assert not np.array_equal(_sample(sd, e, k, m), host)
    finally:
        e.set_concat_condition(None)
        e.set_img_cfg()


def test_two_branch_forms_and_cfgpp_base(sd, engines):
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    rng = np.random.default_rng(50)
    cat = rng.standard_normal((1, 5, 16, 16)).astype(np.float32)
    cond, uncond = _cond()
    kw = dict(width=128, height=128, steps=3, seed=4, batch=1)
    try:
        e.set_concat_condition(cat)
        # img_cfg == txt_cfg: the uncond branch does not run, cond and img_uncond combine — on every path alike
        e.set_img_cfg(3.0)
        c0 = e.stats()["unet_calls"]
        a = e.sample_latents(cond, uncond, cfg=3.0, method=sd.EULER, **kw)
        assert e.stats()["unet_calls"] - c0 == 2 * 3
        np.testing.assert_array_equal(e.sample_latents(cond, uncond, cfg=3.0, method=sd.EULER, fuse_cfg=True, device_sampler=True, **kw), a)
        # a CFG++ method takes its denoised_uncond from img_uncond first: with three branches its result moves with img_uncond_concat even at img_cfg == txt_cfg ...
        e.set_img_cfg(1.5)
        b = e.sample_latents(cond, uncond, cfg=7.5, method=sd.EULER_CFG_PP, **kw)
        e.set_concat_condition(cat, cat * 0.5)
        assert not np.array_equal(e.sample_latents(cond, uncond, cfg=7.5, method=sd.EULER_CFG_PP, **kw), b)
        # ... and with the img_uncond branch off (img_cfg 1) it does not: the base is uncond
        e.set_img_cfg(1.0)
        e.set_concat_condition(cat)
        c = e.sample_latents(cond, uncond, cfg=7.5, method=sd.EULER_CFG_PP, **kw)
        e.set_concat_condition(cat, cat * 0.5)
        np.testing.assert_array_equal(e.sample_latents(cond, uncond, cfg=7.5, method=sd.EULER_CFG_PP, **kw), c)
    finally:
        e.set_concat_condition(None)
        e.set_img_cfg()


def test_plain_context_ignores_img_cfg(sd, engines):
    e = engines("SD15_TINY", sd.UNET_PLAIN)
    cond, uncond = _cond()
    kw = dict(width=128, height=128, steps=3, cfg=7.5, seed=2, batch=2, method=sd.EULER_A)
    want = e.sample_latents(cond, uncond, **kw)
    want_dev = e.sample_latents(cond, uncond, fuse_cfg=True, device_sampler=True, **kw)
    try:
        assert "3-conditioning CFG is not supported" in e.set_img_cfg(2.0)
        np.testing.assert_array_equal(e.sample_latents(cond, uncond, **kw), want)
        np.testing.assert_array_equal(e.sample_latents(cond, uncond, fuse_cfg=True, device_sampler=True, **kw), want_dev)
    finally:
        e.set_img_cfg()
    with pytest.raises(sd.EngineError, match="takes no c_concat"):
        e.set_concat_condition(np.zeros((1, 5, 16, 16), np.float32))


def test_refusals(sd, engines):
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    cond, uncond = _cond()
    kw = dict(width=128, height=128, steps=3, cfg=7.5, seed=2, batch=1, method=sd.EULER)
    with pytest.raises(sd.EngineError, match="model needs c_concat"):
        e.sample_latents(cond, uncond, **kw)
    with pytest.raises(sd.EngineError, match="sd_set_concat_condition"):
        e.set_concat_condition(np.zeros((1, 4, 16, 16), np.float32))
    cat = np.random.default_rng(6).standard_normal((1, 5, 16, 16)).astype(np.float32)
    try:
        e.set_concat_condition(cat)
        with pytest.raises(sd.EngineError, match="concat condition is"):
            e.sample_latents(cond, uncond, **dict(kw, width=64))
        e.set_img_cfg(1.5)
        for dev in (False, True):
            with pytest.raises(sd.EngineError, match="adaptive projected guidance"):
                e.sample_latents(cond, uncond, apg=(0.5, 0.0, 0.0, 0.0), device_sampler=dev, fuse_cfg=dev, **kw)
            e.set_step_cache(sd.CACHE_UCACHE, reuse_threshold=1.0)
            with pytest.raises(sd.EngineError, match="step cache"):
                e.sample_latents(cond, uncond, device_sampler=dev, fuse_cfg=dev, **kw)
            e.set_step_cache(None)
            e.set_pair_exchange(lambda ptr, count, stream: True, branch=0)
            with pytest.raises(sd.EngineError, match="CFG-pair exchange"):
                e.sample_latents(cond, uncond, device_sampler=dev, fuse_cfg=dev, **kw)
            e.set_pair_exchange(None)
        # two-branch concat sampling with a cache is allowed and works: host loop, fused pair and device sampler decide alike
        e.set_img_cfg()
        e.set_step_cache(sd.CACHE_UCACHE, reuse_threshold=1.0)
        long = dict(kw, steps=10)
        a = e.sample_latents(cond, uncond, **long)
        skipped = e.stats()["steps_skipped"]
        dec = [(r["step"], r["skipped"]) for r in e.step_cache_trace()]
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(e.sample_latents(cond, uncond, fuse_cfg=True, **long), a)
        e.sample_latents(cond, uncond, fuse_cfg=True, device_sampler=True, **long)
        assert [(r["step"], r["skipped"]) for r in e.step_cache_trace()] == dec and e.stats()["steps_skipped"] == skipped
    finally:
        e.set_pair_exchange(None)
        e.set_step_cache(None)
        e.set_concat_condition(None)
        e.set_img_cfg()


# ---------------------------------------------------------------------------------------------------------------- checkpoint probe
def _write_safetensors(path, tensors):
    header, blobs, off = {}, [], 0
    for name, arr in tensors.items():
        raw = np.ascontiguousarray(arr, np.float32).tobytes()
        header[name] = {"dtype": "F32", "shape": list(arr.shape), "data_offsets": [off, off + len(raw)]}
        blobs.append(raw)
        off += len(raw)
    hj = json.dumps(header).encode()
    hj += b" " * ((8 - len(hj) % 8) % 8)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(hj)))
        f.write(hj)
        for b in blobs:
            f.write(b)


def test_probe_unet_variant(sd, tmp_path):
    for ic, want in ((4, sd.UNET_PLAIN), (9, sd.UNET_INPAINT), (8, sd.UNET_PIX2PIX)):
        p = tmp_path / f"w{ic}.safetensors"
        _write_safetensors(p, {W0: np.zeros((32, ic, 3, 3), np.float32), "model.diffusion_model.out.2.bias": np.zeros(4, np.float32)})
        assert sd.probe_unet_variant(p) == want
    p = tmp_path / "diffusers.safetensors"
    _write_safetensors(p, {"conv_in.weight": np.zeros((32, 9, 3, 3), np.float32)})
    assert sd.probe_unet_variant(p) == sd.UNET_INPAINT
    p = tmp_path / "w5.safetensors"
    _write_safetensors(p, {W0: np.zeros((32, 5, 3, 3), np.float32)})
    with pytest.raises(sd.EngineError, match="5 input channels"):
        sd.probe_unet_variant(p)
    p = tmp_path / "none.safetensors"
    _write_safetensors(p, {"model.diffusion_model.out.2.bias": np.zeros(4, np.float32)})
    with pytest.raises(sd.EngineError, match="holds no"):
        sd.probe_unet_variant(p)


def test_load_real_width_first_conv(sd, engines, tmp_path):
    """sd_load_weights takes a 9-channel input_blocks.0.0.weight on an inpaint context"""
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    old = e.get_tensor(W0)
    w = (np.random.default_rng(8).standard_normal((32, 9, 3, 3)) * 0.05).astype(np.float32)
    p = tmp_path / "first.safetensors"
    _write_safetensors(p, {W0: w})
    try:
        assert e.load_weights(p)["loaded"] == 1
        np.testing.assert_array_equal(e.get_tensor(W0), w.astype(np.float16).astype(np.float32))
    finally:
        e.set_tensor(W0, old)


# ---------------------------------------------------------------------------------------------------------------- the condition from pixels
def test_make_inpaint_condition(sd, engines):
    rng = np.random.default_rng(9)
    rgb = rng.random((3, 64, 128)).astype(np.float32)   # (latents 16 x 8: the UNet halves its maps three times)
    mask = np.zeros((64, 128), np.float32)
    mask[5:20, 10:30] = 1.0
    mask[50, 100] = 0.5
    e = engines("SD15_TINY", sd.UNET_INPAINT)
    out = e.make_inpaint_condition(rgb, mask, seed=7)
    lm = sd.latent_mask(mask)
    np.testing.assert_array_equal(out["concat"][0], lm)
    np.testing.assert_array_equal(lm, ref.latent_mask(mask))
    rounded = (mask >= 0.5).astype(np.float32)
    masked = ((np.float32(1.0) - rounded) * (rgb - np.float32(0.5))) + np.float32(0.5)
    np.testing.assert_array_equal(out["concat"][1:], e.vae_encode(masked[None], seed=7)[0])
    np.testing.assert_array_equal(out["img_uncond_concat"][0], lm)
    assert not out["img_uncond_concat"][1:].any()
    np.testing.assert_array_equal(out["denoise_mask"], sd.mask_max_pool3(lm))
    np.testing.assert_array_equal(out["init_latent"], e.vae_encode(rgb[None], seed=7)[0])
    # the derived default of sd_set_concat_condition is the same mask | zeros: a three-branch trajectory does not change when it is given explicitly
    cond, uncond = _cond()
    kw = dict(width=128, height=64, steps=2, cfg=7.5, seed=1, batch=1, method=sd.EULER)
    try:
        e.set_img_cfg(1.5)
        e.set_concat_condition(out["concat"])
        a = e.sample_latents(cond, uncond, **kw)
        e.set_concat_condition(out["concat"], out["img_uncond_concat"])
        np.testing.assert_array_equal(e.sample_latents(cond, uncond, **kw), a)
    finally:
        e.set_concat_condition(None)
        e.set_img_cfg()
    # pix2pix on SD1.x: the encoder's mean, neither sampled nor scaled
    p = engines("SD15_TINY", sd.UNET_PIX2PIX)
    lat, mom = p.vae_encode(rgb[None], seed=7, return_moments=True)
    np.testing.assert_array_equal(lat, mom[:, :4])
    o2 = p.make_inpaint_condition(rgb, None, seed=7)
    np.testing.assert_array_equal(o2["concat"], mom[0, :4])
    assert not o2["img_uncond_concat"].any() and "denoise_mask" not in o2
    # SDXL pix2pix encodes normally: sampled and scaled, as a plain SDXL context does
    px, pl = engines("SDXL_TINY", sd.UNET_PIX2PIX), engines("SDXL_TINY", sd.UNET_PLAIN)
    np.testing.assert_array_equal(px.vae_encode(rgb[None], seed=7), pl.vae_encode(rgb[None], seed=7))
