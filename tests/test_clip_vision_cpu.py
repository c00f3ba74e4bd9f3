"""CPU suite: the CLIP vision tower, the Resampler of the "plus" IP-Adapters and the CLIP preprocessing (csrc/host/clip_vision.hpp, engine entry points).

  * node-for-node structure of the tower and Resampler graphs against the op / shape sequence of the reference lines (clip.hpp:212-237, :364-391, :447-463,
    :44-123, ggml_extend.hpp:1349-1485; ip_adapter.hpp:68-113), written out below;
  * tower numerics on the CPU oracle against PyTorch float64 (the tower has no GELU_ERF);
  * the Resampler's GELU_ERF: the CPU oracle does not implement it and the engine says so instead of submitting the graph;
  * the tower file's name rule against a table the reference's own converter produced; plus / plain adapter files told apart; loader round trips;
  * the preprocessing restatement: shapes, bit-equality of the engine's host path, and five mutants that must each change the output."""
import json
from pathlib import Path

import numpy as np
import pytest

import clip_vision_ref as CV
from ref_graphs import engine_graph_description, split_description
from test_model_io import _write_safetensors

ROOT = Path(__file__).resolve().parent.parent


def _engine(sd, oracle, flash=False):
    return sd.Engine(model=sd.SD15_TINY, backend=oracle, flash_attn=flash)


def _ops(desc):
    """[(op, (ne0, ne1, ne2, ne3))] of a description's nodes; UNARY nodes carry their unary-op number"""
    out = []
    for line in split_description(desc)[1]:
        f = line.split()
        ne = tuple(int(v) for v in f[4][3:].split(","))
        op = f[2]
        if op == "UNARY":
            op += ":" + f[6][2:]
        out.append((op, ne))
    return out


# ---------------------------------------------------------------------------------------------------- expected sequences
def _linear(out, rows, N, bias=True):  # ggml_ext_linear: MUL_MAT [+ ADD in place]
    return [("MUL_MAT", (out, rows, N, 1))] + ([("ADD", (out, rows, N, 1))] if bias else [])


def _layer_norm(dim, rows, N):  # ggml_ext_layer_norm: NORM, MUL, ADD
    return [(op, (dim, rows, N, 1)) for op in ("NORM", "MUL", "ADD")]


def _manual_attention(C, heads, Lq, Lk, N, q_ops, k_ops, v_ops):
    """ggml_ext_attention_ext without flash (ggml_extend.hpp:1383-1404, 1455-1485).  The graph lists a node's sources depth first, so the order is
    v-chain, k-chain, q-chain, kq ..., exactly as sdm_graph_describe prints the reference's own graphs (tests/test_ref_graphs.py)."""
    d = C // heads
    seq = []
    seq += v_ops + [("RESHAPE", (d, heads, Lk, N)), ("PERMUTE", (Lk, d, heads, N)), ("CONT", (Lk, d, heads, N)), ("RESHAPE", (Lk, d, heads * N, 1))]
    seq += k_ops + [("RESHAPE", (d, heads, Lk, N)), ("PERMUTE", (d, Lk, heads, N)), ("CONT", (d, Lk, heads, N)), ("RESHAPE", (d, Lk, heads * N, 1))]
    seq += q_ops + [("RESHAPE", (d, heads, Lq, N)), ("PERMUTE", (d, Lq, heads, N)), ("CONT", (d, Lq, heads, N)), ("RESHAPE", (d, Lq, heads * N, 1))]
    seq += [("MUL_MAT", (Lk, Lq, heads * N, 1)), ("SCALE", (Lk, Lq, heads * N, 1)), ("SOFT_MAX", (Lk, Lq, heads * N, 1)), ("MUL_MAT", (d, Lq, heads * N, 1)),
            ("RESHAPE", (d, Lq, heads, N)), ("PERMUTE", (d, heads, Lq, N)), ("CONT", (d, heads, Lq, N)), ("RESHAPE", (C, Lq, N, 1))]
    return seq


def expected_tower(un, info, N, pooled, clip_skip):
    E, P, S, T, I, H, L = (info[k] for k in ("hidden_size", "patch_size", "image_size", "num_positions", "intermediate_size", "n_head", "n_layer"))
    G, np_, K = S // P, T - 1, 3 * P * P
    seq = [("REPEAT", (E, N, 1, 1)), ("RESHAPE", (1, E, 1, N)),                                        # clip.hpp:229-231
           ("IM2COL", (K, G, G, N)), ("RESHAPE", (K, N * np_, 1, 1)), ("RESHAPE", (K, E, 1, 1)), ("MUL_MAT", (N * np_, E, 1, 1)),
           ("RESHAPE", (G, G, N, E)), ("PERMUTE", (G, G, E, N)), ("CONT", (G, G, E, N)),                  # :224 (ggml_conv_2d)
           ("RESHAPE", (np_, E, N, 1)), ("PERMUTE", (E, np_, N, 1)), ("CONT", (E, np_, N, 1)), ("RESHAPE", (1, E, np_, N)),  # :225-227
           ("CONCAT", (1, E, T, N)), ("RESHAPE", (E, T, N, 1)), ("ADD", (E, T, N, 1))]                    # :233-235
    seq += _layer_norm(E, T, N)                                                                          # pre_layernorm, :375
    for _ in range(CV.layers_run(L, clip_skip)):                                                         # :102-112
        seq += _layer_norm(E, T, N)                                                                      # layer_norm1, :73
        seq += _manual_attention(E, H, T, T, N, _linear(E, T, N), _linear(E, T, N), _linear(E, T, N))    # MultiheadAttention, ggml_extend.hpp:4025-4096
        seq += _linear(E, T, N) + [("ADD", (E, T, N, 1))]                                                # out_proj, residual
        seq += _layer_norm(E, T, N) + _linear(I, T, N)                                                   # layer_norm2, fc1
        seq += [("UNARY:" + str(un["GELU" if info["use_gelu"] else "GELU_QUICK"]), (I, T, N, 1))]  # :33-38
        seq += _linear(E, T, N) + [("ADD", (E, T, N, 1))]                                                # fc2, residual
    if pooled:
        seq += _layer_norm(E, T, N)                                                                      # post_layernorm, :381
        seq += [("VIEW", (E, N, 1, 1)), ("CONT", (E, N, 1, 1)), ("MUL_MAT", (info["projection_dim"], N, 1, 1))]  # :385, :459
    return seq


def expected_resampler(un, dim, depth, nq, embed, out, ff, n_tok, N):
    heads = dim // 64
    Lk = n_tok + nq
    # the first layer's residual ADD(latents, attn) lists the latents first: their REPEAT (N > 1 only, :76-78) precedes proj_in (:74), which is listed where norm1 reads it
    seq = ([("REPEAT", (dim, nq, N, 1))] if N > 1 else []) + _linear(dim, n_tok, N)
    for _ in range(depth):
        norm2 = _layer_norm(dim, nq, N)                                                                  # :89
        norm1 = _layer_norm(dim, n_tok, N)                                                               # :88
        kv = norm1 + norm2 + [("CONCAT", (dim, Lk, N, 1))] + _linear(2 * dim, Lk, N, bias=False)          # :91-92
        v_ops = kv + [("VIEW", (dim, Lk, N, 1)), ("CONT", (dim, Lk, N, 1))]                               # :95
        k_ops = [("VIEW", (dim, Lk, N, 1)), ("CONT", (dim, Lk, N, 1))]                                    # :94 (kv is listed already)
        q_ops = _linear(dim, nq, N, bias=False)                                                          # :90 (norm2 is listed already)
        att = _manual_attention(dim, heads, nq, Lk, N, q_ops, k_ops, v_ops)
        seq_layer = att + _linear(dim, nq, N, bias=False) + [("ADD", (dim, nq, N, 1))]                   # :97-98
        seq_layer += _layer_norm(dim, nq, N) + _linear(ff, nq, N, bias=False)                             # :103-104
        seq_layer += [("UNARY:" + str(un["GELU_ERF"]), (ff, nq, N, 1))]                       # :105
        seq_layer += _linear(dim, nq, N, bias=False) + [("ADD", (dim, nq, N, 1))]                         # :106-107
        seq += seq_layer
    seq += _linear(out, nq, N) + _layer_norm(out, nq, N)                                                 # :110-111
    return seq


@pytest.fixture(scope="module")
def unary_numbers(sd):
    """{name: the host's ggml_unary_op number} (ggml_unary_op_name scanned like the backend scans it)"""
    import ctypes as C

    L = sd.lib()
    L.ggml_unary_op_name.argtypes = [C.c_int]
    L.ggml_unary_op_name.restype = C.c_char_p
    table = {}
    for i in range(32):
        nm = L.ggml_unary_op_name(i)
        if nm:
            table.setdefault(nm.decode(), i)
    return table


def _multiset_diff(a, b):
    from collections import Counter

    ca, cb = Counter(a), Counter(b)
    return {"missing": dict(cb - ca), "extra": dict(ca - cb)}


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("pooled,clip_skip", [(True, -1), (False, -1), (False, 2), (True, 2)])
def test_tower_graph_is_the_reference_sequence(sd, oracle, unary_numbers, N, pooled, clip_skip):
    e = _engine(sd, oracle)
    e.clip_vision_init(hidden=128, heads=2, layers=3, image_size=28, patch_size=14, proj=32, weight_seed=1)
    info = e.clip_vision_info()
    px = np.zeros((N, 3, 28, 28), np.float32)
    got = _ops(engine_graph_description(lambda: e.clip_vision_encode(px, pooled, clip_skip), compute=False))
    want = expected_tower(unary_numbers, info, N, pooled, clip_skip)
    # the embeddings prelude and the tail are compared in order; inside a layer the depth-first listing of the attention's sources is compared in order too
    assert got == want, _multiset_diff(got, want)
    layers_run = 3 if clip_skip <= 0 else 3 - clip_skip + 1
    assert sum(1 for op, _ in got if op.startswith("UNARY")) == layers_run
    assert sum(1 for op, _ in got if op == "NORM") == 1 + 2 * layers_run + (1 if pooled else 0)  # non-pooled: the state BEFORE post_layernorm (clip.hpp:389)


def test_tower_configs_restate_the_reference(sd, oracle):
    """vit_l / vit_h / vit_bigg hyper-parameters (clip.hpp:339-356, 428-441) and the activation rule (:21-25): tanh-GELU only at d_model 1024 / 1280"""
    import os

    os.environ["SDCPP_SKIP_WEIGHT_INIT"] = "1"  # shapes only: no 600 M-parameter fill
    try:
        for ver, want in ((sd.CLIP_VIT_L_14, (1024, 4096, 16, 24, 768, 1)), (sd.CLIP_VIT_H_14, (1280, 5120, 16, 32, 1024, 1)), (sd.CLIP_VIT_BIGG_14, (1664, 8192, 16, 48, 768, 0))):
            e = _engine(sd, oracle)
            e.clip_vision_init(ver)
            i = e.clip_vision_info()
            assert (i["hidden_size"], i["intermediate_size"], i["n_head"], i["n_layer"], i["projection_dim"], i["use_gelu"]) == want
            assert (i["image_size"], i["patch_size"], i["num_positions"]) == (224, 14, 257)
            _, ty, _ = e.tensor_info("clip_vision.vision_model.embeddings.patch_embedding.weight")
            assert ty == sd.F16
            assert e.tensor_info("clip_vision.vision_model.embeddings.class_embedding")[1] == sd.F32
            assert e.tensor_info("clip_vision.vision_model.embeddings.position_embedding.weight")[1] == sd.F32
            e.close()
    finally:
        del os.environ["SDCPP_SKIP_WEIGHT_INIT"]


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("n_tok", [5, 257])
def test_resampler_graph_is_the_reference_sequence(sd, oracle, unary_numbers, N, n_tok):
    e = _engine(sd, oracle)
    e.ip_adapter_init_plus(64, 128, 2, 16, 160, 256, 1)
    assert e.ip_adapter_is_plus() and e.ip_adapter_info() == (64, 160, 16)
    emb = np.zeros((N, n_tok, 160), np.float32)
    got = _ops(engine_graph_description(lambda: e.ip_adapter_project(emb), compute=False))
    want = expected_resampler(unary_numbers, 128, 2, 16, 160, 64, 256, n_tok, N)
    assert got == want, _multiset_diff(got, want)
    assert sum(1 for op, _ in got if op == "REPEAT") == (1 if N > 1 else 0)  # ip_adapter.hpp:76-78


def test_resampler_reports_gelu_erf_unsupported_on_the_cpu_oracle(sd, oracle):
    e = _engine(sd, oracle)
    e.ip_adapter_init_plus(64, 128, 2, 16, 160, 256, 1)
    with pytest.raises(sd.EngineError, match="GELU_ERF"):
        e.ip_adapter_project(np.zeros((1, 5, 160), np.float32))
    # the context is still usable afterwards
    assert e.ip_adapter_info() == (64, 160, 16)


# ---------------------------------------------------------------------------------------------------- tower numerics on the CPU oracle
@pytest.mark.parametrize("hidden", [128, 160])  # 2 heads: d = 64, and d = 80 (ViT-H's head size)
@pytest.mark.parametrize("flash", [False, True])
def test_tower_matches_torch_float64_on_the_cpu_oracle(sd, oracle, hidden, flash):
    """Tolerance 5e-3 rel-L2, the bar of this suite's whole-graph parity tests: the oracle rounds every Linear's activations to f16 (2^-11 relative per element, as
    ggml-cpu does for f16 weights) and reads quick-GELU from an f16 table; the weights are shared with the reference (read back from the engine)."""
    e = _engine(sd, oracle, flash)
    e.clip_vision_init(hidden=hidden, heads=2, layers=2, image_size=28, patch_size=14, proj=48, weight_seed=5)
    rng = np.random.default_rng(hidden)
    img = rng.integers(0, 256, (2, 31, 45, 3), dtype=np.uint8)
    px = e.clip_preprocess(img)
    for pooled, skip in ((True, -1), (False, 2)):
        got = e.clip_vision_encode(px, pooled, skip)
        ref = CV.tower(e, px, pooled, skip)
        err = CV.rel_l2(got, ref)
        print(f"tower hidden {hidden} flash {flash} pooled {pooled} clip_skip {skip}: rel-L2 vs torch fp64 {err:.2e}")
        assert got.shape == ref.shape and np.isfinite(got).all()
        assert err < 5e-3


def test_plain_adapter_from_a_picture_on_the_cpu_oracle(sd, oracle):
    """set_ip_adapter(image=...) = preprocess -> encode (pooled) -> project, uncond = the projection of zeros; errors instead of no-ops"""
    e = _engine(sd, oracle)
    img = np.random.default_rng(3).integers(0, 256, (40, 33, 3), dtype=np.uint8)
    with pytest.raises(sd.EngineError, match="no IP-Adapter"):
        e.set_ip_adapter(image=img)
    e.ip_adapter_init(64, 48, 4, 2)
    with pytest.raises(sd.EngineError, match="no vision tower"):
        e.set_ip_adapter(image=img)
    e.clip_vision_init(hidden=128, heads=2, layers=2, image_size=28, patch_size=14, proj=32, weight_seed=5)
    with pytest.raises(sd.EngineError, match="expects"):  # tower projects to 32, the adapter reads 48
        e.set_ip_adapter(image=img)
    e2 = _engine(sd, oracle)
    e2.ip_adapter_init(64, 32, 4, 2)
    e2.clip_vision_init(hidden=128, heads=2, layers=2, image_size=28, patch_size=14, proj=32, weight_seed=5)
    cond = np.random.default_rng(4).standard_normal((1, 77, 64)).astype(np.float32)
    base = e2.sample_latents(cond, cond * 0.5, width=64, height=64, steps=2, cfg=5.0, seed=7)
    e2.set_ip_adapter(image=img, strength=0.7)
    a = e2.sample_latents(cond, cond * 0.5, width=64, height=64, steps=2, cfg=5.0, seed=7)
    emb = e2.clip_vision_encode(e2.clip_preprocess(img), True, -1)
    e2.set_ip_adapter(tokens=e2.ip_adapter_project(emb)[0], strength=0.7)
    b = e2.sample_latents(cond, cond * 0.5, width=64, height=64, steps=2, cfg=5.0, seed=7)
    assert np.array_equal(a, b) and not np.array_equal(a, base)
    e2.set_ip_adapter(image=img, strength=0.0)
    assert np.array_equal(e2.sample_latents(cond, cond * 0.5, width=64, height=64, steps=2, cfg=5.0, seed=7), base)
    e2.set_ip_adapter()
    assert np.array_equal(e2.sample_latents(cond, cond * 0.5, width=64, height=64, steps=2, cfg=5.0, seed=7), base)


# ---------------------------------------------------------------------------------------------------- names and loaders
def test_tower_name_rule_matches_the_reference_table(sd, oracle):
    table = json.loads((ROOT / "tests" / "golden" / "clip_vision_names_ref.json").read_text())
    e = _engine(sd, oracle)
    n = 0
    for raw, ref in table["sd1"].items():
        assert ref.startswith("cond_stage_model.transformer.") or not raw.startswith("clip_vision.") or ref == raw, (raw, ref)
        # the engine keeps the tower under its own prefix: the reference's "cond_stage_model.transformer." is the text tower's here
        want = "clip_vision." + ref[len("cond_stage_model.transformer."):] if ref.startswith("cond_stage_model.transformer.") else ref
        assert e.convert_tensor_name(raw) == want, raw
        n += 1
    assert n > 90 and table["sd1"] == table["sdxl"]


def _tower_file(e, drop=None, nest_projection=False):
    """the engine's tower parameters as an HF-named file (no prefix; torch order = reversed ggml ne)"""
    out = {}
    for name in e.tensor_names():
        if not name.startswith("clip_vision.") or name == drop:
            continue
        key = name[len("clip_vision."):].replace("vision_model.pre_layernorm.", "vision_model.pre_layrnorm.")  # HF's spelling, what real tower files hold
        if nest_projection and key == "visual_projection.weight":
            key = "vision_model.visual_projection.weight"
        ne, ty, _ = e.tensor_info(name)
        shape = [d for d in reversed(ne)]
        while len(shape) > 1 and shape[0] == 1:
            shape = shape[1:]
        out[key] = ("F32", e.get_tensor(name).reshape(shape).astype(np.float32))
    return out


@pytest.mark.parametrize("nest_projection", [False, True])
def test_tower_file_round_trip(sd, oracle, tmp_path, nest_projection):
    src = _engine(sd, oracle)
    src.clip_vision_init(hidden=128, heads=2, layers=2, image_size=28, patch_size=14, proj=32, weight_seed=11)
    _write_safetensors(tmp_path / "tower.safetensors", _tower_file(src, nest_projection=nest_projection))
    dst = _engine(sd, oracle)
    r = dst.load_clip_vision(tmp_path / "tower.safetensors")
    assert (r["missing"], r["unused"]) == (0, 0) and r["loaded"] == sum(1 for n in src.tensor_names() if n.startswith("clip_vision."))
    a, b = src.clip_vision_info(), dst.clip_vision_info()
    assert {k: a[k] for k in a if k != "n_head"} == {k: b[k] for k in b if k != "n_head"}  # (heads are not in a file: hidden / 64 below the full-size towers)
    assert b["n_head"] == 2
    px = np.random.default_rng(0).standard_normal((1, 3, 28, 28)).astype(np.float32)
    assert np.array_equal(src.clip_vision_encode(px), dst.clip_vision_encode(px))
    _write_safetensors(tmp_path / "short.safetensors", _tower_file(src, drop="clip_vision.vision_model.encoder.layers.1.mlp.fc2.bias"))
    d2 = _engine(sd, oracle)
    assert d2.load_clip_vision(tmp_path / "short.safetensors")["missing"] == 1


def _adapter_file(e):
    """the engine's adapter parameters under the file names of an IP-Adapter checkpoint: image_proj.*, ip_adapter.<2 i + 1>.to_{k,v}_ip.weight"""
    out, idx = {}, {}
    for name in e.tensor_names():
        if name.startswith("ip_adapter.image_proj."):
            key = name[len("ip_adapter."):]
        elif name.endswith("to_k_ip.weight") or name.endswith("to_v_ip.weight"):
            key = None
            for i in range(1, 33, 2):
                for kv in "kv":
                    if e.convert_tensor_name(f"ip_adapter.{i}.to_{kv}_ip.weight") == name:
                        key = f"ip_adapter.{i}.to_{kv}_ip.weight"
            assert key, name
        else:
            continue
        ne, _, _ = e.tensor_info(name)
        shape = [d for d in reversed(ne)]
        while len(shape) > 1 and shape[0] == 1:
            shape = shape[1:]
        if key == "image_proj.latents":
            shape = [1] + shape  # the checkpoint's [1, num_queries, dim]
        out[key] = ("F32", e.get_tensor(name).reshape(shape).astype(np.float32))
    return out


def test_plus_and_plain_adapter_files_are_told_apart(sd, oracle, tmp_path):
    plus = _engine(sd, oracle)
    plus.ip_adapter_init_plus(64, 128, 2, 16, 160, 256, 3)
    plain = _engine(sd, oracle)
    plain.ip_adapter_init(64, 48, 4, 3)
    _write_safetensors(tmp_path / "plus.safetensors", _adapter_file(plus))
    _write_safetensors(tmp_path / "plain.safetensors", _adapter_file(plain))
    a = _engine(sd, oracle)
    r = a.load_ip_adapter(tmp_path / "plus.safetensors")
    assert (r["missing"], r["unused"]) == (0, 0), r
    assert a.ip_adapter_is_plus() and a.ip_adapter_info() == (64, 160, 16)
    for n in ("ip_adapter.image_proj.latents", "ip_adapter.image_proj.layers.1.1.3.weight", "ip_adapter.image_proj.proj_out.bias"):
        assert np.array_equal(a.get_tensor(n), plus.get_tensor(n))
    assert a.tensor_info("ip_adapter.image_proj.layers.0.1.1.weight")[0][:2] == [128, 256]
    b = _engine(sd, oracle)
    r = b.load_ip_adapter(tmp_path / "plain.safetensors")
    assert (r["missing"], r["unused"]) == (0, 0), r
    assert not b.ip_adapter_is_plus() and b.ip_adapter_info() == (64, 48, 4)
    # one tensor short
    short = _adapter_file(plus)
    del short["image_proj.layers.0.0.to_kv.weight"]
    _write_safetensors(tmp_path / "short.safetensors", short)
    c = _engine(sd, oracle)
    assert c.load_ip_adapter(tmp_path / "short.safetensors")["missing"] == 1
    # a context holds one adapter
    with pytest.raises(sd.EngineError):
        a.ip_adapter_init(64, 48, 4, 0)
    with pytest.raises(sd.EngineError):
        b.ip_adapter_init_plus(64, 128, 2, 16, 160, 256, 0)


# ---------------------------------------------------------------------------------------------------- preprocessing
def _picture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("w,h,S", [(37, 23, 28), (23, 37, 28), (224, 224, 224), (640, 480, 224), (1, 1, 28), (100, 100, 28), (10, 17, 28), (61, 28, 28)])
def test_preprocess_restatement_shapes_and_engine_host_path(sd, oracle, w, h, S):
    img = _picture(w, h, w * 1000 + h)
    ref = CV.clip_preprocess(img, S)
    assert ref.shape == (1, 3, S, S) and ref.dtype == np.float32
    xi, yi = CV.preprocess_tables(w, h, S)
    assert xi.min() >= 0 and xi.max() < w and yi.min() >= 0 and yi.max() < h and (np.diff(xi) >= 0).all() and (np.diff(yi) >= 0).all()
    if (w, h) == (S, S):
        assert np.array_equal(xi, np.arange(S)) and np.array_equal(yi, np.arange(S))  # identity indices
    # every value is (k / 255 - mean) / std for a byte k of the picture
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    for c in range(3):
        allowed = (k - CV.MEANS[c]) / CV.STDS[c]
        assert np.isin(ref[0, c], allowed).all()
    e = _engine(sd, oracle)
    got = e.clip_preprocess(img, size=S)  # the engine's host path (a backend without the kernel export)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    got3 = e.clip_preprocess(np.stack([img, img[::-1].copy(), img[:, ::-1].copy()]), size=S)
    assert np.array_equal(got3[0], ref[0]) and np.array_equal(got3[1], CV.clip_preprocess(img[::-1], S)[0]) and np.array_equal(got3[2], CV.clip_preprocess(img[:, ::-1], S)[0])


def test_preprocess_geometry_cases_differ():
    """landscape / portrait / square, upscale / downscale, odd crop offsets: what the restatement does with each"""
    S = 28
    # landscape 61 x 28: scale 1 on the height, resized width 61, crop offset (61 - 28) / 2 = 16 (odd margin 33)
    xi, yi = CV.preprocess_tables(61, 28, S)
    assert np.array_equal(yi, np.arange(28)) and np.array_equal(xi, np.arange(16, 44))
    # portrait: the transposed picture gives the transposed crop
    a = _picture(61, 28, 1)
    assert np.array_equal(CV.clip_preprocess(a.transpose(1, 0, 2), S)[0], CV.clip_preprocess(a, S)[0].transpose(0, 2, 1))
    # upscale of a 7 x 7 square by 4: every source pixel four times
    xi, yi = CV.preprocess_tables(7, 7, S)
    assert np.array_equal(xi, np.arange(28) // 4) and np.array_equal(xi, yi)
    # downscale 56 -> 28: every second pixel, starting at 0 (plain Nearest: dst * in / out)
    xi, _ = CV.preprocess_tables(56, 56, S)
    assert np.array_equal(xi, np.arange(28) * 2)
    # non-integer ratio, landscape 640 x 480 -> 224: resized 298 x 224 (truncated from 298.67), offset 37
    xi, yi = CV.preprocess_tables(640, 480, 224)
    assert xi[0] == 37 * 640 // 298 and xi[-1] == (223 + 37) * 640 // 298 and yi[-1] == 223 * 480 // 224


@pytest.mark.parametrize("mutant,w,h,S", [("ceil_offset", 61, 28, 28), ("min_ratio", 37, 23, 28), ("round_extent", 640, 480, 224), ("clamp_after", 37, 23, 28),
                                          ("swap_means", 37, 23, 28)])
def test_preprocess_mutants_change_the_output(mutant, w, h, S):
    img = _picture(w, h, 99)
    assert not np.array_equal(CV.clip_preprocess(img, S, mutant=mutant), CV.clip_preprocess(img, S)), mutant
