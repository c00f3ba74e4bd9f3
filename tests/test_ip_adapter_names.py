"""The engine's IP-Adapter name rule (csrc/host/name_conversion.hpp ip_adapter_to_ldm) against the table the reference's own converter produced
(tests/golden/ip_adapter_names_ref.json, made by tests/golden/make_ip_adapter_names_golden.py), entry by entry, and against the adapter's parameters."""
import json
from pathlib import Path

import numpy as np
import pytest

from test_model_io import _write_safetensors

GOLDEN = Path(__file__).resolve().parent / "golden" / "ip_adapter_names_ref.json"


@pytest.mark.parametrize("family,model", [("sd1", "SD15_TINY"), ("sdxl", "SDXL_TINY")])
def test_ip_adapter_names_match_the_reference_table(sd, oracle, family, model):
    table = json.loads(GOLDEN.read_text())[family]
    assert len(table) >= 2 * 73 + 4 + 10
    e = sd.Engine(model=getattr(sd, model), backend=oracle)
    for raw, want in table.items():
        assert e.convert_tensor_name(raw) == want, raw
    regular = [f"ip_adapter.{i}.to_{kv}_ip.weight" for i in range(73) for kv in "kv"]
    moved = sum(table[r] != r for r in regular)
    assert moved == 2 * (16 if family == "sd1" else 36)    # SD1.x: all 16 cross-attentions (odd indices 1 .. 31); SDXL: the first 36 of its 70 lie below index 73
    assert all(table[f"image_proj.{m}.{p}"] == f"ip_adapter.image_proj.{m}.{p}" for m in ("proj", "norm") for p in ("weight", "bias"))


def test_full_size_table_covers_every_attn2(sd, oracle):
    """SD1.x: the 16 converted names are exactly the attn2 of the full-size UNet's 16 transformer blocks (the tiny model has the same block numbering)"""
    table = json.loads(GOLDEN.read_text())["sd1"]
    got = sorted(v for r, v in table.items() if r.endswith("to_k_ip.weight") and v != r)
    e = sd.Engine(model=sd.SD15_TINY, backend=oracle)
    e.ip_adapter_init(32, 48, 4)
    have = sorted(n for n in e.tensor_names() if n.endswith("attn2.to_k_ip.weight"))
    assert got == have


@pytest.mark.parametrize("model,n_blocks", [("SD15_TINY", 16), ("SDXL_TINY", None)])
def test_adapter_file_loads(sd, oracle, tmp_path, model, n_blocks):
    """a synthetic safetensors adapter in the file dialect (diffusers processor indices, torch [out, in] shapes) loads into a context that has no adapter yet: the
    dimensions come from the file, nothing is missing or unused, every value arrives (f16-representable values: the f16 parameters hold them exactly), and the
    resident weights do not move"""
    e = sd.Engine(model=getattr(sd, model), backend=oracle)
    table = json.loads(GOLDEN.read_text())["sd1" if model == "SD15_TINY" else "sdxl"]
    attn2 = {n[:-len("to_k.weight")]: e.tensor_info(n)[0][1] for n in e.tensor_names() if n.endswith("attn2.to_k.weight")}
    idx_of = {}                               # block prefix -> the file's processor index, through the converter (held to the reference's table above, and to it here)
    for i in range(1, 140, 2):                # SDXL: 70 transformer blocks, indices 1 .. 139
        raw = f"ip_adapter.{i}.to_k_ip.weight"
        conv = e.convert_tensor_name(raw)
        assert conv != raw and table.get(raw, conv) == conv
        idx_of[conv[:-len("to_k_ip.weight")]] = str(i)
        if model == "SD15_TINY" and i == 31:
            break
    assert set(attn2) <= set(idx_of)          # the tiny models number their blocks as the full-size ones do
    if n_blocks:
        assert len(attn2) == n_blocks
    rng = np.random.default_rng(4)
    ip_dim, clip_dim, n_tok = 24, 40, 4
    f16 = lambda *shape: rng.standard_normal(shape).astype(np.float16).astype(np.float32)
    tensors, want = {}, {}
    for prefix, inner in attn2.items():
        for kv in "kv":
            w = f16(inner, ip_dim)
            tensors[f"ip_adapter.{idx_of[prefix]}.to_{kv}_ip.weight"] = ("F32", w)
            want[f"{prefix}to_{kv}_ip.weight"] = w
    for nm, arr in (("proj.weight", f16(n_tok * ip_dim, clip_dim)), ("proj.bias", f16(n_tok * ip_dim)), ("norm.weight", f16(ip_dim)), ("norm.bias", f16(ip_dim))):
        tensors["image_proj." + nm] = ("F32", arr)
        want["ip_adapter.image_proj." + nm] = arr
    path = tmp_path / "adapter.safetensors"
    _write_safetensors(path, tensors)
    probe = next(n for n in e.tensor_names() if n.endswith("attn2.to_k.weight"))
    before = e.get_tensor(probe)
    assert e.ip_adapter_info() is None
    r = e.load_ip_adapter(path)
    assert r == {"loaded": len(tensors), "missing": 0, "unused": 0}
    assert e.ip_adapter_info() == (ip_dim, clip_dim, n_tok)
    for name, arr in want.items():
        np.testing.assert_array_equal(e.get_tensor(name).reshape(arr.shape), arr)
    np.testing.assert_array_equal(e.get_tensor(probe), before)
    with pytest.raises(sd.EngineError, match="other dimensions"):     # a second file with other shapes is refused, the loaded adapter stays
        tensors2 = {k: (dt, np.zeros((a.shape[0], ip_dim + 8), np.float32) if k.endswith("_ip.weight") else a) for k, (dt, a) in tensors.items()}
        tensors2["image_proj.norm.weight"] = ("F32", np.zeros(ip_dim + 8, np.float32))
        tensors2["image_proj.norm.bias"] = ("F32", np.zeros(ip_dim + 8, np.float32))
        tensors2["image_proj.proj.weight"] = ("F32", np.zeros((n_tok * (ip_dim + 8), clip_dim), np.float32))
        tensors2["image_proj.proj.bias"] = ("F32", np.zeros(n_tok * (ip_dim + 8), np.float32))
        _write_safetensors(tmp_path / "other.safetensors", tensors2)
        e.load_ip_adapter(tmp_path / "other.safetensors")
    dit = sd.Engine(model=sd.SD35_TINY, backend=oracle)
    with pytest.raises(sd.EngineError, match="UNet families"):
        dit.load_ip_adapter(path)
