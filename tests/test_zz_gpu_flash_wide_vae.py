"""The KL-VAE mid-block attention (one head of d = 512) through the public interface: Engine(flash_attn=True) emits the FLASH_ATTN_EXT node, which k_flash_wide
claims; Engine(flash_attn=False) keeps the manual chain on the GEMM composition.  Full-width SD1.5 VAE (the *_TINY mid-blocks are 128 wide: k_flash_attn's range) at
8 x 8 and 16 x 16 latents = 64 / 256 positions.  Bar: rel-L2 between the two GPU engines below twice the rel-L2 between the flash_attn=False GPU result and the
oracle's result for the same call (measured here, printed)."""
import os

import numpy as np
import pytest

from attn_scores import rel_l2

pytestmark = pytest.mark.gpu

ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"


@pytest.fixture(scope="module")
def engines(sd, oracle, gpu):
    return [sd.Engine(model=sd.SD15, backend=gpu, flash_attn=True), sd.Engine(model=sd.SD15, backend=gpu, flash_attn=False), sd.Engine(model=sd.SD15, backend=oracle, flash_attn=False)]


@pytest.mark.parametrize("lat", [8, 16])
@pytest.mark.parametrize("call", ["decode", "encode"])
def test_vae_mid_attention_takes_the_wide_kernel(sd, engines, call, lat):
    rng = np.random.default_rng([lat, call == "encode"])
    x = (rng.standard_normal((2, 4, lat, lat)) * 0.5 if call == "decode" else rng.random((2, 3, lat * 8, lat * 8))).astype(np.float32)
    outs, wide = [], []
    for e in engines:
        before = sd.backend_stats()["flash_wide_launches"] if ON_GPU else 0
        outs.append(e.vae_decode(x, raw=True) if call == "decode" else e.vae_encode(x, seed=3, return_moments=True)[1])
        wide.append(sd.backend_stats()["flash_wide_launches"] - before if ON_GPU else 0)
    flash, plain, ref = outs
    own, err = rel_l2(plain, ref), rel_l2(flash, plain)
    print(f"[flash-wide vae] {call} latent {lat}x{lat}: flash vs GEMM composition {err:.3e}; GEMM composition vs oracle {own:.3e}; wide launches {wide}")
    assert np.isfinite(flash).all()
    if ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS"):
        assert wide[0] >= 1 and wide[1] == 0 and wide[2] == 0
    assert err < 2.0 * own or not ON_GPU
