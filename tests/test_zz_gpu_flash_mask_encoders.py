"""The causal attention of the CLIP text tower through the public interface: Engine(flash_attn=True).clip_forward emits FLASH_ATTN_EXT with the f16 causal mask,
which k_flash_mask claims; Engine(flash_attn=False) keeps the manual MUL_MAT -> SCALE -> ADD(mask) -> SOFT_MAX -> MUL_MAT chain.  Full-width SD1.5: its tower is the
real ViT-L (768 wide, 12 heads of 64, 12 layers, 77 tokens) — the *_TINY towers have heads of 16 and never reach the kernel.  Bar: rel-L2 between the two engines
< 3e-3, what tests/test_text_encoders.py holds for f16 weights.  (No T5 leg: the only T5 at real head width is T5-XXL, 4.7 G parameters.)"""
import os

import numpy as np
import pytest

from attn_scores import rel_l2

pytestmark = pytest.mark.gpu

ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
LAYERS, BOS, EOS = 12, 49406, 49407


@pytest.fixture(scope="module")
def engines(sd, gpu):
    return [sd.Engine(model=sd.SD15, backend=gpu, flash_attn=True), sd.Engine(model=sd.SD15, backend=gpu, flash_attn=False)]


@pytest.mark.parametrize("n_words", [9, 75])
def test_clip_l_causal_attention_takes_the_masked_flash_kernel(sd, engines, n_words):
    rng = np.random.default_rng(n_words)
    ids = np.full(77, EOS, dtype=np.int32)
    ids[0] = BOS
    ids[1:1 + n_words] = rng.integers(1, BOS - 1, n_words)
    outs, masked = [], []
    for e in engines:
        before = sd.backend_stats()["flash_mask_launches"] if ON_GPU else 0
        outs.append(e.clip_forward(0, ids))
        masked.append(sd.backend_stats()["flash_mask_launches"] - before if ON_GPU else 0)
    err = rel_l2(outs[0], outs[1])
    print(f"[flash-mask clip] {n_words} words: flash vs manual chain {err:.3e}; masked launches {masked}")
    assert np.isfinite(outs[0]).all()
    if ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS"):
        assert masked == [LAYERS, 0]
    assert err < 3e-3
