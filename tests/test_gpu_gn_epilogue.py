"""GroupNorm statistics from the producing conv's epilogue (option fuse_gn_epilogue, counter fused_gn_epilogue).

An unsplit conv whose result a GroupNorm reads (directly, or through a skip CONCAT) writes per-channel (mean, M2) records of the values it stores
(GnRec side band: epi_conv_gn in k_conv3w and in the conv-mode 256-row tiles of k_gemm16); k_gn_finalize turns the records into the GroupNorm's
scale / shift tables, and the statistics pass over the tensor is not run.  Every case compares the whole graph with the CPU oracle at the bar the
project's GroupNorm-into-conv tests use (rel-L2 < 3e-4) and asserts how far the counter moved.  The oracle result of a case is computed once and shared.

Shapes are the smallest that land on the intended kernel (checked with the window_convs / split_k_gemms counters where they tell):
  * 3x3, 64 -> 256 / 320 channels on 48 images of 32 x 32: 192 tiles of 256 positions, the least conv3w_plan leaves unsplit; four chunks per image;
  * 1x1 conv-mode launches: 32768 rows x 320 columns take the 8-wave 256 x 160 tile (eight wave rows of one row block), 49152 rows x 320 columns with
    K = 512 the 256 x 320 tile, 32768 rows x 640 columns the 4-wave 256 x 160 tile, 49152 rows x 256 columns with K = 2048 the pipelined 256 x 256 tile;
    256 columns below that run on 128-column tiles (256 x 128 or 128 x 128), which fill no side band (fall-back).
"""
import os

import numpy as np
import pytest

from ggml_graph import F16, F32, Graph
from test_gpu_ops import _on_gpu, rel_l2

pytestmark = pytest.mark.gpu

BAR = 3e-4
_oracle_cache = {}


def _run(sd, dev, build):
    with Graph(dev) as g:
        return g.run(build(g, sd.lib()))


def _oracle(sd, oracle, key, build):
    if key not in _oracle_cache:
        _oracle_cache[key] = _run(sd, oracle, build)
        _oracle_cache[key].setflags(write=False)
    return _oracle_cache[key]


def _stats(sd):
    return sd.backend_stats() if _on_gpu() else None


def _check_counters(sd, before, **deltas):
    """asserts how far each named counter moved since `before` (not under SDCPP_BACKEND_OPTS: the session's options change the plans)"""
    if before is None or os.environ.get("SDCPP_BACKEND_OPTS"):
        return
    st = sd.backend_stats()
    for name, want in deltas.items():
        got = st[name] - before[name]
        print(f"{name}: +{got}")
        if isinstance(want, str):  # ">=1"
            assert got >= int(want[2:]), (name, got, want)
        else:
            assert got == want, (name, got, want)


def _affine(g, L, t, w, b, C):
    t = L.ggml_mul_inplace(g.ctx, t, L.ggml_reshape_4d(g.ctx, g.weight(w, F32), 1, 1, C, 1))
    return L.ggml_add_inplace(g.ctx, t, L.ggml_reshape_4d(g.ctx, g.weight(b, F32), 1, 1, C, 1))


def _window_conv_case(OC, extra, N=48, IC=64, HW=32):
    """3x3 conv IC -> OC (+bias) [+ time-embedding add] [+ residual of mean 5.0, sigma 1.5] -> GroupNorm(32) -> affine -> SiLU -> 1x1 conv, plus a later ADD of
    the conv result: both the stored values and the normalised branch reach the output"""
    rng = np.random.default_rng(20 + OC + 7 * len(extra))
    x = rng.standard_normal((N, IC, HW, HW)).astype(np.float32)
    w = (rng.standard_normal((OC, IC, 3, 3)) / np.sqrt(IC * 9)).astype(np.float32)
    b = rng.standard_normal(OC).astype(np.float32)
    r = (rng.standard_normal((N, OC, HW, HW)) * 1.5 + 5.0).astype(np.float32)
    emb = rng.standard_normal((N, 128)).astype(np.float32)
    we = (rng.standard_normal((OC, 128)) / np.sqrt(128)).astype(np.float32)
    be = rng.standard_normal(OC).astype(np.float32)
    gw = (1 + 0.1 * rng.standard_normal(OC)).astype(np.float32)
    gb = rng.standard_normal(OC).astype(np.float32)
    w2 = (rng.standard_normal((OC, OC, 1, 1)) / np.sqrt(OC)).astype(np.float32)

    def build(g, L):
        h = L.ggml_conv_2d(g.ctx, g.weight(w, F16), g.input(x), 1, 1, 1, 1, 1, 1)
        h = L.ggml_add_inplace(g.ctx, h, L.ggml_reshape_4d(g.ctx, g.weight(b, F32), 1, 1, OC, 1))
        if "emb" in extra:
            e = L.ggml_mul_mat(g.ctx, g.weight(we, F16), L.ggml_silu(g.ctx, g.input(emb)))
            e = L.ggml_add_inplace(g.ctx, e, g.weight(be, F32))
            h = L.ggml_add(g.ctx, h, L.ggml_reshape_4d(g.ctx, e, 1, 1, OC, N))
        if "res" in extra:
            h = L.ggml_add(g.ctx, h, g.input(r))
        t = L.ggml_group_norm(g.ctx, h, 32, 1e-6)
        t = L.ggml_silu_inplace(g.ctx, _affine(g, L, t, gw, gb, OC))
        t = L.ggml_conv_2d(g.ctx, g.weight(w2, F16), t, 1, 1, 0, 0, 1, 1)
        return L.ggml_add(g.ctx, t, h)

    return build, (N, OC, HW, HW)


@pytest.mark.parametrize("OC", [256, 320])
def test_unsplit_window_conv_writes_group_norm_records(sd, oracle, gpu, OC):
    """k_conv3w, both column tiles: four 256-position chunks per image to merge; with 320 channels a group has 10 — groups cut through the 32-channel blocks
    and the 16-channel register sets of a lane"""
    build, shape = _window_conv_case(OC, ())
    ref = _oracle(sd, oracle, ("window", OC, ()), build)
    before = _stats(sd)
    out = _run(sd, gpu, build)
    err = rel_l2(out, ref)
    print(f"OC={OC}: rel-L2 vs oracle {err:.3e}")
    assert out.shape == shape and np.isfinite(out).all()
    assert err < BAR
    _check_counters(sd, before, window_convs=1, fused_gn_epilogue=1)


@pytest.mark.parametrize("extra,fused", [(("res",), 1), (("emb",), 1), (("emb", "res"), 0)])
def test_window_conv_records_with_residual_far_from_zero_and_embedding_add(sd, oracle, gpu, extra, fused):
    """The records describe exactly the value stored: + residual (mean 5.0, sigma 1.5 — the per-chunk numbers must not cancel) and + the time-embedding add.
    A conv epilogue takes ONE of the two ADDs (plan_conv_chain: the embedding add, else the residual); with both in the graph the residual ADD runs as
    its own launch, the GroupNorm reads that launch's result and keeps its statistics pass — the counter stays, the result is the oracle's all the same."""
    build, shape = _window_conv_case(320, extra)
    ref = _oracle(sd, oracle, ("window", 320, extra), build)
    before = _stats(sd)
    out = _run(sd, gpu, build)
    err = rel_l2(out, ref)
    print(f"{'+'.join(extra)}: rel-L2 vs oracle {err:.3e}")
    assert out.shape == shape and np.isfinite(out).all()
    assert err < BAR
    _check_counters(sd, before, window_convs=1, fused_gn_epilogue=fused, fused_chan_add=1 if "emb" in extra else 0)


@pytest.mark.parametrize("N,C,inner,fused", [(32, 320, 320, 1), (48, 320, 512, 1), (48, 256, 2048, 1), (32, 256, 256, 0)])
def test_token_linear_into_nchw_residual_writes_group_norm_records(sd, oracle, gpu, N, C, inner, fused):
    """proj_out Linear on tokens -> NCHW + bias + residual (one conv-mode 1x1 launch, the graph of test_token_linear_into_nchw_residual) -> GroupNorm -> conv on
    32 x 32 maps (1024 positions: four whole 256-row tiles per image).  320 columns: the 8-wave 256 x 160 tile (K = 320) and the 256 x 320 tile (K = 512); 256
    columns: the pipelined 256 x 256 tile (K = 2048), and below it a 128-column tile, which writes no records (fall-back, counter unchanged)"""
    H = W = 32
    rng = np.random.default_rng(300 + N + C + inner)
    t = rng.standard_normal((N, H * W, inner)).astype(np.float32)
    xin = (rng.standard_normal((N, C, H, W)) * 1.5 + 2.0).astype(np.float32)
    wl = (rng.standard_normal((C, inner)) / np.sqrt(inner)).astype(np.float32)
    bl = rng.standard_normal(C).astype(np.float32)
    gw = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    gb = rng.standard_normal(C).astype(np.float32)
    w2 = (rng.standard_normal((64, C, 1, 1)) / np.sqrt(C)).astype(np.float32)

    def build(g, L):
        y = L.ggml_mul_mat(g.ctx, g.weight(wl, F16), g.input(t))
        y = L.ggml_add_inplace(g.ctx, y, g.weight(bl, F32))
        y = L.ggml_cont(g.ctx, L.ggml_permute(g.ctx, y, 1, 0, 2, 3))
        y = L.ggml_reshape_4d(g.ctx, y, W, H, C, N)
        h = L.ggml_add(g.ctx, y, g.input(xin))
        u = L.ggml_group_norm(g.ctx, h, 32, 1e-6)
        u = L.ggml_silu_inplace(g.ctx, _affine(g, L, u, gw, gb, C))
        return L.ggml_conv_2d(g.ctx, g.weight(w2, F16), u, 1, 1, 0, 0, 1, 1)

    ref = _oracle(sd, oracle, ("proj", N, C, inner), build)
    before = _stats(sd)
    out = _run(sd, gpu, build)
    err = rel_l2(out, ref)
    print(f"N={N} C={C} K={inner}: rel-L2 vs oracle {err:.3e}")
    assert out.shape == (N, 64, H, W) and np.isfinite(out).all()
    assert err < BAR
    _check_counters(sd, before, fused_proj_tokens=">=1", fused_gn_epilogue=fused)


@pytest.mark.parametrize("b_is_input", [False, True])
def test_skip_concat_group_norm_from_the_records_of_two_convs(sd, oracle, gpu, b_is_input):
    """CONCAT(conv_a(x) [640 channels], conv_b(y) [320]) -> GroupNorm(32) -> affine -> SiLU -> 3x3 conv, + the skip 1x1 conv on the concatenation: the graph of
    test_skip_concat_group_norm_two_sources with conv-produced sources at 16 x 16 (one 256-position chunk per image).  960 channels at 30 per group: groups 21
    and 22 straddle the two sources, whose means differ.  The sources are 1x1 convs on 128 images: 32768 rows x 640 columns take the 4-wave 256 x 160 tile,
    x 320 columns the 8-wave one.  With a plain graph input as second source there are no records for it: the two-source statistics pass stays."""
    N, Ca, Cb, HW, IC = 128, 640, 320, 16, 64
    C = Ca + Cb
    rng = np.random.default_rng(77)
    x = (rng.standard_normal((N, IC, HW, HW)) * 1.3).astype(np.float32)
    y = (rng.standard_normal((N, IC, HW, HW)) * 0.7).astype(np.float32)
    wa = (rng.standard_normal((Ca, IC, 1, 1)) / np.sqrt(IC)).astype(np.float32)
    ba = (rng.standard_normal(Ca) + 1.5).astype(np.float32)
    wb = (rng.standard_normal((Cb, IC, 1, 1)) / np.sqrt(IC)).astype(np.float32)
    bb = (rng.standard_normal(Cb) - 1.5).astype(np.float32)
    b_in = (rng.standard_normal((N, Cb, HW, HW)) * 0.7 - 1.5).astype(np.float32)
    gw = (1 + 0.1 * rng.standard_normal(C)).astype(np.float32)
    gb = rng.standard_normal(C).astype(np.float32)
    OC = 32
    wc = (rng.standard_normal((OC, C, 3, 3)) / np.sqrt(C * 9)).astype(np.float32)
    ws = (rng.standard_normal((OC, C, 1, 1)) / np.sqrt(C)).astype(np.float32)

    def build(g, L):
        a = L.ggml_conv_2d(g.ctx, g.weight(wa, F16), g.input(x), 1, 1, 0, 0, 1, 1)
        a = L.ggml_add_inplace(g.ctx, a, L.ggml_reshape_4d(g.ctx, g.weight(ba, F32), 1, 1, Ca, 1))
        if b_is_input:
            b = g.input(b_in)
        else:
            b = L.ggml_conv_2d(g.ctx, g.weight(wb, F16), g.input(y), 1, 1, 0, 0, 1, 1)
            b = L.ggml_add_inplace(g.ctx, b, L.ggml_reshape_4d(g.ctx, g.weight(bb, F32), 1, 1, Cb, 1))
        h = L.ggml_concat(g.ctx, a, b, 2)
        t = L.ggml_group_norm(g.ctx, h, 32, 1e-6)
        t = L.ggml_silu_inplace(g.ctx, _affine(g, L, t, gw, gb, C))
        o = L.ggml_conv_2d(g.ctx, g.weight(wc, F16), t, 1, 1, 1, 1, 1, 1)
        sk = L.ggml_conv_2d(g.ctx, g.weight(ws, F16), h, 1, 1, 0, 0, 1, 1)
        return L.ggml_add(g.ctx, o, sk)

    ref = _oracle(sd, oracle, ("concat", b_is_input), build)
    before = _stats(sd)
    out = _run(sd, gpu, build)
    err = rel_l2(out, ref)
    print(f"second source {'graph input' if b_is_input else 'conv'}: rel-L2 vs oracle {err:.3e}")
    assert out.shape == (N, OC, HW, HW) and np.isfinite(out).all()
    assert err < BAR
    _check_counters(sd, before, fused_concat_gn=1, fused_gn_epilogue=0 if b_is_input else 1)


def test_tiles_straddling_images_keep_the_statistics_pass(sd, oracle, gpu):
    """conv output 24 x 24 = 576 positions per image: a 256-row tile would straddle images, no side band is registered, the GroupNorm runs its own pass"""
    N, IC, OC, HW = 16, 64, 320, 24
    rng = np.random.default_rng(576)
    x = rng.standard_normal((N, IC, HW, HW)).astype(np.float32)
    w = (rng.standard_normal((OC, IC, 3, 3)) / np.sqrt(IC * 9)).astype(np.float32)
    b = (rng.standard_normal(OC) + 2.0).astype(np.float32)
    gw = (1 + 0.1 * rng.standard_normal(OC)).astype(np.float32)
    gb = rng.standard_normal(OC).astype(np.float32)
    w2 = (rng.standard_normal((64, OC, 1, 1)) / np.sqrt(OC)).astype(np.float32)

    def build(g, L):
        h = L.ggml_conv_2d(g.ctx, g.weight(w, F16), g.input(x), 1, 1, 1, 1, 1, 1)
        h = L.ggml_add_inplace(g.ctx, h, L.ggml_reshape_4d(g.ctx, g.weight(b, F32), 1, 1, OC, 1))
        t = L.ggml_group_norm(g.ctx, h, 32, 1e-6)
        t = L.ggml_silu_inplace(g.ctx, _affine(g, L, t, gw, gb, OC))
        return L.ggml_conv_2d(g.ctx, g.weight(w2, F16), t, 1, 1, 0, 0, 1, 1)

    ref = _oracle(sd, oracle, ("straddle",), build)
    before = _stats(sd)
    out = _run(sd, gpu, build)
    err = rel_l2(out, ref)
    print(f"24 x 24: rel-L2 vs oracle {err:.3e}")
    assert np.isfinite(out).all() and err < BAR
    _check_counters(sd, before, fused_gn_epilogue=0, fused_norm=">=1")


def test_records_are_deterministic_and_the_option_restores_the_pass(sd, oracle, gpu):
    """every merge order is fixed (no atomics): two runs agree bit for bit; fuse_gn_epilogue = 0 plans the statistics pass again, within the oracle bar"""
    build, _ = _window_conv_case(256, ())
    ref = _oracle(sd, oracle, ("window", 256, ()), build)
    before = _stats(sd)
    a = _run(sd, gpu, build)
    b = _run(sd, gpu, build)
    assert np.array_equal(a, b)
    assert rel_l2(a, ref) < BAR
    _check_counters(sd, before, fused_gn_epilogue=">=1")  # (once per plan built: the second run may come out of the plan cache)
    if not _on_gpu():
        return
    try:
        sd.backend_set_option("fuse_gn_epilogue", 0)
        before = _stats(sd)
        c = _run(sd, gpu, build)
        print(f"fuse_gn_epilogue=0: rel-L2 vs oracle {rel_l2(c, ref):.3e}, vs the default plan {rel_l2(c, a):.3e}")
        assert rel_l2(c, ref) < BAR and rel_l2(c, a) < BAR
        _check_counters(sd, before, fused_gn_epilogue=0, window_convs=1)
    finally:
        sd.backend_set_option("fuse_gn_epilogue", 1)
