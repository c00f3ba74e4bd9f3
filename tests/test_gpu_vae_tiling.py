"""VAE tiling on the MI355X backend: the device merge against the numpy restatement bit for bit (tile_batch = 1: every tile runs the plan of the one-tile
call), batched tiles against the oracle backend's tiled result, the fused merge kernel (k_tile_merge, option fuse_tile_merge) against the plain MUL / MUL /
ADD-in-place nodes bit for bit, plan reuse and hipGraph replay of the tile graph, and the canvas under GGML_MI355X_POISON=1."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import vae_tiling_ref as ref

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
TILE = dict(tile_size_x=8, tile_size_y=8, target_overlap=0.5)


def psnr(a, b):
    mse = float(np.mean((a.astype(np.float64) - b) ** 2))
    return 10 * np.log10(1.0 / max(mse, 1e-20))


@pytest.fixture(scope="module")
def engines(sd, oracle, gpu):
    return {name: (sd.Engine(model=getattr(sd, name), backend=gpu), sd.Engine(model=getattr(sd, name), backend=oracle)) for name in ("SD15_TINY", "SD35_TINY")}


def latent(name, w, h, n):
    ch, scale = (4, 0.18215) if name == "SD15_TINY" else (16, 1.5305)
    return (np.random.default_rng(w * 31 + h + n).standard_normal((n, ch, h, w)) * scale * 2).astype(np.float32)


def numpy_driver_decode(sd, e, z):
    """crop in numpy, decode each crop through the same engine as ONE tile (the raw decoder output), merge in numpy"""
    p = sd.tiling_plan(z.shape[3], z.shape[2], **TILE)

    def one(crop):
        e.set_vae_tiling(True, tile_size_x=crop.shape[3], tile_size_y=crop.shape[2], target_overlap=0.0, tile_batch=1)
        return e.vae_decode(crop, raw=True)
    return ref.tiled(z, one, p, decode=True, out_channels=3), p


@pytest.mark.parametrize("name,w,h,n", [("SD15_TINY", 19, 17, 1), ("SD15_TINY", 20, 14, 2), ("SD35_TINY", 19, 17, 1), ("SD35_TINY", 20, 14, 2)])
def test_merge_exact_and_batches_match_oracle(sd, engines, name, w, h, n):
    g, o = engines[name]
    z = latent(name, w, h, n)
    try:
        want, p = numpy_driver_decode(sd, g, z)
        g.set_vae_tiling(True, tile_batch=1, **TILE)
        got = g.vae_decode(z, raw=True)
        assert np.isfinite(got).all() and len(p["tiles"]) >= 6
        np.testing.assert_array_equal(got, want)
        o.set_vae_tiling(True, **TILE)
        oracle_rgb = o.vae_decode(z)
        for tb in (3, 0):
            g.set_vae_tiling(True, tile_batch=tb, **TILE)
            rgb = g.vae_decode(z)
            v = psnr(rgb, oracle_rgb)
            print(f"{name} {w}x{h} n={n} tile_batch={tb}: PSNR vs the oracle's tiled decode {v:.1f} dB")
            assert np.isfinite(rgb).all() and v > 35.0
    finally:
        g.set_vae_tiling(False)
        o.set_vae_tiling(False)


def _merge_routes(s0, s1):
    """launches of k_tile_merge<4> and k_tile_merge<1> between two statistics snapshots"""
    return s1["ew_tile_merge_v4"] - s0["ew_tile_merge_v4"], s1["ew_tile_merge_v1"] - s0["ew_tile_merge_v1"]


def _fusion_ab(sd, run, n_batches, route=None):
    """route: "v4" = every merge launch takes the float4 kernel, "v1" = at least one takes the scalar kernel (asserted with the fused merge on)"""
    out, launched, fused = {}, {}, {}
    for on in (0, 1):
        if ON_GPU:
            sd.backend_set_option("fuse_tile_merge", on)
            s0 = sd.backend_stats()
        out[on] = run()
        if ON_GPU:
            s1 = sd.backend_stats()
            launched[on] = s1["kernels_launched"] - s0["kernels_launched"]
            fused[on] = s1["fused_tile_merge"] - s0["fused_tile_merge"]
            v4, v1 = _merge_routes(s0, s1)
            if not os.environ.get("SDCPP_BACKEND_OPTS"):
                assert (v4, v1) == (0, 0) if not on else (v4 > 0 and v1 == 0) if route == "v4" else v1 > 0 if route == "v1" else True, (on, route, v4, v1)
    np.testing.assert_array_equal(out[0], out[1])
    if ON_GPU:
        print(f"kernels launched: plain {launched[0]}, fused {launched[1]}; fused merges planned {fused[1]} for {n_batches} tile batches")
        assert fused[0] == 0 and fused[1] == n_batches
        assert launched[1] < launched[0]
    return out[1]


def test_fused_merge_decode(sd, engines):
    g, _ = engines["SD15_TINY"]
    z = latent("SD15_TINY", 19, 17, 2)
    p = sd.tiling_plan(19, 17, **TILE)
    try:
        g.set_vae_tiling(True, tile_batch=4, **TILE)
        # decode geometry: positions and skips are multiples of 8 pixels, every launch takes k_tile_merge<4>
        _fusion_ab(sd, lambda: g.vae_decode(z, raw=True), -(-len(p["tiles"]) // 4), route="v4")
        # overlap 0 in both axes: the store path (CPY), 16 x 16 latent in four tiles, two per batch
        g.set_vae_tiling(True, tile_size_x=8, tile_size_y=8, target_overlap=0.0, tile_batch=2)
        q = sd.tiling_plan(16, 16, tile_size_x=8, tile_size_y=8, target_overlap=0.0)
        assert q["overlap"] == (0, 0) and len(q["tiles"]) == 4
        _fusion_ab(sd, lambda: g.vae_decode(latent("SD15_TINY", 16, 16, 1), raw=True), 2, route="v4")
    finally:
        if ON_GPU:
            sd.backend_set_option("fuse_tile_merge", 1)
        g.set_vae_tiling(False)


def test_fused_merge_encode_odd_offsets(sd, engines):
    """encode merges at latent resolution: odd positions and skips, the scalar path of the kernel"""
    g, o = engines["SD15_TINY"]
    img = np.random.default_rng(12).random((1, 3, 152, 136)).astype(np.float32)
    kw = dict(tile_size_x=4, tile_size_y=4, target_overlap=0.5)
    p = sd.tiling_plan(17, 19, encode_factor=2.0, **kw)
    assert any(t[0] % 2 or t[1] % 2 for t in p["tiles"]) and any(t[2] or t[3] for t in p["tiles"])
    try:
        g.set_vae_tiling(True, tile_batch=3, **kw)
        mom = _fusion_ab(sd, lambda: g.vae_encode(img, seed=4, return_moments=True)[1], -(-len(p["tiles"]) // 3), route="v1")
        o.set_vae_tiling(True, **kw)
        want = o.vae_encode(img, seed=4, return_moments=True)[1]
        err = float(np.linalg.norm((mom - want).astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))
        print(f"tiled encode moments vs the oracle's: rel-L2 {err:.2e}")
        assert np.isfinite(mom).all() and err < 5e-3   # the per-forward bar of tests/test_gpu_model.py
        # the identity in place of the model: the merge alone, bit for bit against numpy, at odd sizes (scalar path), at multiples of 4 (float4 path), and at the
        # float4 path's near miss: a canvas and tiles of multiples of 4 cells with one tile per batch at x = 0, 6, 12 (the middle batch has bx % 4 != 0)
        for (w, h, tx, ty, ov, tb, route) in ((19, 17, 8, 8, 0.3, 3, "v1"), (11, 9, 8, 4, 0.25, 2, "v1"), (64, 40, 32, 32, 0.5, 4, "v4"), (8, 8, 4, 4, 0.0, 3, None),
                                              (20, 8, 8, 8, 0.25, 1, "v1+v4")):
            x = np.random.default_rng(w + h).standard_normal((2, 3, h, w)).astype(np.float32)
            g.set_vae_tiling(True, tile_size_x=tx, tile_size_y=ty, target_overlap=ov, tile_batch=tb)
            q = sd.tiling_plan(w, h, tile_size_x=tx, tile_size_y=ty, target_overlap=ov)
            canvas = np.zeros_like(x)
            for (px, py, dx, dy) in q["tiles"]:
                ref.merge(canvas, x[:, :, py:py + q["tile_size"][1], px:px + q["tile_size"][0]], px, py, q["overlap"][0], q["overlap"][1], dx, dy)
            s0 = sd.backend_stats() if ON_GPU else None
            np.testing.assert_array_equal(g.tiling_blend(x), canvas)
            if ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS"):
                v4, v1 = _merge_routes(s0, sd.backend_stats())
                print(f"blend {w}x{h} tiles {tx}x{ty} batch {tb}: k_tile_merge<4> launches {v4}, k_tile_merge<1> launches {v1}")
                if route == "v1":
                    assert v4 == 0 and v1 > 0
                elif route == "v4":
                    assert v4 > 0 and v1 == 0
                elif route == "v1+v4":
                    assert [t[0] for t in q["tiles"]] == [0, 6, 12] and v1 > 0 and v4 > 0
    finally:
        if ON_GPU:
            sd.backend_set_option("fuse_tile_merge", 1)
        g.set_vae_tiling(False)
        o.set_vae_tiling(False)


def test_tile_graph_is_one_topology(sd, engines):
    g, _ = engines["SD15_TINY"]
    z = latent("SD15_TINY", 20, 19, 1)
    p = sd.tiling_plan(20, 19, **TILE)
    T = len(p["tiles"])
    assert T == 12
    try:
        g.set_vae_tiling(True, tile_batch=5, **TILE)   # two full batches + a short one
        n_batches = -(-T // 5)
        if ON_GPU:
            sd.backend_set_option("fuse_tile_merge", 1)   # (drops cached plans: the first call below plans everything)
            s0 = sd.backend_stats()
        a = g.vae_decode(z, raw=True)
        if ON_GPU:
            s1 = sd.backend_stats()
        b = g.vae_decode(z, raw=True)
        np.testing.assert_array_equal(a, b)
        if ON_GPU:
            s2 = sd.backend_stats()
            first, second = s1["plans_built"] - s0["plans_built"], s2["plans_built"] - s1["plans_built"]
            print(f"{T} tiles in {n_batches} batches: plans built {first} then {second}, graph replays {s2['graph_replays'] - s0['graph_replays']}")
            # one plan for every full tile batch, one for the short last batch, one merge plan per batch (the positions are theirs); nothing new the second time
            assert first <= 2 + n_batches and second == 0
            assert s2["graph_replays"] > s0["graph_replays"]
    finally:
        g.set_vae_tiling(False)


def test_merge_cut_by_graph_views_runs_plain(sd, engines):
    """An eval callback that asks for every MUL node cuts each merge graph behind m1 and behind m2: the slices are sub-graph views in which m1 / m2 are read
    outside (the planner's phantom reader), so the fused merge must refuse and the plain nodes must give the same bits"""
    g, _ = engines["SD15_TINY"]
    x = np.random.default_rng(77).standard_normal((2, 3, 17, 19)).astype(np.float32)
    kw = dict(tile_size_x=8, tile_size_y=8, target_overlap=0.5, tile_batch=3)
    n_batches = -(-len(sd.tiling_plan(19, 17, **{k: v for k, v in kw.items() if k != "tile_batch"})["tiles"]) // 3)
    mul = sd.op_number("MUL")
    try:
        g.set_vae_tiling(True, **kw)
        want = g.tiling_blend(x)
        s0 = sd.backend_stats() if ON_GPU else None
        with sd.EvalTrace(lambda i, ts: ts.op == mul, with_src1=False) as tr:
            got = g.tiling_blend(x)
        np.testing.assert_array_equal(got, want)
        assert len(tr.records) == 2 * n_batches
        if ON_GPU:
            s1 = sd.backend_stats()
            assert s1["fused_tile_merge"] == s0["fused_tile_merge"] and s1["view_graphs"] > s0["view_graphs"]
    finally:
        g.set_vae_tiling(False)


POISON_CHILD = """
import sys
sys.path.insert(0, {root!r})
import numpy as np
import sdcpp_amd as sd
sd.lib()
sd.load_mi355x_backend()
e = sd.Engine(model=sd.SD15_TINY, backend="MI355X0")
e.set_vae_tiling(True, tile_size_x=8, tile_size_y=8, target_overlap=0.5, tile_batch=3)
z = (np.random.default_rng(2).standard_normal((1, 4, 17, 19)) * 0.36).astype(np.float32)
out = e.vae_decode(z, raw=True)
assert out.shape == (1, 3, 136, 152)
print("FINITE" if np.isfinite(out).all() else "NOT FINITE")
"""


@pytest.mark.skipif(not ON_GPU, reason="the poison pattern is the MI355X backend's allocator option")
def test_canvas_is_zeroed_under_poison(gpu):
    """Every fresh device buffer is filled with NaN bit patterns: a canvas that was accumulated into without being cleared would come back NaN"""
    root = str(Path(__file__).resolve().parent.parent)
    env = dict(os.environ, GGML_MI355X_POISON="1")
    r = subprocess.run([sys.executable, "-c", POISON_CHILD.format(root=root)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FINITE" in r.stdout and "NOT FINITE" not in r.stdout
