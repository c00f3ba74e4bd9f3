#!/usr/bin/env python
"""What making IP-Adapter image tokens from a picture costs: the CLIP preprocessing kernel, the ViT-H/14 vision tower at full width (32 layers, hidden 1280, 257
tokens) with the embeddings stage as one launch (k_patch_embed, backend option fuse_patch_embed=1) and as plain nodes (=0: k_im2col, a generic GEMM, two transposing
CONTs, REPEAT, CONCAT, ADD), the plus adapters' Resampler (dim 1280, depth 4, 16 queries, output 2048, ff 5120: the SDXL plus adapter's shape), and the whole
sd_set_ip_adapter_image call — in ONE process on one GPU, on synthetic weights, batch 1 and 8, medians of `reps` timed calls after an untimed one that builds the plans.

Times are host wall-clock around synchronous entry points (each ends with the result on the host).  The two tower legs alternate over the repetitions, so a drift of
the shared machine hits both alike; the embeddings stage alone is also timed as an op graph (the chain of clip.hpp:224-235 on a [224, 224, 3, n] input), where it
is not buried under 32 encoder layers.  min / max are the run-to-run spread.  Appends to profiles/clip_vision_probe.txt.

usage: clip_vision_probe.py [reps=5] [out=FILE]"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sdcpp_amd as sd


def timed(fn, reps):
    fn()  # builds the plans
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return np.array(t)


def fmt(t):
    return f"{np.median(t):9.3f} ms   (min {t.min():.3f}, max {t.max():.3f} over {t.size} runs)"


def main():
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    reps = int(opts.get("reps", 5))
    path = Path(opts.get("out", ROOT / "profiles" / "clip_vision_probe.txt"))
    path.parent.mkdir(parents=True, exist_ok=True)
    out = open(path, "a")

    def say(line):
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    sd.load_mi355x_backend()
    rng = np.random.default_rng(0)
    t0 = time.time()
    e = sd.Engine(model=sd.SD15_TINY, wtype=sd.F16, flash_attn=True)  # the UNet does not matter here: the tower and the adapter carry their own weights
    e.clip_vision_init(sd.CLIP_VIT_H_14, weight_seed=1)
    e.ip_adapter_init_plus(64, 1280, 4, 16, 1280, 5120, weight_seed=1)  # output 64 = the tiny UNet's context width; the Resampler's cost sits in its 1280-wide layers
    info = e.clip_vision_info()
    say(f"== CLIP ViT-H/14 vision tower ({info['n_layer']} layers, hidden {info['hidden_size']}, {info['num_positions']} tokens), synthetic f16 weights, {reps} timed runs per leg "
        f"(context made in {time.time() - t0:.0f} s)")
    for n in (1, 8):
        img = rng.integers(0, 256, (n, 480, 640, 3), dtype=np.uint8)
        say(f" -- batch {n}, pictures 640 x 480")
        say(f"   clip_preprocess (kernel, uploads and download)     {fmt(timed(lambda: e.clip_preprocess(img), reps))}")
        px = e.clip_preprocess(img)
        legs = {1: [], 0: []}
        res = {}
        for rep in range(reps + 1):  # alternate; an option change drops the plans, so every timed call follows an untimed one of its leg
            for fuse in (1, 0):
                sd.backend_set_option("fuse_patch_embed", fuse)
                e.clip_vision_encode(px, False, 2)
                t1 = time.perf_counter()
                res[fuse] = e.clip_vision_encode(px, False, 2)
                if rep > 0:
                    legs[fuse].append((time.perf_counter() - t1) * 1e3)
        sd.backend_set_option("fuse_patch_embed", 0)  # the default
        say(f"   tower, hidden state at clip_skip 2, fuse_patch_embed=1 {fmt(np.array(legs[1]))}")
        say(f"   tower, hidden state at clip_skip 2, fuse_patch_embed=0 {fmt(np.array(legs[0]))}")
        say(f"   fused vs plain embeddings: hidden states rel-L2 {float(np.linalg.norm(res[1] - res[0]) / np.linalg.norm(res[0])):.2e}")
        say(f"   tower, pooled                                      {fmt(timed(lambda: e.clip_vision_encode(px, True, -1), reps))}")
        hid = res[1]
        say(f"   Resampler (1280, depth 4, 16 queries, 257 tokens)  {fmt(timed(lambda: e.ip_adapter_project(hid), reps))}")
        # the embeddings stage alone, as an op graph
        from ggml_graph import F16, F32, Graph

        E, P, S = info["hidden_size"], info["patch_size"], info["image_size"]
        w = rng.standard_normal((E, 3, P, P)).astype(np.float32) * 0.05
        cls, pos = rng.standard_normal((E,)).astype(np.float32), rng.standard_normal((info["num_positions"], E)).astype(np.float32)
        emb = {1: [], 0: []}
        L = sd.lib()
        for rep in range(reps + 1):
            for fuse in (1, 0):
                sd.backend_set_option("fuse_patch_embed", fuse)
                with Graph("MI355X0") as g:
                    x = g.input(px)
                    conv = L.ggml_conv_2d(g.ctx, g.weight(w, F16), x, P, P, 0, 0, 1, 1)
                    pe = L.ggml_reshape_3d(g.ctx, conv, info["num_positions"] - 1, E, n)
                    pe = L.ggml_reshape_4d(g.ctx, L.ggml_cont(g.ctx, L.ggml_permute(g.ctx, pe, 1, 0, 2, 3)), 1, E, info["num_positions"] - 1, n)
                    c = L.ggml_reshape_4d(g.ctx, L.ggml_repeat(g.ctx, g.weight(cls, F32), L.ggml_new_tensor_2d(g.ctx, F32, E, n)), 1, E, 1, n)
                    y = L.ggml_add(g.ctx, L.ggml_reshape_3d(g.ctx, L.ggml_concat(g.ctx, c, pe, 2), E, info["num_positions"], n), g.weight(pos, F32))
                    g.run(y)  # places the graph, uploads, builds the plan
                    gf_t = []
                    for _ in range(3):  # the same graph again: a plan-cache hit, kernels only (+ the result's download)
                        t1 = time.perf_counter()
                        g.run(y)
                        gf_t.append((time.perf_counter() - t1) * 1e3)
                if rep > 0:
                    emb[fuse].append(min(gf_t))
        sd.backend_set_option("fuse_patch_embed", 0)  # the default
        say(f"   embeddings stage alone, one launch (k_patch_embed)  {fmt(np.array(emb[1]))}")
        say(f"   embeddings stage alone, plain nodes                {fmt(np.array(emb[0]))}")
        if n == 1:
            one = img[0]
            say(f"   set_ip_adapter(image=...), plus adapter, whole call {fmt(timed(lambda: e.set_ip_adapter(image=one, strength=0.6), reps))}")
    e.close()


if __name__ == "__main__":
    main()
