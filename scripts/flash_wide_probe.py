#!/usr/bin/env python
"""The d = 512 attention of the KL-VAE mid-block, timed on the device on its two routes (kernels/flash_wide.hip):
  wide      the FLASH_ATTN_EXT node (f16 K / V) on k_flash_wide — what Engine(flash_attn=True) emits now;
  composed  the MUL_MAT -> SCALE -> SOFT_MAX -> MUL_MAT chain on the GEMM composition (planner.cpp plan_manual_attention) — what the same flag fell back to
            before the node was claimed, and what flash_attn=False still takes.
Part 1: the attention alone, d = 512, Lq = Lk in {1024, 4096, 16384}, HN in {1, 8}.  Time = HIP events around every dispatch of the graph summed over all kernel
families, one graph_compute per sample after 2 warm-up runs; median of 5 with min .. max.  Scratch = the arena bytes the plan allocates, from the planner's own
formula (the composition: Q image, K / V weight images, f32 scores, f16 probabilities; the node: none).  TFLOP/s = 4 Lq Lk d HN / time.
Part 2 (--vae): KL-VAE decode of the full-width SD1.5 decoder, wall clock around the call after one warm-up (it ends in a device-to-host copy), median of 5:
512^2 batch 8, 1024^2 batch 1, and 1024^2 under set_vae_tiling with 64 x 64-latent tiles; flash_attn=True against flash_attn=False.
  python scripts/flash_wide_probe.py [--vae] [--shrink N]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sdcpp_amd as sd
from ggml_graph import F16, Graph


def rup64(x):
    return (x + 63) // 64 * 64


def timed(L, g, node):
    g.run(node)
    gf = L.ggml_new_graph_custom(g.ctx, 64, False)
    L.ggml_build_forward_expand(gf, node)
    us = []
    for i in range(7):
        sd.kernel_timing_enable(sd.KF_ALL)
        L.ggml_backend_graph_compute(g.backend, gf)
        t = sd.kernel_timings()
        if i >= 2:
            us.append(sum(f["total_ms"] for f in t) * 1e3)
    sd.kernel_timing_enable(0)
    return us


def attention(a):
    L, rng, d = sd.lib(), np.random.default_rng(0), 512
    for Ln in (1024, 4096, 16384):
        Ln //= a.shrink
        for HN in (1, 8):
            q, k, v = (rng.standard_normal((HN, Ln, d)).astype(np.float32) for _ in range(3))
            scale, flop = 1.0 / np.sqrt(d), 4.0 * Ln * Ln * d * HN
            scratch = {"wide": 0, "composed": Ln * rup64(d) * 2 + 2 * rup64(Ln) * rup64(d) * 2 + Ln * Ln * 4 + Ln * rup64(Ln) * 2}
            line = f"d {d} Lq = Lk {Ln:5d} HN {HN}"
            for route in ("wide", "composed"):
                with Graph("MI355X0") as g:
                    if route == "wide":
                        node = L.ggml_flash_attn_ext(g.ctx, g.input(q), g.input(k, F16), g.input(v, F16), None, scale, 0.0, 0.0)
                    else:
                        kq = L.ggml_soft_max_inplace(g.ctx, L.ggml_scale_inplace(g.ctx, L.ggml_mul_mat(g.ctx, g.input(k), g.input(q)), scale))
                        node = L.ggml_mul_mat(g.ctx, g.input(np.ascontiguousarray(v.transpose(0, 2, 1))), kq)
                    us = timed(L, g, node)
                line += f" | {route}: {np.median(us):9.1f} us [{min(us):.1f} .. {max(us):.1f}] {flop / np.median(us) / 1e6:6.1f} TFLOP/s, scratch {scratch[route] / 2**20:7.1f} MiB"
            print(line, flush=True)


def vae(a):
    rng = np.random.default_rng(1)
    legs = [("512^2 batch 8", (8, 4, 64 // a.shrink, 64 // a.shrink), False), ("1024^2 batch 1", (1, 4, 128 // a.shrink, 128 // a.shrink), False),
            ("1024^2 batch 1, 64 x 64-latent tiles", (1, 4, 128 // a.shrink, 128 // a.shrink), True)]
    for name, shape, tiled in legs:
        z = (rng.standard_normal(shape) * 0.5).astype(np.float32)
        line = f"VAE decode {name}"
        for flash in (True, False):
            e = sd.Engine(model=sd.SD15, backend="MI355X0", flash_attn=flash)
            if tiled:
                e.set_vae_tiling(True, tile_size_x=64 // a.shrink, tile_size_y=64 // a.shrink)
            e.vae_decode(z)
            ms = []
            for _ in range(5):
                t0 = time.perf_counter()
                e.vae_decode(z)
                ms.append((time.perf_counter() - t0) * 1e3)
            del e
            line += f" | flash_attn={flash}: {np.median(ms):8.1f} ms [{min(ms):.1f} .. {max(ms):.1f}]"
        print(line, flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--vae", action="store_true")
    ap.add_argument("--shrink", type=int, default=1, help="divide the sizes by this (rehearsal)")
    a = ap.parse_args()
    sd.load_mi355x_backend()
    print(f"backend: {sd.BACKEND_LIB}")
    vae(a) if a.vae else attention(a)
