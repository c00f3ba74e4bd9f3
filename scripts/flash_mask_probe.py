#!/usr/bin/env python
"""Masked attention timed on the device on its two routes (kernels/flash_mask.hip):
  mask    the FLASH_ATTN_EXT node with an f16 mask (f16 K / V) on k_flash_mask — what Engine(flash_attn=True) emits for the text encoders now;
  chain   MUL_MAT -> SCALE -> ADD(mask) -> SOFT_MAX -> MUL_MAT — what the same flag fell back to before the node was claimed, and what flash_attn=False still takes;
  plain   (the joint-attention shape only) the same node without its mask on k_flash_attn: what the mask stream costs.
Shapes: CLIP-L 77 x 77, 12 heads, d = 64, causal; T5-XXL 256 and 512 tokens, 64 heads, d = 64, per-head bias; a Chroma-like joint attention of 4352 tokens, 24 heads,
d = 128, the last 200 keys masked.  Time = HIP events around every dispatch of the graph summed over all kernel families, one graph_compute per sample after 2 warm-up
runs; median of 5 with min .. max; one process.  (The dead-tile skip the kernel once had was a compile-time switch, timed by running this script on both builds:
profiles/flash_mask_probe.txt holds both; it did not pay and is gone.)
  python scripts/flash_mask_probe.py [--shrink N]"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sdcpp_amd as sd
from ggml_graph import F16, Graph


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


def main(a):
    L, rng = sd.lib(), np.random.default_rng(0)
    shapes = [("CLIP-L causal", 64, 77, 12, 1, "causal"), ("T5-XXL bias", 64, 256, 64, 64, "bias"), ("T5-XXL bias", 64, 512, 64, 64, "bias"),
              ("joint, 200 keys padded", 128, 4352 // a.shrink, 24, 1, "keypad")]
    for name, d, Ln, HN, Hm, kind in shapes:
        q, k, v = (rng.standard_normal((HN, Ln, d)).astype(np.float32) for _ in range(3))
        m = rng.normal(0.0, 2.0, (Hm, Ln, Ln)).astype(np.float32) if kind == "bias" else np.zeros((Hm, Ln, Ln), np.float32)
        if kind == "causal":
            m[:, np.triu_indices(Ln, 1)[0], np.triu_indices(Ln, 1)[1]] = -np.inf
        if kind == "keypad":
            m[:, :, Ln - 200 // a.shrink:] = -np.inf
        scale, flop = 1.0 / np.sqrt(d), 4.0 * Ln * Ln * d * HN
        line = f"{name}: d {d} L {Ln:5d} HN {HN:2d} Hm {Hm:2d}"
        for route in ("mask", "chain") + (("plain",) if kind == "keypad" else ()):
            with Graph("MI355X0") as g:
                if route == "chain":
                    kq = L.ggml_scale_inplace(g.ctx, L.ggml_mul_mat(g.ctx, g.input(k), g.input(q)), scale)
                    kq = L.ggml_soft_max_inplace(g.ctx, L.ggml_add_inplace(g.ctx, kq, g.input(m)))
                    node = L.ggml_mul_mat(g.ctx, g.input(np.ascontiguousarray(v.transpose(0, 2, 1))), kq)
                else:
                    node = L.ggml_flash_attn_ext(g.ctx, g.input(q), g.input(k, F16), g.input(v, F16), g.input(m, F16) if route == "mask" else None, scale, 0.0, 0.0)
                us = timed(L, g, node)
            line += f" | {route}: {np.median(us):9.1f} us [{min(us):.1f} .. {max(us):.1f}] {flop / np.median(us) / 1e6:6.1f} TFLOP/s"
        print(line, flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shrink", type=int, default=1, help="divide the joint-attention size by this (rehearsal)")
    a = ap.parse_args()
    sd.load_mi355x_backend()
    print(f"backend: {sd.BACKEND_LIB}")
    main(a)
