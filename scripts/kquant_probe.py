#!/usr/bin/env python
"""One Linear of FLUX.1-dev's shapes per weight type and route, timed on the device: the measurement behind the K-quant policy (kernels/kquant.hip).
Routes of a q4_K / q5_K / q6_K weight: k1-rb2 / k1-rb4 = k_kq_gemm on 64- / 128-row tiles (up to 32 rows both are the 32-row tile), image = cached f16 image +
k_gemm16 (the image is built once, outside the timed launches), jit = k_kq_image in front of every k_gemm16.  q4_0 / q8_0: default = the planner's own choice,
image = the cached f16 image.  Time = HIP events around every dispatch of the graph summed over all kernel families (pack / split-K / image passes count), one
graph_compute per sample after 2 warm-up runs; median of 5 with min .. max.  The weights of ONE Linear are L2 / Infinity-Cache warm between samples for the small
shapes: the figures compare routes, they are not a step's share.
  python scripts/kquant_probe.py [--types q4_K,q6_K,q4_0,q8_0]        (SDCPP_BACKEND_LIB = another build of the backend: the same shapes on the parent commit)"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sdcpp_amd as sd
from ggml_graph import F32, Graph

TYPES = {"q4_0": 2, "q8_0": 8, "q4_K": 12, "q5_K": 13, "q6_K": 14}
BYTES_PER_256 = {2: 144, 8: 272, 12: 144, 13: 176, 14: 210}
BIG = dict(qgemm16_max_rows=8192)
KROUTES = {"k1-rb2": dict(qgemm16=1, qgemm16_rb=2, **BIG), "k1-rb4": dict(qgemm16=1, qgemm16_rb=4, **BIG), "image": dict(qgemm16=0, jit_qimages=0),
           "jit": dict(qgemm16=0, jit_qimages=1)}
QROUTES = {"default": {}, "image": dict(qgemv=0, qgemm16=0, jit_qimages=0, qinloop_min_rows=0)}
DEFAULTS = dict(qgemm16=1, qgemm16_rb=3, qgemm16_max_rows=512, jit_qimages=4096, qgemv=1, qinloop_min_rows=513)
SHAPES = [(3072, 18432, (1,)), (4096, 3072, (256, 512)), (3072, 9216, (256, 512)), (3072, 12288, (4608,))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="q4_K,q6_K,q4_0,q8_0")
    ap.add_argument("--shrink", type=int, default=1, help="divide M by this (rehearsal)")
    a = ap.parse_args()
    sd.load_mi355x_backend()
    L, rng = sd.lib(), np.random.default_rng(0)
    print(f"backend: {sd.BACKEND_LIB}")
    for K, M, rowset in SHAPES:
        M //= a.shrink
        w = (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(M).astype(np.float32)
        for tname in a.types.split(","):
            wt = TYPES[tname]
            for rows in rowset:
                x = rng.standard_normal((rows, K)).astype(np.float32)
                line = f"{tname} {K:5d} -> {M:5d} rows {rows:4d} ({M * K // 256 * BYTES_PER_256[wt] / 1e6:5.1f} MB raw)"
                for route, opts in (KROUTES if wt >= 12 else QROUTES).items():
                    if rows <= 32 and route == "k1-rb4":
                        continue
                    for k, v in opts.items():
                        sd.backend_set_option(k, v)
                    with Graph("MI355X0") as g:
                        node = L.ggml_add_inplace(g.ctx, L.ggml_mul_mat(g.ctx, g.weight(w, wt), g.input(x)), g.weight(b, F32))
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
                    for k in opts:
                        sd.backend_set_option(k, DEFAULTS[k])
                    line += f" | {route}: {np.median(us):7.1f} us [{min(us):.1f} .. {max(us):.1f}]"
                print(line, flush=True)


if __name__ == "__main__":
    main()
