#!/usr/bin/env python
"""One Linear of FLUX.1-dev's shapes per route for q2_K and q3_K weights, with q4_K FROM THE SAME RUN as the yardstick: the measurement behind their row
thresholds (kq_gemm_supported in kernels/kquant.hip).  Built like scripts/kquant_probe.py.  Routes: k1 = k_kq_gemm with its row limit lifted
(qgemm16_max_rows = 16384, so that a type that hands over at half the option is still on it at 4608 rows; 64-row tiles above 32 rows), image = cached f16 image +
k_gemm16 (the image is built once, outside the timed launches), jit = k_kq_image in front of every k_gemm16.  Time = HIP events around every dispatch of the graph summed over all kernel families (pack / split-K / image passes count), one
graph_compute per sample after 2 warm-up runs; median of 5 with min .. max.  CACHE-WARM: the weights of ONE Linear stay in L2 / Infinity Cache between samples
for the small shapes, so the figures compare routes and types, they are not a step's share.
  python scripts/kquant_low_probe.py [--types q2_K,q3_K,q4_K]"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sdcpp_amd as sd
from ggml_graph import F32, Graph

TYPES = {"q2_K": 10, "q3_K": 11, "q4_K": 12}
BYTES_PER_256 = {10: 84, 11: 110, 12: 144}
ROUTES = {"k1": dict(qgemm16=1, qgemm16_max_rows=16384), "image": dict(qgemm16=0, jit_qimages=0), "jit": dict(qgemm16=0, jit_qimages=1)}
DEFAULTS = dict(qgemm16=1, qgemm16_max_rows=512, jit_qimages=4096)
SHAPES = [(3072, 18432, (1,)), (4096, 3072, (256, 512)), (3072, 9216, (256, 512)), (3072, 12288, (4608,))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="q2_K,q3_K,q4_K")
    ap.add_argument("--shrink", type=int, default=1, help="divide M by this (rehearsal)")
    a = ap.parse_args()
    sd.load_mi355x_backend()
    L, rng = sd.lib(), np.random.default_rng(0)
    print(f"backend: {sd.BACKEND_LIB}")
    for K, M, rowset in SHAPES:
        M //= a.shrink
        w = (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(M).astype(np.float32)
        for rows in rowset:
            x = rng.standard_normal((rows, K)).astype(np.float32)
            for tname in a.types.split(","):
                wt = TYPES[tname]
                line = f"{tname} {K:5d} -> {M:5d} rows {rows:4d} ({M * K // 256 * BYTES_PER_256[wt] / 1e6:5.1f} MB raw)"
                for route, opts in ROUTES.items():
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
