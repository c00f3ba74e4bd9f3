#!/usr/bin/env python
"""One Linear per weight type and route, timed on the device: the measurement behind the MXFP4 policy (kernels/bquant.hip), in the shape of
scripts/bquant_probe.py.  mxfp4 / iq4_nl: kernel = k_bq_gemm (its row limit lifted), image = cached f16 image + k_gemm16 (built once, outside the timed launches),
jit = k_bq_image in front of every k_gemm16.  q4_0: default = the planner's own choice (its raw kernels up to 512 rows), image = the cached f16 image.  The three
types run one after the other on each shape, in one process.  Time = HIP events around every dispatch of the graph summed over all kernel families, one
graph_compute per sample after 2 warm-up runs; median of 5 with min .. max.  The weights of ONE Linear stay L2 / Infinity-Cache warm between samples (at most
15 MB raw): the figures compare routes and types, they are not a step's share.
  python scripts/mxfp4_probe.py [--shrink N]        (SDCPP_BACKEND_LIB = another build of the backend)"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "scripts")]
import sdcpp_amd as sd
from bquant_probe import BROUTES, DEFAULTS, QROUTES, linear
from ggml_graph import Graph

TYPES = {"mxfp4": (39, 17), "iq4_nl": (20, 18), "q4_0": (2, 18)}   # ggml type, bytes per 32 weights
SHAPES = [(1280, 1280, (1,)), (3072, 9216, (1, 256, 512)), (4096, 3072, (256, 512))]   # (K, M, rows)


def main():
    ap = argparse.ArgumentParser()
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
            for tname, (wt, bpb) in TYPES.items():
                line = f"{tname:6s} {K:5d} -> {M:5d} rows {rows:4d} ({M * K // 32 * bpb / 1e6:5.1f} MB raw)"
                for route, opts in (QROUTES if wt == 2 else BROUTES).items():
                    for k, v in opts.items():
                        sd.backend_set_option(k, v)
                    with Graph("MI355X0") as g:
                        node = linear(L, g, w, wt, b, x, False)
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
