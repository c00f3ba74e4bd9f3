#!/usr/bin/env python
"""One Linear of the SD1.5 / SDXL / FLUX shapes per weight type and route, timed on the device: the measurement behind the q4_1 / q5_0 / q5_1 / iq4_nl policy
(kernels/bquant.hip).  Routes of such a weight: kernel = k_bq_gemm (its row limit lifted), image = cached f16 image + k_gemm16 (the image is
built once, outside the timed launches), jit = k_bq_image in front of every k_gemm16.  q4_0 / q8_0: default = the planner's own choice, image = the cached f16
image.  The GEGLU line is FF1 (320 -> 2560) + bias + GEGLU + an f16 FF2 (1280 -> 320): FF2's launch is in every figure of that line, and FF1 goes through the
image in the GEGLU order on every route.  Time = HIP events around every dispatch of the graph summed over all kernel families (pack / split-K / image passes
count), one graph_compute per sample after 2 warm-up runs; median of 5 with min .. max.  The weights of ONE Linear are L2 / Infinity-Cache warm between samples
for the small shapes: the figures compare routes, they are not a step's share.
  python scripts/bquant_probe.py [--types q5_0,q4_0,...]        (SDCPP_BACKEND_LIB = another build of the backend: the same shapes on the parent commit)"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import sdcpp_amd as sd
from ggml_graph import F16, F32, Graph, tensor_struct

TYPES = {"q4_0": 2, "q8_0": 8, "q4_1": 3, "q5_0": 6, "q5_1": 7, "iq4_nl": 20}
BYTES_PER_32 = {2: 18, 8: 34, 3: 20, 6: 22, 7: 24, 20: 18}
BROUTES = {"kernel": dict(qgemm16=1, qgemm16_max_rows=8192), "image": dict(qgemm16=0, jit_qimages=0), "jit": dict(qgemm16=0, jit_qimages=1)}
QROUTES = {"default": {}, "image": dict(qgemv=0, qgemm16=0, jit_qimages=0, qinloop_min_rows=0)}
DEFAULTS = dict(qgemm16=1, qgemm16_max_rows=512, jit_qimages=4096, qgemv=1, qinloop_min_rows=513)
# (K, M, rows, GEGLU)
SHAPES = [(1280, 1280, (1, 2, 8), False), (768, 320, (77, 616), False), (2048, 640, (77, 616), False), (320, 2560, (4096,), True),
          (3072, 18432, (1,), False), (4096, 3072, (256, 512), False)]


def linear(L, g, w, wt, b, x, geglu):
    y = L.ggml_add_inplace(g.ctx, L.ggml_mul_mat(g.ctx, g.weight(w, wt), g.input(x)), g.weight(b, F32))
    if not geglu:
        return y
    s, M = tensor_struct(y), w.shape[0]
    ne, nb = [int(s.ne[i]) for i in range(4)], [int(s.nb[i]) for i in range(4)]
    lo = L.ggml_view_4d(g.ctx, y, M // 2, ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], 0)
    hi = L.ggml_view_4d(g.ctx, y, M // 2, ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], M // 2 * 4)
    h = L.ggml_mul(g.ctx, lo, L.ggml_gelu_inplace(g.ctx, L.ggml_cont(g.ctx, hi)))
    return L.ggml_mul_mat(g.ctx, g.weight(np.full((w.shape[1], M // 2), 1.0 / M, np.float32), F16), h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="q4_1,q5_0,q5_1,iq4_nl,q4_0,q8_0")
    ap.add_argument("--shrink", type=int, default=1, help="divide M by this (rehearsal)")
    a = ap.parse_args()
    sd.load_mi355x_backend()
    L, rng = sd.lib(), np.random.default_rng(0)
    print(f"backend: {sd.BACKEND_LIB}")
    for K, M, rowset, geglu in SHAPES:
        M //= a.shrink
        w = (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)
        b = rng.standard_normal(M).astype(np.float32)
        for tname in a.types.split(","):
            wt = TYPES[tname]
            for rows in rowset:
                x = rng.standard_normal((rows, K)).astype(np.float32)
                line = f"{tname:6s} {K:5d} -> {M:5d}{' GEGLU' if geglu else ''} rows {rows:4d} ({M * K // 32 * BYTES_PER_32[wt] / 1e6:5.1f} MB raw)"
                for route, opts in (QROUTES if wt in (2, 8) else BROUTES).items():
                    if geglu and route in ("kernel", "jit"):   # (a GEGLU Linear always takes the cached image, in the GEGLU order)
                        continue
                    for k, v in opts.items():
                        sd.backend_set_option(k, v)
                    with Graph("MI355X0") as g:
                        node = linear(L, g, w, wt, b, x, geglu)
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
