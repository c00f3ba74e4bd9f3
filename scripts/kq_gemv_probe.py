#!/usr/bin/env python
"""The hoisted K-quant groups as ONE k_kq_gemv launch against the same graph as N separate k_kq_gemm launches (option qgemv = 0): the measurement behind
kq_gemv_supported (kernels/kquant.hip).  Built like scripts/kquant_low_probe.py.  A group is N chains SiLU -> MUL_MAT -> ADD(bias) on one input
of 1 or 2 rows (plan_hoisted_mod); every member is its own tensor in device memory (one member's random super-blocks, uploaded N times: 75 .. 370 MB per 3072-wide
group, which streams from HBM; the 1280-wide group, 7 .. 17 MB, stays in the caches).  Run it on the build under test and, with SDCPP_BACKEND_LIB, on a build of the
parent commit (there both columns are N x k_kq_gemm).  q8_0's launch_qgemv_group on the first shape is the rate to aim for.
  kernels: HIP events around every dispatch of the graph summed over all kernel families, one graph_compute per sample after 2 warm-up runs, median of 5 with
           min .. max; GB/s = raw weight bytes over that median.  The device-to-device copies of the members' columns (grouped route only) are not in it:
  wall:    host clock around graph_compute (which synchronises), timing off, median of 20 with min .. max: launch overhead and those copies included.
  python scripts/kq_gemv_probe.py [--types q4_K,q6_K] [--shrink 16]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import kquant_low_ref as KQL
import kquant_ref as KQ
import sdcpp_amd as sd
from ggml_graph import F32, Graph

TYPES = {"q8_0": 8, **KQL.TYPES, **KQ.TYPES}
BLOCK = {8: (32, 34), **{t: (256, b) for t, b in {**KQL.BLOCK_BYTES, **KQ.BLOCK_BYTES}.items()}}
# (K, member sizes, rows): FLUX double-block and single-block modulation, the SDXL ResBlock embedding projections shaped as a modulation group
SHAPES = [(3072, (18432,) * 8, (1,)), (3072, (9216,) * 8, (1, 2)), (1280, (320,) * 8 + (640,) * 7 + (1280,) * 7, (2,))]


def raw_blocks(rng, wt, n):
    """n random blocks of the type, |w| of a few units"""
    if wt == 8:
        d = np.full((n, 1), 2.0 ** -6, np.float16).view(np.uint8)
        return np.concatenate([d, rng.integers(0, 256, (n, 32), dtype=np.uint8)], axis=1)
    Q = KQL if wt in KQL.TYPES.values() else KQ
    return Q.pack(wt, *Q.random_fields(rng, wt, n, np.full(n, 2.0 ** -6, np.float16), np.full(n, 2.0 ** -6, np.float16)))


def measure(L, wt, K, Ms, x, blocks, bias):
    with Graph("MI355X0") as g:
        xi, outs = g.input(x), []
        for M in Ms:
            w = L.ggml_new_tensor_2d(g.wctx, wt, K, M)
            g._weights.append((w, blocks[: M * K // BLOCK[wt][0]].tobytes()))
            outs.append(L.ggml_add_inplace(g.ctx, L.ggml_mul_mat(g.ctx, w, L.ggml_silu(g.ctx, xi)), g.weight(bias[:M], F32)))
        g.run(*outs)
        gf = L.ggml_new_graph_custom(g.ctx, 256, False)
        for o in outs:
            L.ggml_build_forward_expand(gf, o)
        us, wall = [], []
        for i in range(7):
            sd.kernel_timing_enable(sd.KF_ALL)
            L.ggml_backend_graph_compute(g.backend, gf)
            t = sd.kernel_timings()
            if i >= 2:
                us.append(sum(f["total_ms"] for f in t) * 1e3)
        sd.kernel_timing_enable(0)
        for i in range(22):
            t0 = time.perf_counter()
            L.ggml_backend_graph_compute(g.backend, gf)
            if i >= 2:
                wall.append((time.perf_counter() - t0) * 1e6)
    return us, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--types", default="q8_0,q2_K,q3_K,q4_K,q5_K,q6_K")
    ap.add_argument("--shrink", type=int, default=1, help="divide the member sizes by this (rehearsal)")
    a = ap.parse_args()
    sd.load_mi355x_backend()
    L, rng = sd.lib(), np.random.default_rng(0)
    print(f"backend: {sd.BACKEND_LIB}")
    for si, (K, Ms, rowset) in enumerate(SHAPES):
        Ms = tuple(max(4, M // a.shrink // 4 * 4) for M in Ms)
        bias = rng.standard_normal(max(Ms)).astype(np.float32)
        for tname in a.types.split(","):
            wt = TYPES[tname]
            if wt == 8 and si > 0:
                continue
            blocks = raw_blocks(rng, wt, max(Ms) * K // BLOCK[wt][0])
            mb = sum(Ms) * K // BLOCK[wt][0] * BLOCK[wt][1] / 1e6
            for rows in rowset:
                x = rng.standard_normal((rows, K)).astype(np.float32)
                line = f"{tname} {len(Ms):2d} x {K} -> {Ms[0]}..{Ms[-1]} rows {rows} ({mb:6.1f} MB raw)"
                for mode, q in (("group", 1), ("separate", 0)):
                    sd.backend_set_option("qgemv", q)
                    try:
                        us, wall = measure(L, wt, K, Ms, x, blocks, bias)
                    finally:
                        sd.backend_set_option("qgemv", 1)
                    m = float(np.median(us))
                    line += f" | {mode}: {m:7.1f} us [{min(us):.1f} .. {max(us):.1f}] {mb / m * 1e3:6.0f} GB/s, wall {np.median(wall):7.1f} us [{min(wall):.1f} .. {max(wall):.1f}]"
                print(line, flush=True)


if __name__ == "__main__":
    main()
