"""The case table of the Linear route tests: each case is ONE Linear (a MUL_MAT with a static weight and its epilogue nodes; the transcendental epilogues add an
identity second Linear that makes the f16 image observable, the grouped launches take the smallest graph the planner groups) on integer-valued data, with the kernel
route it must take stated as launch-counter moves.  tests/test_linear_ref_cpu.py runs every case on the CPU oracle and against the mutants of linear_ref.py (no GPU
needed); tests/test_gpu_linear_routes.py runs it on the product backend, bit for bit, and asserts the counters.

Routes, derived from the launchers' own rules (kernels/gemm16.hip g16_use_bn64, g16_pick_tile, g16_t320_split, gemm16_split_k, gemm16_split_plan, g16_streamk_grid,
g16_tail_rows, g16_pad256_ok, gemm16_qinloop_supported; kernels/qgemm.hip qgemv_supported, fgemv_supported, qgemm16_split_k and the rb choice of launch_qgemm16;
backend/planner.cpp plan_linear, plan_sibling_group, plan_hoisted_mod) and confirmed by the counters on the GPU:

  gemv      <= 16 rows: k_fgemv (f16 / f32 weights, rows * K within 96 KB), k_qgemv (q8_0 / q4_0, 1 .. 2 rows, K <= 12288), k_qgemv_rows<4 / 8 / 16> (3 .. 16 rows within
            128 KB; above 4 rows only with option qgemv_max_rows); bias / residual in the kernel, SiLU of the rows while they are staged (presilu)
  qgemm16   q8_0 / q4_0, 3 .. 512 rows, K % 256 == 0: k_qgemm16<RB = 1 / 2 / 4> by row count (<= 32 / <= 64 / more; RB 4 becomes 2 while the grid stays under 512
            workgroups, option qgemm16_rb = 4 keeps it), K slices of >= 2 segments of 256 towards 512 workgroups, summed by the slab reduce
  t128      k_gemm16 on 128-row tiles: 64 columns wide (t128n64) for M <= 64, and for M % 64 == 0 up to 128 tiles of 128 x 128; else 128 wide (t128).  Slab split
            towards splitk_target = 384 workgroups (<= 8 slices of >= 8 stages), or combined in the launch (splitk_inkernel = 1)
  t256      256 x 128 (t256; t256w by option only), 256 x 160 (t160 by option only: the cost model gives Linears the eight-wave t160n) by the round-cost model
  pipe      the pipelined 256 x 320 (M % 320 == 0, >= 32 K stages, >= 192 tiles, or its own K slices), 256 x 256 (M % 256 == 0, or % 128 from 2048 columns on,
            >= 64 stages, >= 192 tiles) and 256 x 192 tiles (M % 192 == 0, or % 64 from 2048 columns on, where they fill the chip better); raw q8_0 / q4_0 rows
            dequantised in the main loop above 512 rows; stream-K (option streamk) and the row split (option tail_split) of the 256 x 256 tile
Option gemm16_tile forces a tile where the default policy would need a workload-sized launch, with splitk_target = 1 to keep it unsplit; the pipelined tiles then keep
at least the K stages the default policy asks of them (K >= 1024 for t320, K >= 2048 for t256p / t192p), as in conv_cases.py.  (The pipelined loop is written to be
correct below its depth of four stages — G16_PIPE_LOOP clamps its prologue to the stage count, and stream-K hands it ranges of a few stages, which the stream-K cases
run — but no whole launch of fewer than 32 / 64 stages reaches these tiles except through option gemm16_tile, an A/B switch: such launches are not part of this table.)  The default-policy cases ("policy")
are derived for 256 CUs and skip on another device.

Not reachable by these graphs, and left where they are tested: grouped launches with f16 head-major outputs (the hoisted cross-attention K / V projections: only in
front of a FLASH_ATTN_EXT node, tests/test_gpu_ops.py test_cross_attention_kv_of_all_blocks_hoisted); the hoisted ResBlock embedding projections (their output feeds
a conv's chan_add, never a tensor of its own: test_conv_time_embedding_add_fused; they run on launch_fgemv / launch_qgemv, whose kernels the gemv cases cover);
256 x 160 with four waves under the default policy (conv only).

181 cases."""
from __future__ import annotations

import zlib
from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

import linear_ref as R
from ggml_graph import BF16, F16, F32, Q4_0, Q8_0, Graph, tensor_struct

OPTION_DEFAULTS = {"gemm16_tile": -1, "splitk_target": 384, "splitk_inkernel": 0, "fgemv_max_rows": 16, "qgemv_max_rows": 4, "qgemm16_rb": 3, "streamk": 0, "tail_split": 0,
                   "jit_qimages": 4096, "qgemv": 1}
T128, T256, T256W, T160, T160N, T320, T256P, T128N64, T192P = range(9)   # values of option gemm16_tile
TILE_OPT = {"t128": T128, "t256": T256, "t256w": T256W, "t160": T160, "t160n": T160N, "t320": T320, "t256p": T256P, "t128n64": T128N64, "t192p": T192P}
TILE_SHAPE = {"t128": (128, 128), "t128n64": (128, 64), "t256": (256, 128), "t256w": (256, 128), "t160": (256, 160), "t160n": (256, 160), "t320": (256, 320),
              "t256p": (256, 256), "t192p": (256, 192)}
LIN_ROUTE_FIELDS = ("lin_t128 lin_t128n64 lin_t256 lin_t256w lin_t160 lin_t160n lin_t320 lin_t256p lin_t192p lin_t256p_q8 lin_t256p_q4 lin_t192p_q8 lin_t192p_q4 "
                    "lin_streamk lin_rowsplit_main lin_multi lin_splitk_reduce lin_splitk_reduce_ln lin_geglu_pair lin_geglu16 "
                    "lin_qgemv lin_qgemv_rows4 lin_qgemv_rows8 lin_qgemv_rows16 lin_qgemv_group lin_qgemm16_rb1 lin_qgemm16_rb2 lin_qgemm16_rb4 lin_qgemm16_reduce "
                    "lin_fgemv_f16 lin_fgemv_f32 lin_wswz_q").split()
# ... and the planner's counters such a graph can move
ROUTE_FIELDS = LIN_ROUTE_FIELDS + ("fused_linear split_k_gemms split_k_inlaunch fused_gate fused_gelu fused_geglu fused_linear_geglu qgemv_linears qgemm16_linears fgemv_linears "
                                   "fused_presilu fused_sibling_linears head_major_gemms hoisted_mod_linears jit_images qinloop_linears fused_ln_reduce generic_matmul").split()
WTYPES = {"f16": F16, "f32": F32, "bf16": BF16, "q8_0": Q8_0, "q4_0": Q4_0}
FAMILIES = ("gemv", "qgemm16", "t128", "t256", "pipe")


@dataclass
class Case:
    id: str
    family: str                # one of FAMILIES
    rows: int                  # activation rows over all batch dims
    K: int
    M: int
    wtype: str = "f16"
    epi: str = "none"          # one of linear_ref.EPILOGUES
    batch: tuple = (1, 1)      # (ne[2], ne[3]) of the activation
    opts: dict = field(default_factory=dict)     # backend options of the run (restored to OPTION_DEFAULTS afterwards)
    routes: dict = field(default_factory=dict)   # counter -> moves expected; every other field of ROUTE_FIELDS must not move
    S: int = 1                 # K slices of the launch
    tile: str = "t128"         # the tile whose units the failure message speaks in (and the last-tile mutants cut by)
    policy: bool = False       # a default-policy shape derived for 256 CUs
    strided: bool = False      # the activation is a view whose rows are 2 K floats apart
    kind: str = "linear"       # "linear" | "multi" (two head-major siblings in one launch) | "group" (three modulation Linears in one k_qgemv launch)
    fast: bool = False         # chip-filling shape: the reference goes through a float32 matmul

    @property
    def batches(self):
        return self.batch[0] * self.batch[1]

    @property
    def out_cols(self):
        return self.M // 2 if self.epi == "geglu" else self.M


CASES: list[Case] = []


def add(cid, family, rows, K, M, routes, **k):
    r = {**routes, "fused_linear": 1 + routes.get("fused_linear", 0)}   # a case's own "fused_linear" counts its further Linears
    CASES.append(Case(cid, family, rows, K, M, routes={f: v for f, v in r.items() if v}, **k))


def forced_tile(name, M, geglu=False):
    """the tile g16_launch ends on under option gemm16_tile = name (g16_use_bn64, the forced branch of g16_pick_tile; a GEGLU launch is laid out for 128-column pairs)"""
    if M <= 64 and not geglu:
        return "t128n64"
    if name == "t128n64":
        return "t128n64" if M % 64 == 0 and not geglu else "t128"
    if name == "t320":
        return "t320" if M % 320 == 0 and not geglu else "t256"
    if name == "t256p":
        return "t256p" if M % 256 == 0 else "t256"
    if name == "t192p":
        return "t192p" if (M % 192 == 0 or (M % 64 == 0 and M >= 2048)) and not geglu else "t256"
    if name in ("t160", "t160n"):
        return name if M % 160 == 0 and not geglu else "t256"
    return name


def merge(*ds):
    out = {}
    for d in ds:
        for k, v in d.items():
            out[k] = out.get(k, 0) + v
    return out


def g16_routes(tile, epi, M, *, second_tile=None, split=None, gate_fused=True):
    """counter moves of one gemm16 Linear on `tile` with its epilogue; second_tile: where the identity second Linear of gelu / geglu lands"""
    r = {"lin_" + tile: 1}
    if split == "reduce":
        r.update(split_k_gemms=1, lin_splitk_reduce=1)
    elif split == "inlaunch":
        r.update(split_k_gemms=1, split_k_inlaunch=1)
    if epi == "gate" and gate_fused:
        r["fused_gate"] = 1
    if epi == "gelu":
        r = merge(r, {"fused_gelu": 1, "fused_linear": 1, "lin_" + second_tile: 1})
    if epi == "geglu":
        r = merge(r, {"fused_geglu": 1, "fused_linear_geglu": 1, "lin_geglu_pair": 1, "fused_linear": 1, "lin_" + second_tile: 1})
    return r


# ------------------------------------------------------------------------------------------------ forced tiles at their edges
def _tile_cases():
    unsplit = {"splitk_target": 1}
    # per tile: family, widths (ragged, exact, several tiles), K values; rows and epilogues cycle so that every tile meets every row edge class and every epilogue its family
    plain = ["none", "bias", "bias+res", "res+bias", "scale", "gate"]
    tiles = {"t128": ("t128", (65, 130, 200, 384), (8, 40, 64, 72, 100, 320, 2880)),
             "t128n64": ("t128", (1, 63, 64, 128, 320), (8, 40, 64, 72, 100, 320, 2880)),
             "t256": ("t256", (65, 130, 200, 384), (8, 40, 64, 72, 100, 320, 2880)),
             "t256w": ("t256", (128, 130, 200), (72, 8, 320, 100, 2880, 40, 64)),
             "t160": ("t256", (160, 320, 640), (40, 320, 8, 2880, 64, 100, 72)),
             "t160n": ("t256", (160, 320, 640), (100, 64, 2880, 8, 72, 40, 320)),
             "t320": ("pipe", (320, 640), (1024, 2880, 1000, 1096)),
             "t256p": ("pipe", (256, 512), (2048, 2880, 2088, 2120)),
             "t192p": ("pipe", (192, 384, 2112, 2176), (2048, 2880, 2088, 2120))}
    row_edges = (127, 128, 129, 255, 256, 257, 720)
    wts = ("f16", "f16", "bf16", "f16", "f32", "f16", "f16")
    n = 0
    for name, (fam, Ms, Ks) in tiles.items():
        for i, rows in enumerate(row_edges):
            M, K, epi, wt = Ms[i % len(Ms)], Ks[i % len(Ks)], plain[n % len(plain)], wts[n % len(wts)]
            n += 1
            if epi == "gate" and rows % 3 == 0:
                batch = (3, 1)          # 720 = 3 images of 240 tokens
            else:
                batch = (1, 1)
            tile = forced_tile(name, M)
            add(f"{name}-forced-{rows}x{K}-to-{M}-{wt}-{epi}", fam, rows, K, M, g16_routes(tile, epi, M), wtype=wt, epi=epi, batch=batch, tile=tile,
                opts={**unsplit, "gemm16_tile": TILE_OPT[name]})
    # quantised weights through the f16 image (K % 256 != 0 keeps them off k_qgemm16; launch_wswz_linear dequantises), a batched activation, a strided one
    for name, fam, rows, K, M, wt, epi, extra in (("t128", "t128", 257, 320, 130, "q8_0", "bias", {}), ("t128", "t128", 129, 96, 200, "q4_0", "bias+res", {}),
                                                  ("t256", "t256", 257, 320, 130, "q4_0", "res+bias", {}), ("t160n", "t256", 255, 96, 320, "q8_0", "bias", {}),
                                                  ("t320", "pipe", 257, 1056, 320, "q8_0", "bias+res", {}), ("t256p", "pipe", 255, 2080, 256, "q4_0", "bias", {}),
                                                  ("t192p", "pipe", 257, 2080, 384, "q8_0", "res+bias", {}),
                                                  ("t128", "t128", 387, 72, 130, "f16", "bias+res", {"batch": (3, 1)}), ("t256", "t256", 774, 100, 200, "f16", "bias", {"batch": (3, 2)}),
                                                  ("t320", "pipe", 387, 1024, 320, "f16", "bias+res", {"batch": (3, 1)}),
                                                  ("t128", "t128", 257, 72, 130, "f16", "bias", {"strided": True}), ("t256p", "pipe", 300, 2048, 256, "f16", "bias+res", {"strided": True}),
                                                  ("t160", "t256", 300, 40, 160, "bf16", "bias", {"strided": True, "batch": (3, 1)})):
        tile = forced_tile(name, M)
        tag = "-".join(([f"batch{extra['batch'][0]}x{extra['batch'][1]}"] if "batch" in extra else []) + (["strided"] if extra.get("strided") else []))
        add(f"{name}-forced-{rows}x{K}-to-{M}-{wt}-{epi}" + ("-" + tag if tag else ""), fam, rows, K, M, g16_routes(tile, epi, M), wtype=wt, epi=epi, tile=tile,
            opts={**unsplit, "gemm16_tile": TILE_OPT[name]}, **extra)
    # rows <= 16 pushed onto the GEMM (fgemv_max_rows = 0)
    for name, fam, rows, K, M, epi in (("t128", "t128", 1, 40, 130, "bias"), ("t128n64", "t128", 16, 72, 64, "bias+res"), ("t256", "t256", 5, 320, 200, "res+bias"),
                                       ("t320", "pipe", 16, 1024, 320, "bias")):
        tile = forced_tile(name, M)
        add(f"{name}-forced-{rows}-rows-on-the-gemm-{K}-to-{M}-{epi}", fam, rows, K, M, g16_routes(tile, epi, M), epi=epi, tile=tile,
            opts={**unsplit, "gemm16_tile": TILE_OPT[name], "fgemv_max_rows": 0})
    # the transcendental epilogues on every tile family: x in -1 .. 1, K = 64 / 100 keeps the pre-activations small; the identity second Linear runs under the same options
    for name, fam, rows, K, M in (("t128", "t128", 257, 64, 192), ("t128n64", "t128", 129, 100, 64), ("t256", "t256", 300, 64, 192), ("t160n", "t256", 257, 100, 320),
                                  ("t320", "pipe", 257, 1024, 320), ("t256p", "pipe", 129, 2048, 256), ("t192p", "pipe", 257, 2048, 192)):
        o = {**unsplit, "gemm16_tile": TILE_OPT[name]}
        tile = forced_tile(name, M)
        add(f"{name}-forced-{rows}x{K}-to-{M}-gelu", fam, rows, K, M, g16_routes(tile, "gelu", M, second_tile=tile), epi="gelu", tile=tile, opts=o)
    # GEGLU on the 128-column value / gate pairing (a forced tile keeps gemm16_geglu_mode on it; the pipelined tiles meet GEGLU on the 16-column interleave: policy cases)
    for name, fam, rows, K, M in (("t128", "t128", 257, 64, 384), ("t256", "t256", 300, 100, 256)):
        o = {**unsplit, "gemm16_tile": TILE_OPT[name]}
        tile = forced_tile(name, M, geglu=True)
        add(f"{name}-forced-{rows}x{K}-to-{M}-geglu", fam, rows, K, M, g16_routes(tile, "geglu", M, second_tile=forced_tile(name, M // 2)), epi="geglu", tile=tile, opts=o)
    # ... and under the default policy: one 128 x 128 tile per value / gate pair, the identity FF2 on 128 x 64 tiles
    add("t128-default-policy-100x64-to-256-geglu", "t128", 100, 64, 256, g16_routes("t128", "geglu", 256, second_tile="t128n64"), epi="geglu", tile="t128")


# ------------------------------------------------------------------------------------------------ split launches of the 128-row tiles (default policy at any CU count)
def _split_cases():
    # 3 x 2 = 6 workgroups, 90 K stages over 8 slices of 12 (the last one 6): every epilogue the slab reduce serves; scale is separate nodes around it.
    # (a gated Linear does not take the slab split: plan_linear fuses the gate only where gemm16_split_k == 1, and then the MUL and ADD run on their own)
    for e in ("none", "bias", "bias+res", "res+bias", "scale"):
        add(f"t128-split-s8-90-stages-{e}", "t128", 257, 2880, 130, g16_routes("t128", e, 130, split="reduce"), epi=e, S=8)
    add("t128-split-s8-gate-runs-unfused", "t128", 257, 2880, 130, g16_routes("t128", "gate", 130, split="reduce", gate_fused=False), epi="gate", S=8)
    add("t128n64-split-s8-bias+res", "t128", 257, 2880, 64, g16_routes("t128n64", "bias+res", 64, split="reduce"), epi="bias+res", S=8, tile="t128n64")
    # 6 x 22 = 132 workgroups -> 2 slices of 9 stages (K = 520 padded to 576)
    add("t128-split-s2-18-stages-bias+res", "t128", 720, 520, 2762, g16_routes("t128", "bias+res", 2762, split="reduce"), epi="bias+res", S=2)
    # combined in the launch by the last-arriving workgroup (splitk_inkernel = 1): 4 slices of 23, 23, 23, 21 stages, the full epilogue in the kernel
    for e in ("bias+res", "none", "res+bias"):
        add(f"t128-split-in-launch-s4-{e}", "t128", 257, 2880, 130, g16_routes("t128", e, 130, split="inlaunch"), epi=e, S=4, opts={"splitk_inkernel": 1})
    add("t128-split-in-launch-s4-gate-runs-unfused", "t128", 257, 2880, 130, g16_routes("t128", "gate", 130, split="inlaunch", gate_fused=False), epi="gate", S=4,
        opts={"splitk_inkernel": 1})
    # the FUSED gate on the in-launch combine: plan_linear fuses it where gemm16_split_k == 1, which only rules the slab split out; 14 x 14 = 196 tiles of 128 x 128
    # (more than splitk_target / 2 = 192: no slab split) still take 2 slices in the launch, and the last-arriving workgroup applies (acc + b) * gate[image] + r
    # with its rows-per-image indexing: 7 images of 256 tokens
    add("t128-split-in-launch-s2-1792x512-to-1792-fused-gate-7-images", "t128", 1792, 512, 1792, g16_routes("t128", "gate", 1792, split="inlaunch"), epi="gate", S=2,
        batch=(7, 1), opts={"splitk_inkernel": 1})
    # GELU -> f16 image by the last-arriving workgroup: 3 x 3 tiles of 128 x 64, 4 slices of 8 stages (its identity fc2: 6 stages, unsplit)
    add("t128n64-split-in-launch-s4-gelu", "t128", 257, 1024, 192, g16_routes("t128n64", "gelu", 192, second_tile="t128n64", split="inlaunch"), epi="gelu", S=4,
        tile="t128n64", opts={"splitk_inkernel": 1})
    # the slab reduce that also writes the next LayerNorm's operand image (k_splitk_reduce_ln): 8 x 10 = 80 tiles -> 4 slices of 8 stages.  The f32 rows are checked
    # bit for bit through + r2; the LayerNorm branch (out of scope: not exact on any data) only has to be finite.  Its Linear: 8 tiles -> 5 slices of the 40 stages
    add("t128n64-split-s4-reduce-writes-layer-norm-image", "t128", 1000, 1024, 1280,
        {"lin_t128n64": 2, "lin_splitk_reduce_ln": 1, "lin_splitk_reduce": 1, "split_k_gemms": 2, "fused_ln_reduce": 1, "fused_linear": 1}, epi="ln_next", S=4, tile="t128n64")


# ------------------------------------------------------------------------------------------------ the default policy on 256 CUs
def _policy_cases():
    P = dict(policy=True, fast=True)
    # 12 x 16 = 192 tiles of 256 x 256, 64 stages; the last row tile ragged
    add("t256p-default-policy-3000x2048-to-4096-bias+res", "pipe", 3000, 2048, 4096, g16_routes("t256p", "bias+res", 4096), epi="bias+res", tile="t256p", **P)
    # 24 x 8 = 192 tiles of 256 x 192 (144 of 256 x 256 would not fill the chip)
    add("t192p-default-policy-6100x2048-to-1536-bias", "pipe", 6100, 2048, 1536, g16_routes("t192p", "bias", 1536), epi="bias", tile="t192p", **P)
    # ... a width that is a multiple of 64 only: 16 x 12 tiles, the last column tile 64 wide (wblk_lim clamps its weight fetches)
    add("t192p-default-policy-ragged-width-4096x2048-to-2176-res+bias", "pipe", 4096, 2048, 2176, g16_routes("t192p", "res+bias", 2176), epi="res+bias", tile="t192p", **P)
    # the padded-256 width: 2432 = 9.5 tiles; 20 x 10 = 200 tiles fill a round, 20 x 13 of 256 x 192 would leave the second one mostly empty
    add("t256p-default-policy-padded-width-5100x2048-to-2432-bias", "pipe", 5100, 2048, 2432, g16_routes("t256p", "bias", 2432), epi="bias", tile="t256p", **P)
    # 24 x 8 = 192 tiles of 256 x 320, 32 stages
    add("t320-default-policy-6100x1024-to-2560-bias+res", "pipe", 6100, 1024, 2560, g16_routes("t320", "bias+res", 2560), epi="bias+res", tile="t320", **P)
    # ... and its K slices: 8 x 8 = 64 tiles x 4 slices of 20 stages
    add("t320-default-policy-k-slices-s4-2048x2560-to-2560-bias+res", "pipe", 2048, 2560, 2560, g16_routes("t320", "bias+res", 2560, split="reduce"), epi="bias+res", S=4, tile="t320", **P)
    # the round-cost model: 86 x 9 = 774 tiles of 128 x 128 are two rounds, 43 x 9 = 387 of 256 x 128 one
    add("t256-default-policy-11000x72-to-1152-bias", "t256", 11000, 72, 1152, g16_routes("t256", "bias", 1152), epi="bias", tile="t256", **P)
    # 128 x 4 = 512 tiles of 256 x 160 are one round of eight-wave workgroups against two rounds of either 128-column tile
    add("t160n-default-policy-32700x64-to-640-none", "t256", 32700, 64, 640, g16_routes("t160n", "none", 640), epi="none", tile="t160n", **P)
    # ... and 128 x 2 = 256 of them (one per CU) where 768 tiles of 128 x 128 are exactly one round
    add("t160n-default-policy-one-per-cu-32700x64-to-320-bias", "t256", 32700, 64, 320, g16_routes("t160n", "bias", 320), epi="bias", tile="t160n", **P)
    # GEGLU on the 16-column interleave: 8 x 32 = 256 tiles of 256 x 320, one round
    add("t320-default-policy-geglu16-2048x1280-to-10240", "pipe", 2048, 1280, 10240,
        {"lin_t320": 2, "lin_geglu16": 1, "fused_geglu": 1, "fused_linear_geglu": 1, "fused_linear": 1, "lin_splitk_reduce": 1, "split_k_gemms": 1}, epi="geglu", tile="t320", **P)
    # (its identity FF2, 2048 x 5120 -> 5120: 8 x 16 = 128 tiles of 256 x 320 x 2 K slices of 80 stages)
    # row split (tail_split = 1): 17 x 16 = 272 tiles = one whole round of 256 + the last 204 rows on 128 x 128 tiles (row_base = 4096)
    add("t256p-row-split-4300x2048-to-4096-bias+res", "pipe", 4300, 2048, 4096, {"lin_rowsplit_main": 1, "lin_t128": 1}, epi="bias+res", tile="t256p", opts={"tail_split": 1}, **P)
    # stream-K, every candidate (mode 2): 13 x 16 = 208 tiles cut over 256 persistent workgroups; hybrid (mode 3): 24 x 16 = 384 tiles = one whole round + 128 tiles cut
    add("t256p-stream-k-mode-2-3300x2048-to-4096-bias+res", "pipe", 3300, 2048, 4096, {"lin_streamk": 1, "split_k_gemms": 1, "split_k_inlaunch": 1}, epi="bias+res", tile="t256p",
        opts={"streamk": 2}, **P)
    add("t256p-stream-k-mode-3-6100x2048-to-4096-bias", "pipe", 6100, 2048, 4096, {"lin_streamk": 1, "split_k_gemms": 1, "split_k_inlaunch": 1}, epi="bias", tile="t256p",
        opts={"streamk": 3}, **P)
    # ... and the fused epilogues in stream-K's last-arriver combine: the DiT gate over 3 images of 1100 tokens, GELU -> f16 image (its identity fc2, 3300 x 4096 ->
    # 4096, is a stream-K launch of the same grid itself), GEGLU on the 128-column pairing (gemm16_geglu_mode: the 256 x 256 tile takes the paired image; its identity
    # FF2, 3300 x 2048 -> 2048: 26 x 16 tiles of 128 x 128)
    sk = {"lin_streamk": 1, "split_k_gemms": 1, "split_k_inlaunch": 1}
    add("t256p-stream-k-mode-2-3300x2048-to-4096-gate-3-images", "pipe", 3300, 2048, 4096, {**sk, "fused_gate": 1}, epi="gate", batch=(3, 1), tile="t256p", opts={"streamk": 2}, **P)
    add("t256p-stream-k-mode-2-3300x2048-to-4096-gelu", "pipe", 3300, 2048, 4096, {"lin_streamk": 2, "split_k_gemms": 2, "split_k_inlaunch": 2, "fused_gelu": 1, "fused_linear": 1},
        epi="gelu", tile="t256p", opts={"streamk": 2}, **P)
    add("t256p-stream-k-mode-2-3300x2048-to-4096-geglu", "pipe", 3300, 2048, 4096,
        {**sk, "lin_geglu_pair": 1, "fused_geglu": 1, "fused_linear_geglu": 1, "fused_linear": 1, "lin_t128": 1}, epi="geglu", tile="t256p", opts={"streamk": 2}, **P)
    # raw q8_0 / q4_0 rows dequantised in the main loop (above 512 rows, on the tile the f16 image would take), ragged last row tiles
    for wt in ("q8_0", "q4_0"):
        q = wt[:2]
        add(f"t256p-in-loop-dequant-{wt}-3000x2048-to-4096-bias+res", "pipe", 3000, 2048, 4096, {f"lin_t256p_{q}": 1, "qinloop_linears": 1}, wtype=wt, epi="bias+res", tile="t256p", **P)
        add(f"t192p-in-loop-dequant-{wt}-6100x2048-to-1536-bias", "pipe", 6100, 2048, 1536, {f"lin_t192p_{q}": 1, "qinloop_linears": 1}, wtype=wt, epi="bias", tile="t192p", **P)


# ------------------------------------------------------------------------------------------------ the raw-block kernels
def _quantised_cases():
    # the just-in-time f16 image (jit_qimages = 1): 5 x 6 tiles of 128 x 64, M = 200 pads the image rows to 256
    for wt, rows, K, M, e in (("q8_0", 640, 512, 384, "bias"), ("q4_0", 1030, 256, 200, "bias+res")):
        tile = "t128n64" if M % 64 == 0 else "t128"
        add(f"jit-image-{wt}-{rows}x{K}-to-{M}-{e}", "t128", rows, K, M, merge(g16_routes(tile, e, M), {"lin_wswz_q": 1, "jit_images": 1}), wtype=wt, epi=e, tile=tile,
            opts={"jit_qimages": 1, "splitk_target": 1})
    # k_qgemm16: the row classes of RB (3 rows reach it with qgemv off), unsplit (K = 256: one segment) and split (K = 1024: 2 slices of 2 segments)
    epis = iter(["bias", "bias+res", "none", "res+bias", "scale", "bias", "bias+res", "bias"] * 4)
    for rows in (3, 32, 33, 64, 65, 128, 129, 512):
        rb = 1 if rows <= 32 else 2   # RB 4 only from 512 workgroups on (below) or by option
        for wt, K, M, S in (("q8_0", 256, 200, 1), ("q4_0", 1024, 130, 2)):
            e = next(epis)
            r = {f"lin_qgemm16_rb{rb}": 1, "qgemm16_linears": 1, "lin_qgemm16_reduce": 1 if S > 1 else 0}
            add(f"qgemm16-{wt}-{rows}x{K}-to-{M}-s{S}-{e}", "qgemm16", rows, K, M, r, wtype=wt, epi=e, S=S, tile="t128", opts={"qgemv": 0} if rows == 3 else {})
    for rows, wt in ((65, "q8_0"), (128, "q4_0"), (129, "q8_0")):
        add(f"qgemm16-rb4-by-option-{wt}-{rows}x512-to-200-bias+res", "qgemm16", rows, 512, 200, {"lin_qgemm16_rb4": 1, "qgemm16_linears": 1}, wtype=wt, epi="bias+res",
            opts={"qgemm16_rb": 4})
    add("qgemm16-rb4-default-policy-q4_0-512x256-to-16384-bias", "qgemm16", 512, 256, 16384, {"lin_qgemm16_rb4": 1, "qgemm16_linears": 1}, wtype="q4_0", epi="bias")
    # gate and GELU in k_qgemm16's epilogue (3 images of 43 tokens; fc1 -> GELU -> the f16 identity fc2 on 128 x 64 tiles)
    add("qgemm16-q8_0-129x256-to-200-gate", "qgemm16", 129, 256, 200, {"lin_qgemm16_rb2": 1, "qgemm16_linears": 1, "fused_gate": 1}, wtype="q8_0", epi="gate", batch=(3, 1))
    add("qgemm16-q4_0-77x256-to-192-gelu", "qgemm16", 77, 256, 192, {"lin_qgemm16_rb2": 1, "qgemm16_linears": 1, "fused_gelu": 1, "fused_linear": 1, "lin_t128n64": 1},
        wtype="q4_0", epi="gelu", opts={"splitk_target": 1})
    # k_qgemv / k_qgemv_rows: every row class at K = 256 and at its LDS limit
    epis = iter(["bias", "bias+res", "none", "res+bias", "scale", "presilu"] * 4)
    for rows, Kmax, route, o in ((1, 12288, "lin_qgemv", {}), (2, 12288, "lin_qgemv", {}), (3, 16384, "lin_qgemv_rows4", {}), (4, 16384, "lin_qgemv_rows4", {}),
                                 (8, 8192, "lin_qgemv_rows8", {"qgemv_max_rows": 16}), (16, 4096, "lin_qgemv_rows16", {"qgemv_max_rows": 16})):
        for wt, K, M in (("q8_0", 256, 33), ("q4_0", Kmax, 100)):
            e = next(epis)
            add(f"qgemv-{wt}-{rows}x{K}-to-{M}-{e}", "gemv", rows, K, M, {route: 1, "qgemv_linears": 1, "fused_presilu": 1 if e == "presilu" else 0}, wtype=wt, epi=e, opts=o)
    # three modulation Linears of SiLU(vec) in ONE k_qgemv launch (plan_hoisted_mod); the members' outputs side by side are the case's output
    for wt, rows in (("q8_0", 1), ("q4_0", 2)):
        add(f"qgemv-group-of-3-{wt}-{rows}x256-to-3x100", "gemv", rows, 256, 300, {"lin_qgemv_group": 1, "hoisted_mod_linears": 3, "qgemv_linears": 3, "fused_presilu": 3, "fused_linear": 2},
            wtype=wt, epi="presilu", kind="group")


def _float_gemv_cases():
    # k_fgemv: 1, 4, 5, 16 rows, K = 8 and K at the 96 KB limit of the staged rows
    epis = iter(["bias", "bias+res", "presilu", "res+bias", "none", "scale", "presilu", "bias"] * 2)
    for rows in (1, 4, 5, 16):
        r4 = (rows + 3) // 4 * 4
        for wt, esz in (("f16", 2), ("f32", 4)):
            for K, M in ((8, 33), (96 * 1024 // (r4 * esz), 100)):
                e = next(epis)
                add(f"fgemv-{wt}-{rows}x{K}-to-{M}-{e}", "gemv", rows, K, M, {f"lin_fgemv_{wt}": 1, "fgemv_linears": 1, "fused_presilu": 1 if e == "presilu" else 0}, wtype=wt, epi=e)


def _grouped_cases():
    # k / v of one context in ONE launch_gemm16_linear_multi with f32 head-major outputs (plan_sibling_group): 2 images of 77 tokens, 8 heads of 40; 2 heads of 65
    add("multi-2-siblings-154x320-to-320-head-major", "t128", 154, 320, 320, {"lin_multi": 1, "lin_t128n64": 1, "fused_sibling_linears": 1, "head_major_gemms": 2, "fused_linear": 1},
        kind="multi", batch=(2, 1), tile="t128n64")
    add("multi-2-siblings-387x72-to-130-head-major", "t128", 387, 72, 130, {"lin_multi": 1, "lin_t128": 1, "fused_sibling_linears": 1, "head_major_gemms": 2, "fused_linear": 1},
        kind="multi", batch=(3, 1), tile="t128")


_tile_cases()
_split_cases()
_policy_cases()
_quantised_cases()
_float_gemv_cases()
_grouped_cases()
assert len({c.id for c in CASES}) == len(CASES), "case ids are unique"
HEADS = {320: (40, 8), 130: (65, 2)}   # multi: M -> (d, H)


# ------------------------------------------------------------------------------------------------ data, reference, graph
def make_case_data(case: Case, seed: int) -> dict:
    """x in -4 .. 4 (-1 .. 1 in front of a transcendental: the pre-activations stay small), w in -2 .. 2 (quantised: linear_ref.make_quantised), bias in -64 .. 64,
    residual in -8 .. 8, gate in -2 .. 2; no zero in the first column of x and w, on the last row and the last weight row"""
    rng = np.random.default_rng(seed)
    rows, K, M, wt, epi = case.rows, case.K, case.M, case.wtype, case.epi
    small = epi in ("gelu", "geglu")
    x = R.ints(rng, -1, 1, (rows, K)) if small else R.ints(rng, -4, 4, (rows, K))
    x[:, 0] = R.nonzero_ints(rng, -1, 1, rows) if small else R.nonzero_ints(rng, -4, 4, rows)
    x[-1] = R.nonzero_ints(rng, -1, 1, K) if small else R.nonzero_ints(rng, -4, 4, K)
    d = {"x": x}
    nw = {"linear": 1, "multi": 2, "group": 3}[case.kind]
    Mw = M // 3 if case.kind == "group" else M
    ws = []
    for _ in range(nw):
        if epi == "presilu":
            w = R.one_per_row(rng, Mw, K, wt)
        elif wt in ("q8_0", "q4_0"):
            w = R.make_quantised(rng, Mw, K, wt)
        else:
            lim = 1 if epi == "geglu" else 2   # (value x gate products stay far inside f16's range)
            w = R.ints(rng, -lim, lim, (Mw, K))
            w[:, 0] = R.nonzero_ints(rng, -lim, lim, Mw)
            w[-1] = R.nonzero_ints(rng, -lim, lim, K)
        ws.append(w)
    d["w"] = ws[0] if nw == 1 else ws
    if epi not in ("none",) and case.kind != "multi" and not (epi == "presilu" and case.kind == "linear"):
        d["bias"] = R.nonzero_ints(rng, -64, 64, (M,))
    if epi in ("bias+res", "res+bias", "gate", "ln_next"):
        d["residual"] = R.ints(rng, -8, 8, (rows, M))
    if epi == "gate":
        d["gate"] = R.nonzero_ints(rng, -2, 2, (case.batches, M))
    if epi == "ln_next":
        d["ln_w"], d["ln_b"] = R.ints(rng, 1, 2, (M,)), R.ints(rng, -2, 2, (M,))
        d["w2"] = R.ints(rng, -1, 1, (64, M))
        d["r2"] = R.ints(rng, -8, 8, (rows, M))
    return d


_cache: OrderedDict = OrderedDict()


def case_reference(case: Case):
    """(operands, (reference float64, pre-activations or None)) of the case, computed once per shape, type and epilogue"""
    key = (case.kind, case.rows, case.K, case.M, case.wtype, case.epi, case.batches)
    if key not in _cache:
        d = make_case_data(case, zlib.crc32(repr(key).encode()))
        _cache[key] = (d, reference(case, d))
        while len(_cache) > 2:   # the chip-filling cases hold ~200 MB each
            _cache.popitem(last=False)
    return _cache[key]


def reference(case: Case, d: dict, mutant=None):
    """linear_ref of the case's operands (the plain product is computed once per case and shared with the mutant runs); asserts the exactness budget"""
    bm, bn = TILE_SHAPE[case.tile]
    w = d["w"]
    if case.kind == "multi":      # the two siblings' outputs side by side
        order = (1, 0) if mutant == "siblings_swapped" else (0, 1)
        parts = [R.linear_ref(d["x"], w[i], case.wtype, mutant=None if mutant == "siblings_swapped" else mutant, bm=bm, bn=bn)[0] for i in order]
        R.check_exact(d["x"], np.concatenate(w))
        return np.concatenate(parts, axis=1), None
    if case.kind == "group":
        w = np.concatenate(w)
    bias, res, gate = d.get("bias"), d.get("residual"), d.get("gate")
    extra = sum(float(np.abs(a).max()) for a in (bias, res, d.get("r2")) if a is not None)
    ux, uw = (R.PRE_SCALE if case.epi == "scale" else 1.0), (0.25 if case.wtype in ("q8_0", "q4_0") else 1.0)
    if case.epi == "presilu":
        R.check_exact(np.ones(1), w, unit_w=uw, extra=extra)   # one product per output
    else:
        lin = R.check_exact(d["x"], w, unit_x=ux, unit_w=uw)   # the accumulators, then (acc * scale + bias) * gate + residual
        b = (lin * (R.POST_SCALE * ux if case.epi == "scale" else 1.0) + (float(np.abs(bias).max()) if bias is not None else 0.0)) * (float(np.abs(gate).max()) if gate is not None else 1.0)
        b += sum(float(np.abs(a).max()) for a in (res, d.get("r2")) if a is not None)
        if not b / (ux * uw) < R.EXACT_BOUND:
            raise ValueError(f"{case.id}: exactness bound broken by the epilogue: {b}")
    if "_acc" not in d:
        w64 = R._weights64(w, case.wtype, None)
        d["_acc"] = R.matmul(R.prepare(d["x"], case.epi), w64, case.fast)
        if case.fast:   # the float32 matmul is exact under the bound asserted above: int64 on the rows around the tile seams says so too
            rs = np.unique(np.clip([0, 255, 256, case.rows // 2, case.rows - 257, case.rows - 256, case.rows - 1], 0, case.rows - 1))
            xi, wi = np.rint(R.prepare(d["x"][rs], case.epi) / ux).astype(np.int64), np.rint(w64 / uw).astype(np.int64)
            assert np.array_equal((xi @ wi.T) * (ux * uw), d["_acc"][rs]), f"{case.id}: the float32 reference is not exact"
    out, p = R.linear_ref(d["x"], w, case.wtype, epi=case.epi, bias=bias, residual=res, gate=gate, batches=case.batches, mutant=mutant, S=case.S, bm=bm, bn=bn, fast=case.fast,
                          true_acc=d["_acc"])
    if case.epi == "ln_next":
        out = out + d["r2"]
    if case.epi in ("gelu", "geglu") and mutant is None and not float(np.abs(out).max()) < R.F16_MAX / 2:   # (the pre-activations are exact in f32; the image must stay finite)
        raise ValueError(f"{case.id}: image values up to {float(np.abs(out).max())} do not fit f16")
    return out, p


def out_shape(case: Case, cols: int):
    n2, n3 = case.batch
    return (case.rows, cols) if case.batch == (1, 1) else (n2, case.rows // n2, cols) if n3 == 1 else (n3, n2, case.rows // (n2 * n3), cols)


def build(case: Case, d: dict, g: Graph, L):
    """the case's graph -> its output node(s)"""
    rows, K, M, e = case.rows, case.K, case.M, case.epi
    wt = WTYPES[case.wtype]
    shp = lambda a, c: np.ascontiguousarray(a).reshape(out_shape(case, c))
    if case.strided:    # rows of K floats inside rows of 2 K
        wide = np.concatenate([d["x"], -d["x"]], axis=1)
        xw = g.input(shp(wide, 2 * K))
        s = tensor_struct(xw)
        ne = [int(s.ne[i]) for i in range(4)]
        x = L.ggml_view_4d(g.ctx, xw, K, ne[1], ne[2], ne[3], int(s.nb[1]), int(s.nb[2]), int(s.nb[3]), 0)
    else:
        x = g.input(shp(d["x"], K))
    if case.kind == "multi":
        dh, H = HEADS[M]
        n2 = case.batch[0]
        outs = []
        for w in d["w"]:
            y = L.ggml_mul_mat(g.ctx, g.weight(w, wt), x)
            y = L.ggml_reshape_4d(g.ctx, y, dh, H, rows // n2, n2)
            outs.append(L.ggml_cont(g.ctx, L.ggml_permute(g.ctx, y, 0, 2, 1, 3)))   # [d, L, H, N]
        return outs
    if case.kind == "group":
        outs, m = [], M // 3
        for i, w in enumerate(d["w"]):
            y = L.ggml_mul_mat(g.ctx, g.weight(w, wt), L.ggml_silu(g.ctx, x))
            outs.append(L.ggml_add_inplace(g.ctx, y, g.weight(d["bias"][i * m:(i + 1) * m], F32)))
        return outs
    if e == "scale":
        x = L.ggml_scale(g.ctx, x, R.PRE_SCALE)
    if e == "presilu":
        x = L.ggml_silu(g.ctx, x)
    y = L.ggml_mul_mat(g.ctx, g.weight(d["w"], wt), x)
    if e == "scale":
        y = L.ggml_scale(g.ctx, y, R.POST_SCALE)
    if "bias" in d:
        y = L.ggml_add_inplace(g.ctx, y, g.weight(d["bias"], F32))
    if e in ("bias+res", "ln_next"):
        y = L.ggml_add(g.ctx, y, g.input(shp(d["residual"], M)))
    elif e == "res+bias":
        y = L.ggml_add(g.ctx, g.input(shp(d["residual"], M)), y)
    elif e == "gate":
        n2 = case.batch[0]
        gt = g.input(d["gate"].reshape(n2, 1, M))
        y = L.ggml_add(g.ctx, g.input(shp(d["residual"], M)), L.ggml_mul(g.ctx, y, gt))
    elif e == "gelu":
        y = L.ggml_mul_mat(g.ctx, g.weight(np.eye(M, dtype=np.float32), F16), L.ggml_gelu_inplace(g.ctx, y))
    elif e == "geglu":
        inner = M // 2
        s = tensor_struct(y)
        ne, nb = [int(s.ne[i]) for i in range(4)], [int(s.nb[i]) for i in range(4)]
        lo = L.ggml_view_4d(g.ctx, y, inner, ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], 0)
        hi = L.ggml_view_4d(g.ctx, y, inner, ne[1], ne[2], ne[3], nb[1], nb[2], nb[3], inner * 4)
        h = L.ggml_mul(g.ctx, lo, L.ggml_gelu_inplace(g.ctx, L.ggml_cont(g.ctx, hi)))
        y = L.ggml_mul_mat(g.ctx, g.weight(np.eye(inner, dtype=np.float32), F16), h)
    if e == "ln_next":
        t = L.ggml_norm(g.ctx, y, 1e-5)
        t = L.ggml_mul_inplace(g.ctx, t, g.weight(d["ln_w"], F32))
        t = L.ggml_add_inplace(g.ctx, t, g.weight(d["ln_b"], F32))
        t = L.ggml_mul_mat(g.ctx, g.weight(d["w2"], F16), t)
        return [L.ggml_add(g.ctx, y, g.input(d["r2"])), t]
    return y


def run_case(case: Case, device: str, L) -> np.ndarray:
    """-> the case's output as [rows, columns] float32"""
    d, _ = case_reference(case)
    with Graph(device) as g:
        outs = build(case, d, g, L)
        if case.kind == "multi":
            dh, H = HEADS[case.M]
            n2 = case.batch[0]
            res = g.run(*outs)      # each [N, H, L, d] -> token-major [rows, M]
            return np.concatenate([o.reshape(n2, H, case.rows // n2, dh).transpose(0, 2, 1, 3).reshape(case.rows, case.M) for o in res], axis=1)
        if case.kind == "group":
            return np.concatenate([o.reshape(case.rows, -1) for o in g.run(*outs)], axis=1)
        if case.epi == "ln_next":
            z, t = g.run(*outs)
            assert np.isfinite(t).all(), f"{case.id}: the LayerNorm branch is not finite"
            return z.reshape(case.rows, -1)
        return g.run(outs).reshape(case.rows, -1)


def describe_difference(case: Case, out: np.ndarray, want: np.ndarray, bad_mask: np.ndarray) -> str:
    """first differing (row, column), the count, and the bounding box in units of the case's tile: says "last column tile", "tail rows" or "everything" at a glance"""
    bm, bn = TILE_SHAPE[case.tile]
    bad = np.argwhere(bad_mask)
    r, c = bad[0]
    r0, r1, c0, c1 = bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max()
    return (f"{case.id}: {len(bad)} of {want.size} elements differ; first at (row, column) = ({r}, {c}): got {out[r, c]!r}, reference {want[r, c]!r}\n"
            f"  bounding box rows {r0}..{r1}, columns {c0}..{c1} = row tiles {r0 // bm}..{r1 // bm} of {(want.shape[0] + bm - 1) // bm} ({bm} rows), "
            f"column tiles {c0 // bn}..{c1 // bn} of {(want.shape[1] + bn - 1) // bn} ({bn} columns, tile {case.tile})")


def tolerance(case: Case, want: np.ndarray, p, d: dict):
    """None (bit for bit) or the elementwise bar behind a transcendental epilogue as its two terms (f16 rounding of the image value, f32 error of the function)"""
    if case.epi == "gelu":
        return R.transcendental_terms(want, p)
    if case.epi == "geglu":
        v, gt = p
        return R.transcendental_terms(want, gt, np.maximum(1.0, np.abs(v)))
    if case.epi == "presilu":
        w = np.concatenate(d["w"]) if case.kind == "group" else d["w"]
        col = np.abs(w).argmax(axis=1)
        wv = np.abs(w).max(axis=1)
        t1, t2 = R.transcendental_terms(R.silu64(p[:, col]), p[:, col], wv[None, :])
        return t1, t2 + (2.0 ** -24 * np.abs(want) if "bias" in d else 0.0)   # the epilogue's f32 add of the bias rounds once more
    return None


# transcendental epilogue -> [largest |error| / first term where that term is the larger one, largest |error| / second term elsewhere, largest |error| / bar], over the
# cases check_case saw in this process
# (presilu with a bias — the grouped launch — adds 2^-24 |reference| to the issue's bar: the half f32 ulp of the one rounded add of the bias behind the exact product)
worst: dict = {}


def check_case(case: Case, out: np.ndarray) -> None:
    d, (want, p) = case_reference(case)
    assert out.shape == want.shape == (case.rows, (2 if case.kind == "multi" else 1) * case.out_cols), (out.shape, want.shape)
    terms = tolerance(case, want, p, d)
    if terms is None:
        w32 = want.astype(np.float32)
        if not np.array_equal(out, w32):
            raise AssertionError(describe_difference(case, out, w32, out != w32))
        return
    t1, t2 = terms
    tol = t1 + t2
    err = np.abs(out.astype(np.float64) - want)
    first = t1 >= t2
    figs = [float((err / t1)[first].max()) if first.any() else 0.0, float((err / t2)[~first].max()) if (~first).any() else 0.0, float((err / tol).max())]
    worst[case.epi] = [max(a, b) for a, b in zip(worst.get(case.epi, [0.0] * 3), figs)]
    print(f"{case.id}: largest |error| = {figs[0]:.3f} f16 ulps of the image value where the rounding term governs, {figs[1]:.3f} of the 2^-18 max(1, |p|) term elsewhere, "
          f"{figs[2]:.3f} of the bar")
    if not (err <= tol).all():
        raise AssertionError(describe_difference(case, out, want, ~(err <= tol)) + f"\n  largest |error| / bar = {figs[2]:.3f}")
