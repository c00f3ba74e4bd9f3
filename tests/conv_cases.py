"""The case table of the conv route tests: each case is ONE convolution (ggml_conv_2d's IM2COL .. CONT chain with its epilogue nodes, or a CONV_2D node) on
integer-valued data, with the kernel route it must take stated as launch-counter moves.  tests/test_conv_ref_cpu.py runs every case on the CPU oracle and
against the mutants of conv_ref.py (no GPU needed); tests/test_gpu_conv_routes.py runs it on the product backend, bit for bit, and asserts the counters.

Shapes are the smallest that reach a route, derived from the planner's own rules (kernels/conv3w.hip conv3w_plan; kernels/gemm16.hip g16_pick_tile,
g16_t320_split, gemm16_split_k, gemm16_split_plan, gemm16_worder_rows) and confirmed by the counters on the GPU:

  window kernel (family "c3w")   3x3 / stride 1, W in {16, 32, 64, 128}, H * W a multiple of 256, IC >= 64, OC a multiple of 320 or 256, and a launch that fills
                                 the chip: >= 192 tiles of 256 positions x BN columns filling >= 75 % of their rounds of 256, or K slices over the 32-channel blocks
                                 with tiles * S >= 128 and at least conv3w_min_blocks (8; conv3w_min_blocks_deep = 5 up to 64 tiles) blocks per slice
  gemm16 conv tiles              OC <= 64: the 64-column form of the 128-row tile.  256 x 256 pipelined (t256p): OC % 256 == 0 and not % 320, >= 64 K stages of 32,
                                 >= 192 tiles; 256 x 320 pipelined (t320): OC % 320 == 0, >= 16 K stages, >= 192 tiles, or its K slices (8 .. 191 tiles, >= 20 stages per
                                 slice); 256 x 128 (t256) / 256 x 160 (t160, t160n) by the round-cost model; 128 x 128 (t128) otherwise; t256w only by option.
                                 Option gemm16_tile forces a tile where the default policy would need a workload-sized launch; the pipelined tiles then keep at least the
                                 K stages the default policy asks of them (IC = 64 / 1x1 IC = 512 for t320, IC = 256 / 1x1 IC = 2048 for t256p) and run unsplit
                                 (splitk_target = 1), as they do under the default policy
  families                       "c3w", "pipe" (t320, t256p), "t256" (t256, t256w, t160, t160n), "t128" (t128, t128n64): every epilogue appears on each, and on a split launch

83 cases."""
from __future__ import annotations

import zlib
from collections import OrderedDict
from dataclasses import dataclass, field

import numpy as np

import conv_ref
from ggml_graph import F16, F32, Graph

OPTION_DEFAULTS = {"conv3w": 1, "conv3w_min_blocks": 8, "conv3w_min_blocks_deep": 5, "conv3w_prio": 3, "conv_wmajor": 1, "gemm16_tile": -1, "splitk_target": 384,
                   "splitk_inkernel": 0, "conv_tap_major": 0}
T128, T256, T256W, T160, T160N, T320, T256P = range(7)   # values of option gemm16_tile
CONV_ROUTE_FIELDS = ("c3w_tw16_bn256 c3w_tw16_bn320 c3w_tw32_bn256 c3w_tw32_bn320 c3w_tw64_bn256 c3w_tw64_bn320 c3w_tw128_bn256 c3w_tw128_bn320 "
                     "g16_conv_t128 g16_conv_t128n64 g16_conv_t256 g16_conv_t256w g16_conv_t160 g16_conv_t160n g16_conv_t320 g16_conv_t256p "
                     "g16_conv_splitk_reduce g16_conv_wmajor").split()
# ... and the planner's counters a one-conv graph can move
ROUTE_FIELDS = CONV_ROUTE_FIELDS + "window_convs split_k_gemms split_k_inlaunch fused_gn_stats fused_conv_scale fused_chan_add".split()
EPILOGUES = {"none": (), "bias": ("bias",), "bias+res": ("bias", "res"), "res+bias": ("bias", "res_first"), "scale+bias": ("scale", "bias"), "emb": ("bias", "emb")}
PRE_SCALE, POST_SCALE = 0.125, 8.0   # the Conv2d scale of the scale+bias epilogue: SCALE s -> conv -> SCALE 1 / s


@dataclass
class Case:
    id: str
    family: str                # "c3w" | "pipe" | "t256" | "t128"
    N: int
    IC: int
    OC: int
    H: int                     # the input map (before the upscale)
    W: int
    ks: int = 3
    stride: int = 1
    upscale: bool = False
    epi: str = "none"          # key of EPILOGUES
    opts: dict = field(default_factory=dict)     # backend options of the run (restored to OPTION_DEFAULTS afterwards)
    routes: dict = field(default_factory=dict)   # counter -> moves expected; every other field of ROUTE_FIELDS must not move
    slices: int = 1            # K slices of the launch (what drop_last_block_of_a_slice cuts by)
    direct: bool = False       # a CONV_2D node (ggml_conv_2d_direct) instead of the IM2COL chain

    @property
    def epilogue(self):
        return EPILOGUES[self.epi]

    @property
    def out_hw(self):
        u, p = (2 if self.upscale else 1), self.ks // 2
        return (self.H * u + 2 * p - self.ks) // self.stride + 1, (self.W * u + 2 * p - self.ks) // self.stride + 1


CASES: list[Case] = []


def add(cid, family, N, IC, OC, H, W, routes, **k):
    CASES.append(Case(cid, family, N, IC, OC, H, W, routes=routes, **k))


def _c3w(tw, bn, S=1, wmajor=False):
    r = {f"c3w_tw{tw}_bn{bn}": 1, "window_convs": 1}
    if S > 1:
        r.update(split_k_gemms=1, g16_conv_splitk_reduce=1)
    if wmajor:
        r["g16_conv_wmajor"] = 1
    return r


def _g16(tile, split=None, wmajor=False, **more):
    r = {"g16_conv_" + tile: 1}
    if split == "reduce":
        r.update(split_k_gemms=1, g16_conv_splitk_reduce=1)
    elif split == "inlaunch":
        r.update(split_k_gemms=1, split_k_inlaunch=1)
    if wmajor:
        r["g16_conv_wmajor"] = 1
    r.update(more)
    return r


def _epi_counters(epi):
    return {"scale+bias": {"fused_conv_scale": 1}, "emb": {"fused_chan_add": 1}}.get(epi, {})


# ------------------------------------------------------------------------------------------------ the window kernel, default policy
def _window_cases():
    # every TW x BN instantiation unsplit: 96 images of exactly one 256-position tile (both halos are the zero page) x 2 column tiles = 192 workgroups
    one_tile = {16: (16, 16), 32: (8, 32), 64: (4, 64), 128: (2, 128)}   # TW -> (H, W)
    epis = iter(["none", "bias", "bias+res", "res+bias", "scale+bias", "emb", "bias", "none"])
    for tw, (h, w) in one_tile.items():
        for bn in (256, 320):
            e = next(epis)
            add(f"c3w-tw{tw}-bn{bn}-one-tile-images-{e}", "c3w", 96, 64, 2 * bn, h, w, {**_c3w(tw, bn), **_epi_counters(e)}, epi=e)
    # three tiles per image (first, middle, last; H > W and H < W), 32 images
    three = {16: (48, 16, 256, "bias+res"), 32: (24, 32, 320, "emb"), 64: (12, 64, 256, "scale+bias"), 128: (6, 128, 320, "res+bias")}
    for tw, (h, w, bn, e) in three.items():
        add(f"c3w-tw{tw}-bn{bn}-three-tile-images-{e}", "c3w", 32, 64, 2 * bn, h, w, {**_c3w(tw, bn), **_epi_counters(e)}, epi=e)
    # IC = 96 (padded to 128 with zero channels) and IC = 160 (padded to 192)
    for tw, (h, w, bn, ic, e) in {16: (48, 16, 320, 96, "bias"), 64: (12, 64, 320, 96, "none"), 32: (24, 32, 256, 160, "bias+res"), 128: (6, 128, 256, 160, "bias")}.items():
        add(f"c3w-tw{tw}-bn{bn}-ic{ic}-{e}", "c3w", 32, ic, 2 * bn, h, w, _c3w(tw, bn), epi=e)
    # K slices.  Under the default conv3w_min_blocks*: 64 tiles, 10 blocks -> 2 slices of 5
    add("c3w-split-default-policy-s2-res+bias", "c3w", 16, 320, 512, 16, 32, _c3w(32, 256, 2), epi="res+bias", slices=2)
    # ... and small ones with the least blocks per slice lowered to 2: 64 tiles x 2 slices of 2 blocks; 32 tiles x 4 slices of 2; 10 blocks over 4 slices (3, 3, 3, 1);
    # IC = 160: 6 blocks (the last one all padding) over 3 slices.  bias / residual / emb / the Conv2d scale are applied by the reduce pass
    deep2 = {"conv3w_min_blocks_deep": 2}
    add("c3w-split-s2-bias+res", "c3w", 16, 128, 640, 32, 16, _c3w(16, 320, 2), epi="bias+res", opts=deep2, slices=2)
    add("c3w-split-s4-emb", "c3w", 8, 256, 512, 8, 64, {**_c3w(64, 256, 4), "fused_chan_add": 1}, epi="emb", opts=deep2, slices=4)
    add("c3w-split-s4-uneven-10-blocks-scale+bias", "c3w", 2, 320, 640, 16, 128, {**_c3w(128, 320, 4), "fused_conv_scale": 1}, epi="scale+bias", opts=deep2, slices=4)
    add("c3w-split-s3-ic160-none", "c3w", 6, 160, 512, 32, 32, _c3w(32, 256, 3), epi="none", opts=deep2, slices=3)
    add("c3w-split-s4-bias", "c3w", 4, 256, 640, 16, 64, _c3w(64, 320, 4), epi="bias", opts=deep2, slices=4)
    add("c3w-split-s4-prio0-bias", "c3w", 8, 256, 640, 16, 32, _c3w(32, 320, 4), epi="bias", opts={**deep2, "conv3w_prio": 0}, slices=4)
    # weight-major workgroup order: a 16-wide map with 9 * OC >= 2 * N * H * W (4 row tiles x 8 column tiles x 4 slices)
    add("c3w-weight-major-s4-bias+res", "c3w", 4, 256, 2048, 16, 16, _c3w(16, 256, 4, wmajor=True), epi="bias+res", opts=deep2, slices=4)
    # nearest misses of the unsplit three-tile shape: each breaks one predicate of conv3w_plan and lands on a gemm16 tile
    add("c3w-miss-16x24-positions-not-256", "t128", 64, 64, 512, 24, 16, _g16("t128"), epi="bias")
    add("c3w-miss-w48", "t128", 32, 64, 512, 16, 48, _g16("t128"), epi="bias")
    add("c3w-miss-ic32", "t128", 96, 32, 512, 16, 16, _g16("t128"), epi="bias")
    add("c3w-miss-oc384-default-policy-t256", "t256", 9, 64, 384, 64, 64, _g16("t256"), epi="bias+res")
    add("c3w-miss-stride2", "t128", 32, 64, 512, 48, 16, _g16("t128", "reduce"), stride=2, epi="bias", slices=2)
    add("c3w-miss-upscaled-input", "t128", 32, 64, 512, 24, 8, _g16("t128"), upscale=True, epi="bias")
    add("c3w-miss-option-conv3w-0", "t128", 32, 64, 512, 48, 16, _g16("t128"), epi="bias", opts={"conv3w": 0})


# ------------------------------------------------------------------------------------------------ the gemm16 conv tiles
def _tile_cases():
    unsplit = {"splitk_target": 1}
    # per tile: (option value, family, IC, 1x1 IC, OC, epilogues of the four geometries)
    tiles = {"t128": (T128, "t128", 96, 96, 130, ("none", "bias+res", "scale+bias", "emb")),
             "t256": (T256, "t256", 96, 96, 130, ("bias", "res+bias", "emb", "scale+bias")),
             "t256w": (T256W, "t256", 64, 64, 128, ("bias+res", "none", "bias", "bias")),
             "t160": (T160, "t256", 64, 96, 160, ("none", "scale+bias", "bias+res", "bias")),
             "t160n": (T160N, "t256", 96, 64, 320, ("emb", "bias", "none", "res+bias")),
             "t320": (T320, "pipe", 96, 512, 320, ("bias+res", "none", "emb", "scale+bias")),
             "t256p": (T256P, "pipe", 256, 2048, 256, ("scale+bias", "emb", "res+bias", "bias"))}
    for name, (opt, fam, ic, ic1, oc, epis) in tiles.items():
        o = {**unsplit, "gemm16_tile": opt}
        # 3 images of 12 x 20 = 720 rows: 256-row tiles straddle the images at rows 256 and 512, the last tile is partial
        add(f"{name}-3x3-3-images-12x20-{epis[0]}", fam, 3, ic, oc, 12, 20, {**_g16(name), **_epi_counters(epis[0])}, epi=epis[0], opts=o)
        # stride 2 on an odd map, 13 x 9 -> 7 x 5, 8 images = 280 rows
        add(f"{name}-3x3-stride2-13x9-{epis[1]}", fam, 8, ic, oc, 13, 9, {**_g16(name), **_epi_counters(epis[1])}, stride=2, epi=epis[1], opts=o)
        add(f"{name}-1x1-{epis[2]}", fam, 3, ic1, oc, 12, 20, {**_g16(name), **_epi_counters(epis[2])}, ks=1, epi=epis[2], opts=o)
        # the deferred nearest x2 upscale folded into the gather: 6 x 10 -> 12 x 20
        add(f"{name}-upscale-6x10-3x3-{epis[3]}", fam, 3, ic, oc, 6, 10, {**_g16(name), **_epi_counters(epis[3])}, upscale=True, epi=epis[3], opts=o)
    # the 64-column form (OC <= 64, no option needed): OC = 4 and OC = 64
    add("t128n64-oc4-3x3-3-images-12x20-bias", "t128", 3, 96, 4, 12, 20, _g16("t128n64"), epi="bias", opts=unsplit)
    add("t128n64-oc64-3x3-stride2-13x9-bias+res", "t128", 8, 64, 64, 13, 9, _g16("t128n64"), stride=2, epi="bias+res", opts=unsplit)
    add("t128n64-oc64-1x1-none", "t128", 3, 96, 64, 12, 20, _g16("t128n64"), ks=1, epi="none", opts=unsplit)
    add("t128n64-oc4-upscale-6x10-3x3-bias", "t128", 3, 64, 4, 6, 10, _g16("t128n64"), upscale=True, epi="bias", opts=unsplit)
    # IC = 4 (60 zero channels in every 64-channel block)
    add("t128-ic4-oc130-bias", "t128", 3, 4, 130, 12, 20, _g16("t128"), epi="bias", opts=unsplit)
    add("t256-ic4-oc130-bias", "t256", 3, 4, 130, 12, 20, _g16("t256"), epi="bias", opts={**unsplit, "gemm16_tile": T256})
    # the smallest shapes the DEFAULT policy sends to the pipelined and the 256-row tiles (t256: c3w-miss-oc384 above)
    add("t256p-default-policy-16-images-32x48-bias", "pipe", 16, 256, 512, 32, 48, _g16("t256p"), epi="bias")
    add("t320-default-policy-16-images-32x48-bias+res", "pipe", 16, 64, 640, 32, 48, _g16("t320"), epi="bias+res")
    add("t160-default-policy-64-images-32x64-none", "t256", 64, 64, 160, 32, 64, _g16("t160"), epi="none")
    add("t160n-default-policy-10-images-47x47-bias", "t256", 10, 64, 480, 47, 47, _g16("t160n"), epi="bias")
    # split launches.  The tiny grid: 90 K stages over 8 slices of 12 (the last one 6), every epilogue through k_splitk_reduce; the same shape unsplit
    for e in ("bias+res", "emb", "scale+bias", "none", "res+bias"):
        add(f"t128-split-s8-90-stages-{e}", "t128", 3, 320, 130, 12, 20, {**_g16("t128", "reduce"), **_epi_counters(e)}, epi=e, slices=8)
    add("t128-same-shape-unsplit-bias+res", "t128", 3, 320, 130, 12, 20, _g16("t128"), epi="bias+res", opts=unsplit)
    add("t128-split-stride2-13x9-bias", "t128", 8, 320, 130, 13, 9, _g16("t128", "reduce"), stride=2, epi="bias", slices=8)
    add("t128n64-split-oc64-bias", "t128", 3, 320, 64, 12, 20, _g16("t128n64", "reduce"), epi="bias", slices=8)
    # combined in the launch by the last-arriving workgroup: 4 slices of 23, 23, 23, 21 stages
    add("t128-split-in-launch-s4-bias+res", "t128", 3, 320, 130, 12, 20, _g16("t128", "inlaunch"), epi="bias+res", opts={"splitk_inkernel": 1}, slices=4)
    # the 256 x 320 tile's own K slices (g16_t320_split): 32 tiles x 4 slices of 23, 23, 23, 21 stages, weight-major order
    add("t320-k-slices-s4-8-images-32x8-bias+res", "pipe", 8, 320, 1280, 32, 8, _g16("t320", "reduce", wmajor=True), epi="bias+res", slices=4)
    # K ordered (tap, channel block) instead of (channel block, tap)
    add("t320-tap-major-ic128-bias", "pipe", 3, 128, 320, 12, 20, _g16("t320"), epi="bias", opts={**unsplit, "gemm16_tile": T320, "conv_tap_major": 1})
    add("t128-tap-major-ic128-split-bias", "t128", 3, 128, 130, 12, 20, _g16("t128", "reduce"), epi="bias", opts={"conv_tap_major": 1}, slices=4)
    # CONV_2D nodes: no epilogue fusion, no split
    add("direct-3x3-oc130", "t128", 3, 96, 130, 12, 20, _g16("t128"), direct=True)
    add("direct-1x1-oc130", "t128", 3, 96, 130, 12, 20, _g16("t128"), ks=1, direct=True)


_window_cases()
_tile_cases()
assert len({c.id for c in CASES}) == len(CASES), "case ids are unique"


# ------------------------------------------------------------------------------------------------ data, reference, graph
_cache: OrderedDict = OrderedDict()   # geometry + epilogue -> (data, reference): cases that share both (the epilogue-less split / unsplit pairs) compute them once


def case_reference(case: Case):
    """(operands, conv_ref of them) of the case, computed once per geometry and epilogue"""
    key = (case.N, case.IC, case.OC, case.H, case.W, case.ks, case.stride, case.upscale, case.epilogue)
    if key not in _cache:
        d = conv_ref.make_case_data(case, zlib.crc32(repr(key).encode()))
        _cache[key] = (d, conv_ref.conv_ref(d["x"], d["w"], case.stride, case.ks // 2, **ref_kwargs(case, d)))
        while len(_cache) > 2:   # the large cases hold ~100 MB each
            _cache.popitem(last=False)
    return _cache[key]


def ref_kwargs(case: Case, d: dict) -> dict:
    k = dict(upscale2x=case.upscale, bias=d.get("bias"), chan_add=d.get("chan_add"), residual=d.get("residual"))
    if "scale" in case.epilogue:
        k.update(pre_scale=PRE_SCALE, post_scale=POST_SCALE)
    return k


def build(case: Case, d: dict, g: Graph, L):
    e, p, OC = case.epilogue, case.ks // 2, case.OC
    x = g.input(d["x"])
    if "scale" in e:
        x = L.ggml_scale(g.ctx, x, PRE_SCALE)
    if case.upscale:
        x = L.ggml_upscale(g.ctx, x, 2, 0)   # nearest
    conv = L.ggml_conv_2d_direct if case.direct else L.ggml_conv_2d
    y = conv(g.ctx, g.weight(d["w"], F16), x, case.stride, case.stride, p, p, 1, 1)
    if "scale" in e:
        y = L.ggml_scale(g.ctx, y, POST_SCALE)
    if "bias" in e:
        y = L.ggml_add_inplace(g.ctx, y, L.ggml_reshape_4d(g.ctx, g.weight(d["bias"], F32), 1, 1, OC, 1))
    if "emb" in e:   # the ResBlock's time-embedding branch: a small Linear, reshaped to [1, 1, OC, N]
        t = L.ggml_mul_mat(g.ctx, g.weight(d["emb_w"], F16), g.input(d["emb"]))
        t = L.ggml_add_inplace(g.ctx, t, g.weight(d["emb_b"], F32))
        y = L.ggml_add(g.ctx, y, L.ggml_reshape_4d(g.ctx, t, 1, 1, OC, case.N))
    if "res" in e:
        y = L.ggml_add(g.ctx, y, g.input(d["residual"]))
    if "res_first" in e:
        y = L.ggml_add(g.ctx, g.input(d["residual"]), y)
    return y


def run_case(case: Case, device: str, L) -> np.ndarray:
    d, _ = case_reference(case)
    with Graph(device) as g:
        return g.run(build(case, d, g, L))


def describe_difference(case: Case, out: np.ndarray, want: np.ndarray) -> str:
    """first differing (n, oc, oh, ow), the count, and the bounding box per image: says "halo", "tail tile" or "slice" at a glance"""
    bad = np.argwhere(out != want)
    n, oc, oh, ow = bad[0]
    lines = [f"{case.id}: {len(bad)} of {want.size} elements differ; first at (n, oc, oh, ow) = ({n}, {oc}, {oh}, {ow}): got {out[n, oc, oh, ow]}, reference {want[n, oc, oh, ow]}"]
    for img in np.unique(bad[:, 0])[:8]:
        b = bad[bad[:, 0] == img]
        lines.append(f"  image {img}: {len(b)} differ, oc {b[:, 1].min()}..{b[:, 1].max()}, oh {b[:, 2].min()}..{b[:, 2].max()}, ow {b[:, 3].min()}..{b[:, 3].max()}")
    return "\n".join(lines)


def check_case(case: Case, out: np.ndarray) -> None:
    _, want = case_reference(case)
    OH, OW = case.out_hw
    assert out.shape == want.shape == (case.N, case.OC, OH, OW), (out.shape, want.shape)
    if not np.array_equal(out, want):
        raise AssertionError(describe_difference(case, out, want))
    np.testing.assert_array_equal(out, want)
