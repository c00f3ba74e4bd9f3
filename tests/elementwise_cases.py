"""The case table of the glue-kernel route tests: each case builds a one- or two-node ggml graph, states its NumPy reference (elementwise_ref.py) and names
the kernel route of elementwise.hip it must take.  tests/test_elementwise_ref_cpu.py runs every case on the CPU oracle (that validates the references on a
machine without a GPU), tests/test_gpu_elementwise_routes.py runs it on the product backend and asserts the route counters.

A route's cases come in pairs: the smallest shape that lands on it, and its nearest miss (one predicate of the launcher broken), which must land on the
fall-back and give the same values."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

import elementwise_ref as ref
from ggml_graph import BF16, F16, F32, I32, Q4_0, Q8_0, dequant, tensor_struct

GRID_STRIDE_N = 4 * 4096 * 256 + 7   # grid_for caps a grid at 4096 blocks of 256 threads, 4 elements each on the float4 routes: every thread takes a second trip
TYPE_NAME = {F32: "f32", F16: "f16", BF16: "bf16", Q8_0: "q8_0", Q4_0: "q4_0"}
UNARY_ENUM = {"neg": "ggml_neg", "exp": "ggml_exp"}


@dataclass
class Case:
    id: str
    build: Callable            # (g, L) -> node, or (node, tensor to fetch instead of the node: the parent of an in-place view)
    want: Callable             # () -> expected array
    routes: dict = field(default_factory=dict)   # stat field -> launches expected; every other ew_bin_* / ew_copy_* / ew_concat_* field must not move
    check: str = "bits"        # "bits" | "bits_nan" (NaN payloads too) | "abs" (|out - ref| <= tol * max(1, max|ref|)) | "abs_plain" (<= tol) | "rel" (<= tol * |ref| per element)
    tol: float = 0.0
    oracle_tol: float | None = None   # the CPU oracle's own error where it is larger (ggml-cpu's f16 GELU tables)
    extra: Callable | None = None     # (out, want) -> None: further assertions on the result


def rng_for(case_id: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def np_permute(a: np.ndarray, ax) -> np.ndarray:
    """ggml_permute(a, ax0..ax3) on an array in reversed-ne order: result dimension ax[i] is source dimension i"""
    a4 = ref.as4(a)
    axes = [0] * 4
    for i in range(4):
        axes[3 - ax[i]] = 3 - i
    return np.transpose(a4, axes)


CASES: list[Case] = []


def _big(k: int) -> np.ndarray:
    """the k-th grid-stride sized operand (made when a case asks for it, not at import)"""
    return (np.random.default_rng(1000 + k).standard_normal(GRID_STRIDE_N) * 3).astype(np.float32)


def add(*a, **k):
    CASES.append(Case(*a, **k))


# ------------------------------------------------------------------------------------------------ binary
def _bin_case(cid, op, a, b, route, build=None, want=None):
    fn = "ggml_" + op
    add(cid, build or (lambda g, L: getattr(L, fn)(g.ctx, g.input(a), g.input(b))), want or (lambda: ref.binary(op, a, b)), {route: 1})


def _binary_cases():
    for op in ("add", "sub", "mul", "div"):
        for n in (1024, 1025, 1026, 1027, 3):   # n = 4k .. 4k+3 and the tail alone
            r = rng_for(f"bin-same-{op}-{n}")
            _bin_case(f"bin-same-{op}-n{n}", op, r.standard_normal(n).astype(np.float32), (r.standard_normal(n) + 3).astype(np.float32), "ew_bin_same")
        r = rng_for("bin-" + op)
        nrm = lambda *s: r.standard_normal(s).astype(np.float32)
        off = lambda *s: (r.standard_normal(s) + 3).astype(np.float32)
        _bin_case(f"bin-rowvec-{op}", op, nrm(3, 77, 64), off(64), "ew_bin_rowvec")
        _bin_case(f"bin-rowvec-miss-ne0-66-{op}", op, nrm(3, 77, 66), off(66), "ew_bin_generic")
        _bin_case(f"bin-tokvec-{op}", op, nrm(3, 5, 64), off(3, 1, 64), "ew_bin_tokvec")
        _bin_case(f"bin-tokvec-miss-ne0-62-{op}", op, nrm(3, 5, 62), off(3, 1, 62), "ew_bin_generic")
        _bin_case(f"bin-tokvec-miss-ne3-2-{op}", op, nrm(2, 3, 5, 64), off(1, 3, 1, 64), "ew_bin_generic")
        _bin_case(f"bin-chan-c-{op}", op, nrm(2, 8, 16, 16), off(1, 8, 1, 1), "ew_bin_chan")
        _bin_case(f"bin-chan-cn-{op}", op, nrm(2, 8, 16, 16), off(2, 8, 1, 1), "ew_bin_chan")
        _bin_case(f"bin-chan-miss-inner-225-{op}", op, nrm(2, 8, 15, 15), off(2, 8, 1, 1), "ew_bin_generic")
        _bin_case(f"bin-generic-bcast-dims-0-2-{op}", op, nrm(2, 3, 5, 8), off(2, 1, 5, 1), "ew_bin_generic")

        # a is a permuted view
        xa, xb = nrm(2, 3, 5, 8), off(2, 3, 8, 5)
        _bin_case(f"bin-generic-a-permuted-{op}", op, None, None, "ew_bin_generic",
                  build=lambda g, L, fn="ggml_" + op, xa=xa, xb=xb: getattr(L, fn)(g.ctx, L.ggml_permute(g.ctx, g.input(xa), 1, 0, 2, 3), g.input(xb)),
                  want=lambda op=op, xa=xa, xb=xb: ref.binary(op, np_permute(xa, (1, 0, 2, 3)), xb))
        # b is a strided view: 8 of the 12 columns of every row
        ya, yb = nrm(7, 8), off(7, 12)
        _bin_case(f"bin-generic-b-strided-{op}", op, None, None, "ew_bin_generic",
                  build=lambda g, L, fn="ggml_" + op, ya=ya, yb=yb: getattr(L, fn)(g.ctx, g.input(ya), L.ggml_view_2d(g.ctx, g.input(yb), 8, 7, 12 * 4, 0)),
                  want=lambda op=op, ya=ya, yb=yb: ref.binary(op, ya, yb[:, :8]))

    # in place on views (ADD and MUL have in-place builders): a same-shape contiguous op whose pointers are 4 bytes off a 16-byte boundary ...
    for op in ("add", "mul"):
        r = rng_for("bin-inplace-" + op)
        x, b = r.standard_normal(41).astype(np.float32), (r.standard_normal(40) + 3).astype(np.float32)

        def build_off4(g, L, fn=f"ggml_{op}_inplace", x=x, b=b):
            xin = g.input(x)
            return getattr(L, fn)(g.ctx, L.ggml_view_1d(g.ctx, xin, 40, 4), g.input(b)), xin

        add(f"bin-generic-inplace-offset-4-{op}", build_off4, lambda op=op, x=x, b=b: np.concatenate([x[:1], ref.binary(op, x[1:], b)]), {"ew_bin_generic": 1})
        # ... and a destination with row padding (dnb[1] > ne0 * 4): the bytes between the rows must stay as they were
        x2, b2 = r.standard_normal((6, 12)).astype(np.float32), (r.standard_normal((6, 8)) + 3).astype(np.float32)

        def build_padded(g, L, fn=f"ggml_{op}_inplace", x2=x2, b2=b2):
            xin = g.input(x2)
            return getattr(L, fn)(g.ctx, L.ggml_view_2d(g.ctx, xin, 8, 6, 12 * 4, 0), g.input(b2)), xin

        add(f"bin-generic-dst-row-padding-{op}", build_padded, lambda op=op, x2=x2, b2=b2: np.concatenate([ref.binary(op, x2[:, :8], b2), x2[:, 8:]], axis=1),
            {"ew_bin_generic": 1})

    # the grid-stride loop: threads take a second trip and the tail still lands
    _bin_case("bin-same-add-gridstride", "add", None, None, "ew_bin_same", build=lambda g, L: L.ggml_add(g.ctx, g.input(_big(0)), g.input(_big(1))),
              want=lambda: ref.binary("add", _big(0), _big(1)))

    # DIV at the edges of the format: divisors near the subnormal limit, subnormal, and +-0 (inf and NaN patterns as IEEE 754 has them)
    num = np.array([1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, 1e-38, 3e38, 1e-45, 1.17549435e-38, 7.0, np.nan], dtype=np.float32)
    den = np.array([0.0, -0.0, 1.17549435e-38, -1.17549435e-38, 1.1754942e-38, 1e-45, -1e-45, 2e-38, 3e38, np.inf, 3.0, 1e-40], dtype=np.float32)
    da, db = [m.astype(np.float32).copy() for m in np.meshgrid(num, den, indexing="ij")]
    _bin_case("bin-same-div-edges", "div", da, db, "ew_bin_same")
    _bin_case("bin-generic-div-edges", "div", da[:, :11], db[:, :11], "ew_bin_generic",
              build=lambda g, L: L.ggml_div(g.ctx, g.input(da[:, :11].copy()), L.ggml_view_2d(g.ctx, g.input(db), 11, 12, 12 * 4, 0)))


# ------------------------------------------------------------------------------------------------ unary, scale
SATURATING = np.array([s * v for v in (0.0, 1e-8, 10.0, 20.0, 50.0, 88.0, 100.0, 1e4) for s in (1.0, -1.0)], dtype=np.float32)
GELU_ORACLE_TOL = 2e-3   # ggml-cpu's GELU / GELU-quick go through f16 tables (input and output rounded to f16): tests/test_gpu_ops.py::test_unary


def _saturated_ends(op):
    def check(out, want):
        x = SATURATING
        assert np.isfinite(out).all(), out
        if op == "silu":
            assert (out[x >= 50] == x[x >= 50]).all() and (out[x <= -100] == 0).all()
        elif op == "sigmoid":
            assert ((out >= 0) & (out <= 1)).all()
        elif op == "tanh":
            assert (out[x >= 20] == 1).all() and (out[x <= -20] == -1).all()
    return check


def _unary_cases():
    for op, chk, tol, otol in (("silu", "abs", 2e-6, None), ("sigmoid", "abs", 2e-6, None), ("tanh", "abs", 2e-6, None), ("gelu", "abs", 2e-6, GELU_ORACLE_TOL),
                               ("gelu_quick", "abs", 2e-6, GELU_ORACLE_TOL), ("relu", "bits", 0.0, None), ("neg", "bits", 0.0, None), ("exp", "rel", 4e-6, None)):
        fn = UNARY_ENUM.get(op, "ggml_" + op)
        for n in (1024, 1025, 1026, 1027):
            x = (rng_for(f"un-{op}-{n}").standard_normal(n) * 3).astype(np.float32)
            add(f"un-{op}-n{n}", lambda g, L, fn=fn, x=x: getattr(L, fn)(g.ctx, g.input(x)), lambda op=op, x=x: ref.unary(op, x), {}, chk, tol, otol)
        # arguments at which the exp / reciprocal forms saturate.  EXP overflows float32 above 88.7: it gets the part of the list below that.
        xs = SATURATING[np.abs(SATURATING) <= 88] if op == "exp" else SATURATING
        sat_chk = "bits" if chk == "bits" else ("rel" if op == "exp" else "abs_elem")
        add(f"un-{op}-saturating", lambda g, L, fn=fn, xs=xs: getattr(L, fn)(g.ctx, g.input(xs)), lambda op=op, xs=xs: ref.unary(op, xs), {}, sat_chk, tol, otol,
            extra=None if op == "exp" else _saturated_ends(op))
    add("un-silu-gridstride", lambda g, L: L.ggml_silu(g.ctx, g.input(_big(2))), lambda: ref.unary("silu", _big(2)), {}, "abs", 2e-6)

    # SCALE: x * s + b is one fused multiply-add (hipcc contracts it; ggml-cpu's ggml_vec_mad1_f32 is an FMA on the FMA-capable hosts the oracle is built for):
    # exact against the product and sum rounded ONCE
    for n, s, b in ((1027, 0.125, 0.0), (1027, 1.7, -0.3), (1024, -0.3333333, 1e-3), (5, 3.0, 1e8)):
        xs_ = rng_for(f"scale-{n}-{s}-{b}").standard_normal(n).astype(np.float32)

        def build(g, L, xs_=xs_, s=s, b=b):
            node = L.ggml_scale(g.ctx, g.input(xs_), s)
            tensor_struct(node).op_params[1] = int(np.array([b], dtype=np.float32).view(np.int32)[0])   # the bias (upstream's ggml_scale_bias)
            return node

        add(f"scale-n{n}-s{s}-b{b}", build, lambda xs_=xs_, s=s, b=b: ref.scale_bias(xs_, s, b), {})


# ------------------------------------------------------------------------------------------------ copy / cast
COPY_PAIRS = ((F32, F32), (F32, F16), (F16, F32), (F16, F16), (F32, BF16), (BF16, F32))
UNSUPPORTED_COPY_PAIRS = ((F16, BF16), (BF16, F16), (BF16, BF16))
# f32 values whose conversion has an edge: ties (to even) in f16 and bf16, overflow to inf, subnormal results, NaN (one with a payload that only lives
# in the low mantissa bits: the bf16 quiet rule), signed zeros, infinities
SPECIALS = np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 65520.0, -65536.0, 1e-8, 5.9604645e-8, 2.0 ** -25, 3 * 2.0 ** -25, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 3.4e38,
                     -3.4e38, 1e-40, 0.0, -0.0, np.inf, -np.inf, np.nan, 0.0], dtype=np.float32)
SPECIALS[-1] = np.array([0x7F800001], dtype=np.uint32).view(np.float32)[0]


def _copy_input(cid, shape, st):
    x = rng_for(cid).standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    flat[:min(flat.size, SPECIALS.size)] = SPECIALS[:flat.size]
    return ref.round_to(x, TYPE_NAME[st])   # what the source tensor holds


def _cast(g, L, view, st, dt):
    return L.ggml_cont(g.ctx, view) if st == dt else L.ggml_cast(g.ctx, view, dt)


def _copy_cases():
    for st, dt in COPY_PAIRS:
        tag = f"{TYPE_NAME[st]}-{TYPE_NAME[dt]}"
        chk = "bits_nan" if dt == BF16 else "bits"

        def case(name, shape, view, want, route, tag=tag, st=st, dt=dt, chk=chk, flat_extra=0):
            cid = f"copy-{name}-{tag}"
            x = _copy_input(cid, shape, st)
            add(cid, lambda g, L: _cast(g, L, view(g, L, g.input(x, st)), st, dt), lambda: ref.round_to(want(x), TYPE_NAME[dt]), {route: 1}, chk)

        es = 4 if st == F32 else 2
        case("contig-n4k+1", (1029,), lambda g, L, t: t, lambda x: x, "ew_copy_contig")
        # NCHW -> tokens: dims 1, 2 of the permuted view are one run (merged into one transpose per image), 2 x 2 LDS tiles with ragged edges
        case("transpose-merged", (2, 70, 5, 15), lambda g, L, t: L.ggml_permute(g.ctx, t, 1, 2, 0, 3), lambda x: np_permute(x, (1, 2, 0, 3)), "ew_copy_transpose")
        # dims 1, 2 not merged, R = 65 and C = 63 (no multiples of the 64 x 64 tile), batch in ne2
        case("transpose-65x63", (2, 63, 65), lambda g, L, t: L.ggml_permute(g.ctx, t, 1, 0, 2, 3), lambda x: np_permute(x, (1, 0, 2, 3)), "ew_copy_transpose")
        # ... and a batch in ne3 as well
        case("transpose-batch-ne3", (3, 2, 9, 7), lambda g, L, t: L.ggml_permute(g.ctx, t, 1, 0, 2, 3), lambda x: np_permute(x, (1, 0, 2, 3)), "ew_copy_transpose")
        # head permute, rows of ne0 = 8
        case("rows-head-permute", (2, 5, 3, 8), lambda g, L, t: L.ggml_permute(g.ctx, t, 0, 2, 1, 3), lambda x: np_permute(x, (0, 2, 1, 3)), "ew_copy_rows")
        case("rows-miss-ne0-6", (2, 5, 3, 6), lambda g, L, t: L.ggml_permute(g.ctx, t, 0, 2, 1, 3), lambda x: np_permute(x, (0, 2, 1, 3)), "ew_copy_generic")
        # the same head permute on a view that starts 4 bytes into its buffer: the rows are no longer aligned for the 4-element accesses
        skip = 4 // es
        case("rows-miss-offset-4", (240 + skip,),
             lambda g, L, t, es=es: L.ggml_permute(g.ctx, L.ggml_view_4d(g.ctx, t, 8, 3, 5, 2, 8 * es, 24 * es, 120 * es, 4), 0, 2, 1, 3),
             lambda x, skip=skip: np_permute(x[skip:].reshape(2, 5, 3, 8), (0, 2, 1, 3)), "ew_copy_generic")
        case("generic-double-permute", (2, 3, 4, 5), lambda g, L, t: L.ggml_permute(g.ctx, t, 3, 2, 1, 0), lambda x: np_permute(x, (3, 2, 1, 0)), "ew_copy_generic")

        # ggml_cpy of a [6, 10] (transposed view) into a [4, 15] destination: logical element order is kept across the two shapes
        cid = f"copy-generic-cpy-6x10-into-4x15-{tag}"
        x = _copy_input(cid, (6, 10), st)

        def build_cpy(g, L, x=x, st=st, dt=dt):
            dst = g.input(np.zeros((15, 4), dtype=np.float32), dt)
            return L.ggml_cpy(g.ctx, L.ggml_transpose(g.ctx, g.input(x, st)), dst)

        add(cid, build_cpy, lambda x=x, dt=dt: ref.copy(x.T, (15, 4), TYPE_NAME[dt]), {"ew_copy_generic": 1}, chk)

    # grid.z of the transpose route carries ne2 * ne3 when dims 1, 2 do not merge: beyond 65535 the copy takes the generic route
    xz = rng_for("copy-gridz").standard_normal((70000, 2, 2)).astype(np.float32)
    add("copy-transpose-miss-gridz-70000", lambda g, L: L.ggml_cont(g.ctx, L.ggml_permute(g.ctx, g.input(xz), 1, 0, 2, 3)), lambda: np_permute(xz, (1, 0, 2, 3)),
        {"ew_copy_generic": 1})


# ------------------------------------------------------------------------------------------------ concat / repeat / upscale / pad
def _layout_cases():
    r = rng_for("layout")
    nrm = lambda *s: r.standard_normal(s).astype(np.float32)

    def cat(cid, a, b, dim, route, va=None, wa=None):
        add(cid, lambda g, L: L.ggml_concat(g.ctx, (va or (lambda g, L, t: t))(g, L, g.input(a)), g.input(b), dim), lambda: ref.concat((wa or (lambda x: x))(a), b, dim),
            {route: 1})

    cat("concat-dim2", nrm(2, 3, 4, 6), nrm(2, 5, 4, 6), 2, "ew_concat_dim2")
    cat("concat-dim2-miss-sa-75", nrm(2, 3, 5, 5), nrm(2, 1, 5, 5), 2, "ew_concat_generic")
    # a holds the first 3 of 6 channels of each image of a larger tensor: its (ne0, ne1) planes are contiguous, the images are not
    planes = lambda w, h: (lambda g, L, t: L.ggml_view_4d(g.ctx, t, w, h, 3, 2, w * 4, w * h * 4, 6 * w * h * 4, 0))
    cat("concat-planes", nrm(2, 6, 4, 6), nrm(2, 5, 4, 6), 2, "ew_concat_planes", planes(6, 4), lambda x: x[:, :3])
    cat("concat-planes-miss-plane-25", nrm(2, 6, 5, 5), nrm(2, 5, 5, 5), 2, "ew_concat_generic", planes(5, 5), lambda x: x[:, :3])
    cat("concat-generic-dim0", nrm(2, 3, 4, 5), nrm(2, 3, 4, 3), 0, "ew_concat_generic")
    cat("concat-generic-dim1", nrm(2, 3, 4, 5), nrm(2, 3, 2, 5), 1, "ew_concat_generic")
    cat("concat-generic-dim3", nrm(2, 3, 4, 5), nrm(1, 3, 4, 5), 3, "ew_concat_generic")

    src = nrm(2, 3, 4, 5)
    for name, mult in (("dim0", (1, 1, 1, 2)), ("dim1", (1, 1, 3, 1)), ("dim2", (1, 2, 1, 1)), ("dim3", (2, 1, 1, 1)), ("dims-0-2", (1, 2, 1, 3))):
        shape = tuple(s * m for s, m in zip(src.shape, mult))
        add(f"repeat-{name}", lambda g, L, shape=shape: L.ggml_repeat(g.ctx, g.input(src), g.input(np.zeros(shape, dtype=np.float32))), lambda shape=shape: ref.repeat(src, shape))

    for f in (2, 3):   # nearest upscale of a permuted source
        add(f"upscale-x{f}-permuted", lambda g, L, f=f: L.ggml_upscale(g.ctx, L.ggml_permute(g.ctx, g.input(src), 1, 0, 2, 3), f, 0),
            lambda f=f: ref.upscale_nearest(np_permute(src, (1, 0, 2, 3)), (2, 3, 5 * f, 4 * f)))

    big = nrm(2, 3, 4, 7)   # the source is the first 5 columns of every row of a larger tensor
    for name, pads in (("lp0", (1, 0, 0, 0, 0, 0, 0, 0)), ("lp1", (0, 0, 2, 0, 0, 0, 0, 0)), ("lp2", (0, 0, 0, 0, 1, 0, 0, 0)), ("lp3", (0, 0, 0, 0, 0, 0, 1, 0)),
                       ("left-and-right", (1, 2, 2, 1, 1, 1, 1, 2)), ("right-only", (0, 2, 0, 1, 0, 0, 0, 0))):
        add(f"pad-{name}-strided-src",
            lambda g, L, pads=pads: L.ggml_pad_ext(g.ctx, L.ggml_view_4d(g.ctx, g.input(big), 5, 4, 3, 2, 7 * 4, 28 * 4, 84 * 4, 0), *pads),
            lambda pads=pads: ref.pad_ext(big[..., :5], pads))


# ------------------------------------------------------------------------------------------------ get_rows, timestep embedding, im2col
def _gather_cases():
    n_rows = 7
    for tt in (F32, F16, BF16, Q8_0, Q4_0):
        for nc in (32, 33, 288):
            if nc % 32 and tt in (Q8_0, Q4_0):
                continue
            cid = f"get-rows-{TYPE_NAME[tt]}-nc{nc}"
            tab = rng_for(cid).standard_normal((n_rows, nc)).astype(np.float32)
            dec = ref.round_to(tab, "bf16") if tt == BF16 else dequant(tab, tt) if tt != F32 else tab   # what the stored table decodes to (the quantised ones by the host library)
            for name, ids in (("", np.array([0, n_rows - 1, 3, n_rows - 1, 0], dtype=np.int32)), ("-one-row", np.array([n_rows - 1], dtype=np.int32))):
                add(cid + name, lambda g, L, tab=tab, tt=tt, ids=ids: L.ggml_get_rows(g.ctx, g.weight(tab, tt), g.input(ids, I32)),
                    lambda dec=dec, ids=ids: ref.get_rows(dec, ids))
    # ids as a transposed (strided) view, one plane of the table per ids row
    tab3 = rng_for("get-rows-strided").standard_normal((2, n_rows, 32)).astype(np.float32)
    ids2 = np.array([[0, 6], [6, 0], [3, 1], [2, 6], [0, 5]], dtype=np.int32)   # stored [5][2]; the view is ne = [5, 2]
    add("get-rows-f32-strided-ids", lambda g, L: L.ggml_get_rows(g.ctx, g.weight(tab3, F32), L.ggml_transpose(g.ctx, g.input(ids2, I32))),
        lambda: ref.get_rows(tab3, ids2.T))

    t = np.array([0.0, 999.0, 500.25, 13.5], dtype=np.float32)
    for dim in (2, 3, 320):   # dim = 3: one cos, one sin and the zero pad
        add(f"timestep-embedding-dim{dim}", lambda g, L, dim=dim: L.ggml_timestep_embedding(g.ctx, g.input(t), dim, 10000),
            lambda dim=dim: ref.timestep_embedding(t, dim, 10000), {}, "abs_plain", 5e-4)   # the bar of test_scale_and_timestep_embedding: f32 cos / sin of arguments up to 999


def _im2col_cases():
    x = rng_for("im2col").standard_normal((2, 3, 5, 7)).astype(np.float32)   # ne = [7, 5, 3, 2]
    x[0, 0, 0, :3] = [65519.0, 1 + 2.0 ** -11, 1e-8]                        # f16 destination: overflow-adjacent, a tie, a subnormal result
    for dt in (F32, F16):
        for name, (kw, kh, s0, s1, p0, p1, d0, d1) in (("3x3-s2-p0", (3, 3, 2, 2, 0, 0, 1, 1)), ("3x3-s2-p1", (3, 3, 2, 2, 1, 1, 1, 1)), ("3x3-s2-p2", (3, 3, 2, 2, 2, 2, 1, 1)),
                                                        ("3x3-s1-p2-d2", (3, 3, 1, 1, 2, 2, 2, 2)), ("1x3-s1-p1x0", (3, 1, 1, 1, 1, 0, 1, 1)),
                                                        ("3x2-s2x1-p1x0-d1x2", (3, 2, 2, 1, 1, 0, 1, 2))):
            args = (kw, kh, s0, s1, p0, p1, d0, d1)
            kern = np.zeros((4, 3, kh, kw), dtype=np.float32)   # only its shape is read

            def build(g, L, kern=kern, a=args, dt=dt, permuted=False):
                xin = L.ggml_permute(g.ctx, g.input(np.ascontiguousarray(np.swapaxes(x, 2, 3))), 1, 0, 2, 3) if permuted else g.input(x)
                return L.ggml_im2col(g.ctx, g.input(kern, F16), xin, a[2], a[3], a[4], a[5], a[6], a[7], True, dt)

            add(f"im2col-{name}-{TYPE_NAME[dt]}", build, lambda a=args, dt=dt: ref.im2col(x, *a, True, TYPE_NAME[dt]))
            if name == "3x3-s2-p1":
                add(f"im2col-{name}-permuted-input-{TYPE_NAME[dt]}", lambda g, L, build=build: build(g, L, permuted=True), lambda a=args, dt=dt: ref.im2col(x, *a, True, TYPE_NAME[dt]))
        # the 1-D form: input [9, 3, 2] (IW, IC, N), kernel [3, 3, 4] (KW, IC, OC) -> [IC * KW, OW, N]
        x1 = rng_for("im2col-1d").standard_normal((2, 3, 9)).astype(np.float32)
        for name, (s0, p0, d0) in (("s1-p1", (1, 1, 1)), ("s2-p2-d2", (2, 2, 2))):
            add(f"im2col-1d-{name}-{TYPE_NAME[dt]}",
                lambda g, L, s0=s0, p0=p0, d0=d0, dt=dt: L.ggml_im2col(g.ctx, g.input(np.zeros((4, 3, 3), dtype=np.float32), F16), g.input(x1), s0, 0, p0, 0, d0, 0, False, dt),
                lambda s0=s0, p0=p0, d0=d0, dt=dt: ref.im2col(x1, 3, 1, s0, 1, p0, 0, d0, 1, False, TYPE_NAME[dt]))


_binary_cases()
_unary_cases()
_copy_cases()
_layout_cases()
_gather_cases()
_im2col_cases()
assert len({c.id for c in CASES}) == len(CASES), "case ids are unique"

ROUTE_FIELDS = ("ew_bin_same ew_bin_rowvec ew_bin_tokvec ew_bin_chan ew_bin_generic ew_copy_contig ew_copy_transpose ew_copy_rows ew_copy_generic "
                "ew_concat_dim2 ew_concat_planes ew_concat_generic").split()


def run_case(case: Case, device: str, L):
    """build the case's graph on `device`, run it, return the result in the shape of case.want()"""
    from ggml_graph import Graph
    with Graph(device) as g:
        built = case.build(g, L)
        node, target = built if isinstance(built, tuple) else (built, None)
        out = g.run(node)
        if target is not None:
            out = g.fetch(target)
    return out


def check_case(case: Case, out: np.ndarray, on_oracle: bool) -> None:
    want = np.asarray(case.want())
    out = np.asarray(out).reshape(want.shape) if out.size == want.size else out
    assert out.shape == want.shape, (out.shape, want.shape)
    tol = case.oracle_tol if (on_oracle and case.oracle_tol is not None) else case.tol
    if case.check in ("bits", "bits_nan"):
        ref.assert_same_bits(out, want.astype(np.float32), nan_bits=case.check == "bits_nan")
    else:
        w64, o64 = want.astype(np.float64), out.astype(np.float64)
        err = np.abs(o64 - w64)
        assert np.isfinite(out).all()
        if case.check == "abs":
            bar = tol * max(1.0, float(np.abs(w64).max()))
        elif case.check == "abs_elem":   # saturating arguments span 1e-8 .. 1e4: the bar scales with each element instead of the largest
            bar = tol * np.maximum(1.0, np.abs(w64))
        elif case.check == "abs_plain":
            bar = tol
        else:
            bar = tol * np.abs(w64)
        worst = int(np.argmax(err - bar))
        print(f"{case.id}: max |out - ref| {err.max():.3e} (max rel {np.max(err / np.maximum(np.abs(w64), 1e-300)):.3e}), bar at the worst element {np.broadcast_to(bar, err.shape).reshape(-1)[worst]:.3e}")
        assert (err <= bar).all(), (case.id, float(err.reshape(-1)[worst]), float(np.broadcast_to(bar, err.shape).reshape(-1)[worst]), float(w64.reshape(-1)[worst]))
    if case.extra is not None:
        case.extra(out.reshape(-1), want.reshape(-1))
