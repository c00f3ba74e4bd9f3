"""Every dispatch route of the memory-bound glue kernels (kernels/elementwise.hip, k_im2col) at its edges.  Each case of elementwise_cases.py is a one- or
two-node graph run on the product backend, compared with a plain NumPy reference (elementwise_ref.py: float64 where there is arithmetic, indexing where there is
not), with the route it took read from the launch counters ew_* of ggml_backend_mi355x_get_stats: the case's route moves by exactly 1, every other route of
the binary / copy / concat launchers by 0.  Routes come in pairs, the smallest shape that lands on one and its nearest miss.

Bars.  + - * /, copies / casts, concat, repeat, upscale, pad, get_rows, im2col, ReLU, NEG, SCALE (one fused multiply-add): bit for bit.  SiLU, sigmoid,
tanh, GELU (tanh form), GELU-quick (sigmoid form): |out - ref| <= 2e-6 * max(1, max|ref|) against float64, on the list of saturating arguments per element
(2e-6 * max(1, |ref|)).  EXP: relative 4e-6 (the argument scaling of a fast exp at |x| = 88 is 88 * 2^-24).  Timestep embedding: 5e-4 absolute.
Measured on the MI355X against float64 (inputs 3 * N(0, 1), n = 1024 .. 1027): SiLU 7.0e-7, sigmoid 9.3e-8, tanh 6.6e-8, GELU 3.3e-7, GELU-quick 6.8e-7
absolute (all inside 2e-6: the 2e-3 of test_unary is the oracle's f16 table), SiLU over the grid-stride size 1.2e-6; EXP 7.0e-8 relative, 6.8e-8 at +-88
(with __expf, which the EXP node used before: 4.6e-7, 1.8e-6 at +88 and a subnormal exp(-88) flushed to 0, which is why it is expf now); timestep
embedding 4.2e-5 at dim 320.
The counter assertions are skipped under SDCPP_BACKEND_OPTS and with SDCPP_GPU_TESTS_ON_ORACLE=1 (there the file repeats tests/test_elementwise_ref_cpu.py
and the product-only predicates skip)."""
import os

import numpy as np
import pytest

from elementwise_cases import CASES, ROUTE_FIELDS, UNSUPPORTED_COPY_PAIRS, TYPE_NAME, check_case, run_case
from ggml_graph import F16, F32, Graph, tensor_struct

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"

_routes_seen: set[str] = set()
_cases_run: set[str] = set()


def _counting():
    return ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_route(sd, gpu, case):
    before = sd.backend_stats() if _counting() else None
    out = run_case(case, gpu, sd.lib())
    after = sd.backend_stats() if _counting() else None
    check_case(case, out, on_oracle=not ON_GPU)
    if before is not None:
        moved = {f: after[f] - before[f] for f in ROUTE_FIELDS if after[f] != before[f]}
        assert moved == case.routes, f"{case.id}: routes taken {moved}, expected {case.routes}"
        _routes_seen.update(moved)
    _cases_run.add(case.id)


@pytest.mark.skipif(not ON_GPU, reason="planner_supports_op is the product backend's predicate")
@pytest.mark.parametrize("st,dt", UNSUPPORTED_COPY_PAIRS, ids=lambda t: TYPE_NAME[t])
def test_unsupported_copy_pairs_are_refused(sd, gpu, st, dt):
    """launch_copy has no kernel for these pairs (it aborts if it is ever reached with one): supports_op has to keep them away from it"""
    x = np.ones((3, 8), dtype=np.float32)
    with Graph(gpu) as g:
        L = sd.lib()
        assert not g.supports(L.ggml_cast(g.ctx, g.input(x, st), dt))
        if st == dt:
            assert not g.supports(L.ggml_cont(g.ctx, L.ggml_transpose(g.ctx, g.input(x, st))))
            assert not g.supports(L.ggml_dup(g.ctx, g.input(x, st)))
        assert not g.supports(L.ggml_cpy(g.ctx, L.ggml_transpose(g.ctx, g.input(x.T.copy(), st)), g.input(x, dt)))
        assert g.supports(L.ggml_cast(g.ctx, g.input(x, F32), dt)) and g.supports(L.ggml_cast(g.ctx, g.input(x, st), F32))


@pytest.mark.skipif(not ON_GPU, reason="planner_supports_op is the product backend's predicate")
def test_concat_refuses_a_non_f32_second_source(sd, gpu):
    """k_concat* read both sources as float.  (The front-end refuses to build a mixed CONCAT; a foreign graph can hold one: the second source is swapped in
    behind the builder's back.)"""
    x = np.ones((2, 3, 4, 8), dtype=np.float32)
    with Graph(gpu) as g:
        L = sd.lib()
        node = L.ggml_concat(g.ctx, g.input(x), g.input(x), 2)
        assert g.supports(node)
        tensor_struct(node).src[1] = g.input(x, F16)
        assert not g.supports(node)


def test_zz_every_route_was_taken():
    """a route that no case reaches fails here instead of going unnoticed"""
    if not _counting():
        return
    if _cases_run != {c.id for c in CASES}:
        pytest.skip("only part of the file was selected")
    assert set(ROUTE_FIELDS) <= _routes_seen, sorted(set(ROUTE_FIELDS) - _routes_seen)
