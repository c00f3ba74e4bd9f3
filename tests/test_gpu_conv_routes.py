"""Every dispatch route of the implicit-GEMM conv family (kernels/conv3w.hip k_conv3w<TW, BN>, kernels/gemm16.hip k_gemm16<..., CONV> on its eight tile
configurations, unsplit / slab split with k_splitk_reduce / combined in the launch, XCD-aware or weight-major workgroup order) at its geometric edges, on data on
which the kernels must be EXACT.

Each case of conv_cases.py is one convolution with its epilogue, run once on the product backend under the case's options and compared with conv_ref.py (plain
NumPy, float64).  The operands are integers (x in -4 .. 4, w in -2 .. 2, bias in -64 .. 64, residual in -8 .. 8, an integer embedding Linear, a power-of-two Conv2d
scale): every product and partial sum in any order is an integer below 2^24 (conv_ref asserts max|x| * max|w| * K + |epilogue terms| < 2^24 for every case), so f16
operands, f32 MFMA accumulation, K slices, another tile, another K order or another workgroup order cannot change a bit.
Bar: bit for bit on the whole tensor (np.array_equal); a failure names the first differing (n, oc, oh, ow), the count and the bounding box per image.
The route is read from the launch counters c3w_* / g16_conv_* of ggml_backend_mi355x_get_stats (counted where c3_launch / g16_launch / the reduce launchers choose):
the case's counters move exactly as it says, every other one by 0.  tests/test_conv_ref_cpu.py shows without a GPU that the oracle equals the reference on every case
and that every applicable indexing mutant differs from it.  83 cases.
Measured on the MI355X: the MFMA's multi-term add is exact on such integers — all 83 cases were bit-identical to the reference on their first run, with the counters as
stated (no kernel or planner bug found by this pass); the file takes 8 s (84 tests, the slowest 0.6 s: its NumPy reference).
The counter assertions are skipped under SDCPP_BACKEND_OPTS and with SDCPP_GPU_TESTS_ON_ORACLE=1 (there the file repeats the CPU file)."""
import os

import pytest

from conv_cases import CASES, CONV_ROUTE_FIELDS, OPTION_DEFAULTS, ROUTE_FIELDS, check_case, run_case

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"

_routes_seen: set[str] = set()
_cases_run: set[str] = set()


def _counting():
    return ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_route(sd, gpu, case):
    assert set(case.opts) <= set(OPTION_DEFAULTS), case.opts
    try:
        if ON_GPU:
            for k, v in case.opts.items():
                sd.backend_set_option(k, v)
        before = sd.backend_stats() if _counting() else None
        out = run_case(case, gpu, sd.lib())
        after = sd.backend_stats() if _counting() else None
    finally:
        if ON_GPU:
            for k in case.opts:
                sd.backend_set_option(k, OPTION_DEFAULTS[k])
    _cases_run.add(case.id)
    check_case(case, out)
    if before is not None:
        moved = {f: after[f] - before[f] for f in ROUTE_FIELDS if after[f] != before[f]}
        assert moved == case.routes, f"{case.id}: counters moved {moved}, expected {case.routes}"
        _routes_seen.update(moved)


def test_zz_every_route_was_taken():
    """a conv route that no case reaches fails here instead of going unnoticed"""
    if not _counting():
        return
    if _cases_run != {c.id for c in CASES}:
        pytest.skip("only part of the file was selected")
    assert set(CONV_ROUTE_FIELDS) <= _routes_seen, sorted(set(CONV_ROUTE_FIELDS) - _routes_seen)
