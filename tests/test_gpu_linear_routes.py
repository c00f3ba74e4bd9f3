"""Every dispatch route of the Linear (weight MUL_MAT) family — kernels/gemm16.hip launch_gemm16_linear / _multi / _geglu on the nine tile configurations of the
non-conv side of g16_launch (f16 weight image or raw q8_0 / q4_0 rows dequantised in the main loop; unsplit, slab split with k_splitk_reduce / k_splitk_reduce_ln,
combined in the launch, stream-K, row split), kernels/qgemm.hip k_qgemv, k_qgemv_rows<4 / 8 / 16>, launch_qgemv_group, k_qgemm16<RB 1 / 2 / 4> with its slab reduce,
k_fgemv<f16 / f32>, k_wswz_q — at its edges, on data on which the kernels must be EXACT.

Each case of linear_cases.py is one Linear with its epilogue, run once on the product backend under the case's options and compared with linear_ref.py (plain NumPy,
float64).  The operands are integers (x in -4 .. 4, w in -2 .. 2 or exactly-stored q8_0 / q4_0 blocks whose scale varies from block to block, bias in -64 .. 64,
residual in -8 .. 8, gate in -2 .. 2, a power-of-two scale): every product and partial sum in any order is exact in f32 (linear_cases.reference asserts the budget
for every case), so f16 operands, MFMA accumulation, K slices, another tile or another summation order cannot change a bit.
Bar: bit for bit on the whole tensor (np.array_equal); a failure names the first differing (row, column), the count and the bounding box in units of the case's tile.
Behind GELU / GEGLU / SiLU the f16 image is made observable by an identity second Linear (one-non-zero-per-row weights for SiLU) and the bar is
|out - ref64| <= ulp_f16(ref64) + 2^-18 * max(1, |p|) (linear_ref.transcendental_bar; x max(1, |v|) for GEGLU's value factor).
The route is read from the launch counters lin_* of ggml_backend_mi355x_get_stats (counted where the launchers choose) and the planner's own counters: the case's
counters move exactly as it says, every other one by 0.  tests/test_linear_ref_cpu.py shows without a GPU that the oracle equals the reference on every case and that
every applicable mutant differs from it.  The default-policy cases are derived for 256 CUs and skip on another device.  181 cases.
Measured on the MI355X: all 158 exact cases were bit-identical to the reference on their first run with the counters as derived (no kernel or planner bug found by
this pass); the file takes 10 s (182 tests, the slowest 1.1 s: the NumPy reference of the 2048 x 1280 -> 10240 GEGLU).  Largest transcendental-epilogue errors seen,
in both terms of the bar — where the f16 rounding term is the larger one, in f16 ulps of the image value; elsewhere, as a share of the 2^-18 max(1, |p|) term:
GELU 0.49 ulps / 0.15; GEGLU 0.49 ulps / 0.06 (both times max(1, |v|)); SiLU in the row-staging kernels 0.46 ulps / never the larger term.  That is: every image value
is the correctly rounded f16 of a function value good to f32, and of the factor-16 margin assumed for fast-math intrinsics 2.5 are used.  Largest share of the whole
bar: 0.49.  (The grouped k_qgemv launch adds a bias behind the SiLU image: its bar carries one more term than the issue's, 2^-24 |reference|, the half f32 ulp
of that one rounded add; measured there: 0.007 of the bar on the oracle, 0.42 of it on the GPU.)
The counter assertions are skipped under SDCPP_BACKEND_OPTS and with SDCPP_GPU_TESTS_ON_ORACLE=1 (there the file repeats the CPU file)."""
import ctypes as C
import os
from pathlib import Path

import pytest

import linear_cases
from linear_cases import CASES, LIN_ROUTE_FIELDS, OPTION_DEFAULTS, ROUTE_FIELDS, check_case, run_case

pytestmark = pytest.mark.gpu
ON_GPU = os.environ.get("SDCPP_GPU_TESTS_ON_ORACLE") != "1"
ROOT = Path(__file__).resolve().parent.parent

_routes_seen: set[str] = set()
_cases_run: set[str] = set()
_cus = None


def _counting():
    return ON_GPU and not os.environ.get("SDCPP_BACKEND_OPTS")


def _compute_units(sd) -> int:
    global _cus
    if _cus is None:
        cal = sd.calibrate() if ON_GPU else {"compute_units": 256}
        assert cal and cal.get("compute_units", 0) > 0, "the backend's calibration reported no compute units: the default-policy cases cannot be placed"
        _cus = int(cal["compute_units"])
    return _cus


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_route(sd, gpu, case):
    assert set(case.opts) <= set(OPTION_DEFAULTS), case.opts
    if case.policy and _compute_units(sd) != 256:
        pytest.skip(f"a default-policy shape derived for 256 CUs; this device reports {_compute_units(sd)}")
    exact_oracle = None
    if not ON_GPU and case.wtype in ("q8_0", "q4_0"):   # (the oracle's own path quantises the activation rows)
        exact_oracle = C.CDLL(str(ROOT / "oracle" / "_build" / "libggml-cpu-oracle.so"))
        exact_oracle.oracle_set_exact_weights(1)
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
        if exact_oracle is not None:
            exact_oracle.oracle_set_exact_weights(0)
    _cases_run.add(case.id)
    check_case(case, out)
    if before is not None:
        moved = {f: after[f] - before[f] for f in ROUTE_FIELDS if after[f] != before[f]}
        assert moved == case.routes, f"{case.id}: counters moved {moved}, expected {case.routes}"
        _routes_seen.update(moved)


def test_zz_every_route_was_taken():
    """a Linear route that no case reaches fails here instead of going unnoticed"""
    if not _counting():
        return
    if _cases_run != {c.id for c in CASES}:
        pytest.skip("only part of the file was selected (or the default-policy cases skipped)")
    assert set(LIN_ROUTE_FIELDS) <= _routes_seen, sorted(set(LIN_ROUTE_FIELDS) - _routes_seen)
    print("largest transcendental-epilogue errors (f16 ulps where the rounding term governs, share of the second term elsewhere, share of the bar):", linear_cases.worst)
