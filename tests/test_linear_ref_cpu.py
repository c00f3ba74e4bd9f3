"""The Linear route cases (linear_cases.py) without a GPU: is a bit-for-bit pass on the GPU worth anything?

  * the CPU oracle device, given the very graph the GPU file runs, equals linear_ref under the GPU file's bar (bit for bit; linear_ref.transcendental_bar behind GELU /
    GEGLU / SiLU): the reference is right and the graph says what the reference says.  Quantised weights run the oracle with oracle_set_exact_weights(1): ggml-cpu's
    own path quantises the activation rows to q8_0, which is not exact on any data;
  * the constructed quantised weights survive the project's quantiser bit for bit (dequant(w) == w), and linear_ref's NumPy restatement of q8_0 / q4_0 agrees with it;
  * every mutant of linear_ref.py (one indexing or dequantisation bug each) that applies to a case differs from linear_ref on that case's data, by more than the bar;
  * every mutant applies to some case, and every epilogue appears on every kernel family that can carry it, and on a split launch.

Exactness budget (asserted by linear_cases.reference for every case): max|x| * max_row(sum |w|), through the epilogue, < 2^24 in units of the operands' common power of
two; the exact operands (x, w) < 2^11 units in their f16 images.  181 cases, 414 tests, about two minutes on 8 cores (the mutants reuse each case's plain
product: only the three dequantisation mutants contract again)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import linear_ref as R
from ggml_graph import dequant
from linear_cases import CASES, FAMILIES, WTYPES, case_reference, check_case, reference, run_case, tolerance

ROOT = Path(__file__).resolve().parent.parent

# epilogues a kernel family cannot carry at all
IMPOSSIBLE = {
    "gemv": {"gate": "plan_linear sends only plain epilogues to the streaming kernels", "gelu": "as gate", "geglu": "as gate", "ln_next": "no split, no reduce pass"},
    "qgemm16": {"geglu": "plan_linear keeps GEGLU launches on gemm16", "presilu": "the SiLU is deferred into the <= 16-row kernels only", "ln_next": "its reduce pass writes no image"},
    "t128": {"presilu": "as qgemm16"},
    "t256": {"presilu": "as qgemm16", "ln_next": "the default policy never splits a 256-row launch of the non-pipelined tiles"},
    "pipe": {"presilu": "as qgemm16", "ln_next": "k_splitk_reduce_ln serves <= 1280 columns in <= 4 slices: the 256 x 320 tile's slices start at 2560 columns here"},
}
NO_SPLIT = {"presilu": "the streaming kernels do not split"}


def _applies(mutant, case):
    return R.mutant_applies(mutant, rows=case.rows, K=case.K, M=case.M, wtype=case.wtype, epi=case.epi, S=case.S, batches=case.batches, siblings=2 if case.kind == "multi" else 1)


class _exact_oracle:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            self.lib = C.CDLL(str(ROOT / "oracle" / "_build" / "libggml-cpu-oracle.so"))
            self.lib.oracle_set_exact_weights(1)

    def __exit__(self, *a):
        if self.on:
            self.lib.oracle_set_exact_weights(0)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_oracle_equals_reference(sd, oracle, case):
    with _exact_oracle(case.wtype in ("q8_0", "q4_0")):
        out = run_case(case, oracle, sd.lib())
    check_case(case, out)


@pytest.mark.parametrize("case", [c for c in CASES if c.wtype in ("q8_0", "q4_0")], ids=lambda c: c.id)
def test_quantised_weights_round_trip(sd, case):
    d, _ = case_reference(case)
    for w in (d["w"] if isinstance(d["w"], list) else [d["w"]]):
        np.testing.assert_array_equal(dequant(w, WTYPES[case.wtype]), w)                                       # the project's quantiser stores w exactly
        np.testing.assert_array_equal(R.dequantise(*R.quantise(w, case.wtype), case.wtype), w.astype(np.float64))   # ... and so does the NumPy restatement
        dq = R.quantise(w, case.wtype)[0]
        assert case.epi == "presilu" or (len(np.unique(dq)) == 4 and (case.K == 32 or (dq[:, 1:] != dq[:, :-1]).all())), "the block scales vary from block to block"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_mutants_differ_from_reference(case):
    d, (want, p) = case_reference(case)
    terms = tolerance(case, want, p, d)
    tol = None if terms is None else terms[0] + terms[1]
    for m in R.MUTANTS:
        if _applies(m, case):
            got, _ = reference(case, d, mutant=m)
            differs = not np.array_equal(got, want) if tol is None else bool((np.abs(got - want) > 2 * tol).any())
            assert differs, f"{case.id}: the data of this case does not tell {m} from the truth"


def test_every_mutant_applies_to_some_case():
    for m in R.MUTANTS:
        assert any(_applies(m, c) for c in CASES), m


def test_every_epilogue_on_every_family_and_on_a_split_launch():
    for e in R.EPILOGUES:
        for fam in FAMILIES:
            if e in IMPOSSIBLE.get(fam, {}):
                assert not any(c.epi == e and c.family == fam for c in CASES), (e, fam)
                continue
            assert any(c.epi == e and c.family == fam for c in CASES), (e, fam)
        if e not in NO_SPLIT:
            assert any(c.epi == e and (c.S > 1 or "lin_streamk" in c.routes) for c in CASES), (e, "split")   # K slices, or stream-K's cut tiles
        if e == "gate":   # fused, on both last-arriver combines, over several images (gate_wrong_batch applies)
            for how in ("split_k_inlaunch",):
                assert any(c.epi == e and c.routes.get("fused_gate") and how in c.routes and c.batches > 1 and c.S > 1 for c in CASES)
                assert any(c.epi == e and c.routes.get("fused_gate") and "lin_streamk" in c.routes and c.batches > 1 for c in CASES)


def test_reference_and_mutants_by_hand():
    """2 x 2 values that can be read off"""
    x = np.array([[1.0, 2.0] + [0.0] * 30, [3.0, 4.0] + [0.0] * 30])
    w = np.array([[1.0, 0.0] + [0.0] * 30, [0.0, 1.0] + [0.0] * 30, [1.0, 1.0] + [0.0] * 30])
    b, r = np.array([10.0, 20.0, 30.0]), np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    np.testing.assert_array_equal(R.linear_ref(x, w)[0], [[1, 2, 3], [3, 4, 7]])
    np.testing.assert_array_equal(R.linear_ref(x, w, epi="bias+res", bias=b, residual=r)[0], [[12, 24, 36], [17, 29, 43]])
    np.testing.assert_array_equal(R.linear_ref(x, w, epi="bias", bias=b, mutant="bias_by_row")[0], [[11, 12, 13], [23, 24, 27]])
    np.testing.assert_array_equal(R.linear_ref(x, w, epi="bias+res", bias=b, residual=r, mutant="residual_wrong_ld")[0], [[12, 24, 36], [16, 28, 42]])
    np.testing.assert_array_equal(R.linear_ref(x, w, epi="gate", bias=b, residual=r, gate=np.array([[2.0, 2, 2], [3.0, 3, 3]]), batches=2)[0], [[23, 46, 69], [43, 77, 117]])
    np.testing.assert_array_equal(R.linear_ref(x, w, epi="scale", bias=b)[0], [[11, 22, 33], [13, 24, 37]])
    np.testing.assert_array_equal(R.linear_ref(x, w, mutant="last_column_tile_shifted", bn=2)[0], [[1, 2, 2], [3, 4, 4]])
    np.testing.assert_array_equal(R.linear_ref(x, w, mutant="last_row_tile_skipped", bm=1)[0], [[1, 2, 3], [0, 0, 0]])
    np.testing.assert_array_equal(R.linear_ref(x, w, mutant="drop_last_k_block_of_a_slice")[0], np.zeros((2, 3)))
    np.testing.assert_array_equal(R.linear_ref(x, w, mutant="read_past_k_padding")[0], [[4, 6, 10], [3, 4, 7]])   # row 0 also meets row 1's first 32 values
    g = R.linear_ref(x, w[:2], epi="geglu", bias=b[:2])[0]
    np.testing.assert_allclose(g, [[11 * R.gelu64(22.0)], [13 * R.gelu64(24.0)]])
    # q4_0: a block of -8 d, 7 d and zeros stores d; the three dequantisation bugs
    blk = np.zeros((1, 64), dtype=np.float32)
    blk[0, 0], blk[0, 17], blk[0, 32], blk[0, 33] = -4.0, 3.5, -16.0, 2.0      # d = 1 / 2 and d = 2
    d, q = R.quantise(blk, "q4_0")
    np.testing.assert_array_equal(d, [[0.5, 2.0]])
    np.testing.assert_array_equal(R.dequantise(d, q, "q4_0"), blk)
    assert R.dequantise(d, q, "q4_0", "q4_nibbles_swapped")[0, 1] == 3.5 and R.dequantise(d, q, "q4_0", "q4_offset_omitted")[0, 0] == 0.0
    assert R.dequantise(d, q, "q4_0", "scale_from_neighbour_block")[0, 0] == -16.0
    with pytest.raises(ValueError):
        R.check_exact(x * 1e6, w * 100)
    with pytest.raises(ValueError):
        R.check_exact(x + 0.5, w)
