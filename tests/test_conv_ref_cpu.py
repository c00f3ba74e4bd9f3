"""The conv route cases (conv_cases.py) without a GPU: is a bit-for-bit pass on the GPU worth anything?

  * the CPU oracle device, given the very graph the GPU file runs, equals conv_ref bit for bit: the reference is right, the graph says what the reference says, and
    ggml-cpu's restatement (im2col to f16, f16 x f16 products summed in f32) is exact on this data too;
  * every mutant of conv_ref.py (one indexing bug each) that applies to a case differs from conv_ref on that case's data: the case would have caught that bug;
  * every mutant applies to some case of every kernel family that can have its feature, and every epilogue appears on every family and on a split launch.

Bar: bit for bit (np.array_equal).  Exactness bound (asserted by conv_ref for every case): max|x| * max|w| * K + |epilogue terms| < 2^24 in units of the operands'
common power of two.  83 cases, 169 tests, about a minute on 8 cores.  The mutants run on the first and last four output channels only (a difference anywhere proves
the point)."""
import numpy as np
import pytest

import conv_ref
from conv_cases import CASES, EPILOGUES, case_reference, check_case, ref_kwargs, run_case

# features a kernel family cannot have at all
IMPOSSIBLE = {
    "c3w": {"tail_rows_bias_only": "the window kernel takes whole 256-position tiles only", "upscale_off_by_one": "conv3w_plan refuses upscaled inputs",
            "stride2_starts_at_1": "conv3w_plan refuses stride 2"},
    "t256": {"drop_last_block_of_a_slice": "the default policy never splits a 256 x 128 / 256 x 160 launch: it has more than splitk_target / 2 workgroups"},
}
FAMILIES = ("c3w", "pipe", "t256", "t128")


def _applies(mutant, case):
    OH, OW = case.out_hw
    return conv_ref.mutant_applies(mutant, N=case.N, IC=case.IC, OC=case.OC, OH=OH, OW=OW, ks=case.ks, stride=case.stride, upscale=case.upscale, S=case.slices)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_oracle_equals_reference(sd, oracle, case):
    check_case(case, run_case(case, oracle, sd.lib()))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_mutants_differ_from_reference(case):
    d, want = case_reference(case)
    sel = np.unique(np.r_[np.arange(min(4, case.OC)), np.arange(max(0, case.OC - 4), case.OC)])
    k = ref_kwargs(case, d)
    if k["bias"] is not None:
        k["bias"] = k["bias"][sel]
    if k["chan_add"] is not None:
        k["chan_add"] = k["chan_add"][:, sel]
    if k["residual"] is not None:
        k["residual"] = k["residual"][:, sel]
    np.testing.assert_array_equal(conv_ref.conv_ref(d["x"], d["w"][sel], case.stride, case.ks // 2, **k), want[:, sel])   # the channel subset itself changes nothing
    for m in conv_ref.MUTANTS:
        if _applies(m, case):
            got = conv_ref.conv_ref(d["x"], d["w"][sel], case.stride, case.ks // 2, mutant=m, S=case.slices, **k)
            assert not np.array_equal(got, want[:, sel]), f"{case.id}: the data of this case does not tell {m} from the truth"


def test_every_mutant_applies_on_every_family():
    for fam in FAMILIES:
        for m in conv_ref.MUTANTS:
            if m in IMPOSSIBLE.get(fam, {}):
                assert not any(_applies(m, c) for c in CASES if c.family == fam), (fam, m)
                continue
            assert any(_applies(m, c) for c in CASES if c.family == fam), f"no case of family {fam} has the feature {m} breaks"


def test_every_epilogue_on_every_family_and_on_a_split_launch():
    for e in EPILOGUES:
        for fam in FAMILIES:
            assert any(c.epi == e and c.family == fam for c in CASES), (e, fam)
        assert any(c.epi == e and c.slices > 1 for c in CASES), (e, "split")


def test_mutants_by_hand():
    """1 channel, 3 x 3 image of 1 .. 9, 3 x 3 kernel that picks one tap: the reference and three mutants on values that can be read off"""
    x = np.arange(1, 10, dtype=np.float32).reshape(1, 1, 3, 3)
    x2 = np.concatenate([x, x + 10])
    pick = lambda kh, kw: np.array([[[[float((a, b) == (kh, kw)) for b in range(3)] for a in range(3)]]], dtype=np.float32)
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(1, 1), 1, 1)[0, 0], x[0, 0])                                   # centre tap: identity
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(0, 1), 1, 1)[0, 0], [[0, 0, 0], [1, 2, 3], [4, 5, 6]])         # the row above, zero halo
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(0, 1), 1, 1, mutant="swap_taps")[0, 0], [[0, 1, 2], [0, 4, 5], [0, 7, 8]])   # (1, 0): the column to the left
    np.testing.assert_array_equal(conv_ref.conv_ref(x2, pick(0, 1), 1, 1, mutant="halo_from_neighbour_image")[1, 0], [[7, 8, 9], [11, 12, 13], [14, 15, 16]])
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(1, 0), 1, 1, mutant="halo_from_wrapped_row")[0, 0], [[0, 1, 2], [3, 4, 5], [6, 7, 8]])
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(1, 1), 2, 1)[0, 0], [[1, 3], [7, 9]])
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(1, 1), 2, 1, mutant="stride2_starts_at_1")[0, 0], [[5, 0], [0, 0]])
    up = conv_ref.conv_ref(x, pick(1, 1), 1, 1, upscale2x=True)[0, 0]
    np.testing.assert_array_equal(up[:, 0], [1, 1, 4, 4, 7, 7])
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(1, 1), 1, 1, upscale2x=True, mutant="upscale_off_by_one")[0, 0][:, 0], [1, 4, 4, 7, 7, 7])
    np.testing.assert_array_equal(conv_ref.conv_ref(x, pick(1, 1), 1, 1, bias=np.array([5.0]), residual=x, pre_scale=0.5, post_scale=2.0)[0, 0], 2 * x[0, 0] + 5)
    with pytest.raises(ValueError):
        conv_ref.conv_ref(x * 1e6, pick(1, 1) * 100, 1, 1)      # 9e6 * 100 * 9 >= 2^24
    with pytest.raises(ValueError):
        conv_ref.conv_ref(x + 0.5, pick(1, 1), 1, 1)            # not integer-valued
