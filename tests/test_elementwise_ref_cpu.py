"""The NumPy references of the glue-kernel route tests (elementwise_ref.py) against the CPU oracle device, on the very graphs the GPU file runs
(elementwise_cases.py): a wrong reference, or a graph that does not say what its reference says, fails here on a machine without a GPU."""
import numpy as np
import pytest

import elementwise_ref as ref
from elementwise_cases import CASES, check_case, np_permute, run_case


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_reference_matches_oracle(sd, oracle, case):
    check_case(case, run_case(case, oracle, sd.lib()), on_oracle=True)


def test_binary_reference_is_numpy_float32():
    """the float64-then-round form of + - * / gives NumPy's (correctly rounded) float32 results bit for bit, at the edges of the format too"""
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.standard_normal(4000), [0.0, -0.0, 1e-38, 1e-45, 3e38, np.inf, 1.0, 1.0]]).astype(np.float32)
    b = np.concatenate([rng.standard_normal(4000) * 1e-3, [0.0, 0.0, 1e-45, 3.0, 3e38, 2.0, 3.0, 1e-40]]).astype(np.float32)
    with np.errstate(all="ignore"):
        for op, fn in (("add", np.add), ("sub", np.subtract), ("mul", np.multiply), ("div", np.divide)):
            ref.assert_same_bits(ref.binary(op, a, b), fn(a, b))


def test_broadcast_is_by_modulo():
    a = np.arange(2 * 3 * 4 * 6, dtype=np.float32).reshape(2, 3, 4, 6)
    b = np.arange(2 * 3, dtype=np.float32).reshape(1, 1, 2, 3) + 100   # b.ne = [3, 2, 1, 1] repeats 2 x 2 x 3 x 2 times
    want = np.empty_like(a)
    for i3 in range(2):
        for i2 in range(3):
            for i1 in range(4):
                for i0 in range(6):
                    want[i3, i2, i1, i0] = a[i3, i2, i1, i0] + b[0, 0, i1 % 2, i0 % 3]
    np.testing.assert_array_equal(ref.binary("add", a, b), want)
    np.testing.assert_array_equal(ref.repeat(b, a.shape), np.tile(b, (2, 3, 2, 2)))


def test_bf16_rounding_and_quiet_nan():
    bits = lambda *u: np.array(u, dtype=np.uint32).view(np.float32)
    x = bits(0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7F800001, 0xFFC12345, 0x80000000, 0x00008000, 0x00018000)
    want = [0x3F80, 0x3F80, 0x3F82, 0x3F81, 0x7F80, 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x8000, 0x0000, 0x0002]
    assert [int(v) for v in ref.bf16_bits(x)] == want
    np.testing.assert_array_equal(ref.bf16_to_f32(ref.bf16_bits(x[:3])), bits(0x3F800000, 0x3F800000, 0x3F820000))


def test_scale_bias_rounds_once():
    # x * s + b where rounding the product first changes the result: x * s = 1 + 2^-11 + 2^-24 exactly, a float32 tie that rounds (to even) down;
    # with b = 2^-25 the exact sum lies above the tie and rounds up
    x, s, b = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -25)
    twice = np.float32(np.float32(x * s) + b)
    once = ref.scale_bias(np.array([x]), s, b)[0]
    assert twice == np.float32(1 + 2.0 ** -11) and once == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    # an element within an ulp of a float64-then-float32 double rounding goes through exact rationals and agrees with float64 where that is exact
    r = np.random.default_rng(1).standard_normal(1000).astype(np.float32)
    np.testing.assert_array_equal(ref.scale_bias(r, 0.5, 0.0), r * np.float32(0.5))
    assert ref._round_fraction_to_f32(__import__("fractions").Fraction(16777217, 16777216)) == np.float32(1.0)       # tie to even, down
    assert ref._round_fraction_to_f32(__import__("fractions").Fraction(16777219, 16777216)) == np.float32(1 + 2.0 ** -22)   # tie to even, up


def test_layout_references_by_hand():
    a = np.arange(2 * 3, dtype=np.float32).reshape(1, 1, 2, 3)           # ne = [3, 2]
    np.testing.assert_array_equal(ref.pad_ext(a, (1, 2, 0, 1, 0, 0, 0, 0))[0, 0], [[0, 0, 1, 2, 0, 0], [0, 3, 4, 5, 0, 0], [0, 0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(ref.upscale_nearest(a, (1, 1, 4, 9))[0, 0, 0], [0, 0, 0, 1, 1, 1, 2, 2, 2])
    np.testing.assert_array_equal(ref.upscale_nearest(a, (1, 1, 4, 9))[0, 0, :, 0], [0, 0, 3, 3])
    np.testing.assert_array_equal(ref.concat(a, a + 10, 0)[0, 0], [[0, 1, 2, 10, 11, 12], [3, 4, 5, 13, 14, 15]])
    np.testing.assert_array_equal(np_permute(a, (1, 0, 2, 3))[0, 0], a[0, 0].T)
    np.testing.assert_array_equal(ref.copy(a[0, 0].T, (2, 3)), [[0, 3, 1], [4, 2, 5]])
    # im2col, 1 channel, 2 x 3 image, 2 x 2 kernel, pad 1, stride 1: the first patch holds only the image's corner, in its last (kh = 1, kw = 1) slot
    col = ref.im2col(a, 2, 2, 1, 1, 1, 1, 1, 1)
    assert col.shape == (1, 3, 4, 4)
    np.testing.assert_array_equal(col[0, 0, 0], [0, 0, 0, 0])
    np.testing.assert_array_equal(col[0, 1, 1], [0, 1, 3, 4])            # (kh, kw) = (0,0) (0,1) (1,0) (1,1): kw fastest
    np.testing.assert_array_equal(ref.timestep_embedding(np.array([0.0, 2.0]), 3, 10000), [[1, 0, 0], [np.cos(2.0), np.sin(2.0), 0]])
