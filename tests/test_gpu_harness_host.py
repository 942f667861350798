"""The bit comparisons of gpu_harness.py on arrays of 4 elements: what they let pass and what they must catch."""
import numpy as np
import pytest

from gpu_harness import bits_equal, same_bits

CHECKS = [(bits_equal, np.float32), (same_bits, np.float32), (same_bits, np.float64)]
IDS = ["bits_equal", "same_bits float32", "same_bits float64"]


@pytest.mark.parametrize("check, dtype", CHECKS, ids=IDS)
def test_equal_bits_pass_with_nan_in_the_same_places(check, dtype):
    ref = np.array([1.5, np.nan, -0.0, np.inf], dtype)
    check(ref.copy(), ref, "equal")
    quiet = ref.copy()
    quiet.view({4: np.uint32, 8: np.uint64}[ref.itemsize])[1] ^= 1         # another NaN payload is still NaN in the same place
    check(quiet, ref, "NaN payload")


@pytest.mark.parametrize("check, dtype", CHECKS, ids=IDS)
def test_differences_are_caught(check, dtype):
    ref = np.array([1.5, np.nan, 0.0, 3.0], dtype)
    others = {"-0.0 against 0.0": np.array([1.5, np.nan, -0.0, 3.0], dtype),
              "NaN position": np.array([np.nan, 1.5, 0.0, 3.0], dtype),
              "NaN against a number": np.array([1.5, 2.0, 0.0, 3.0], dtype),
              "one ulp": np.array([1.5, np.nan, 0.0, np.nextafter(dtype(3.0), dtype(4.0))], dtype),
              "shape": ref.reshape(2, 2)}
    for what, got in others.items():
        with pytest.raises(AssertionError):
            check(got, ref, what)
        if got.shape == ref.shape:
            with pytest.raises(AssertionError):
                check(ref, got, what + ", the other way round")
