"""resize_axis_table (the integer coordinate rule K20 resize_pack implements)
against the float64 expressions of utils.image.resize_bilinear."""

import numpy as np
import pytest

from triton_client_amd.utils.image import resize_axis_table

PAIRS = [(n_in, n_out) for n_in in range(1, 41) for n_out in range(1, 41)]
PAIRS += [(16000, 16384), (16384, 1), (3000, 224), (1, 224)]


def _float64_axis(n_out, n_in):
    """The index / weight lines of resize_bilinear, one axis."""
    s = (np.arange(n_out) + 0.5) * n_in / n_out - 0.5
    i0 = np.clip(np.floor(s).astype(int), 0, n_in - 1)
    i1 = np.clip(i0 + 1, 0, n_in - 1)
    w = np.clip(s - i0, 0, 1)
    return i0, i1, w


def test_table_matches_the_float64_reference():
    for n_in, n_out in PAIRS:
        i0, i1, num, den = resize_axis_table(n_out, n_in)
        r0, r1, rw = _float64_axis(n_out, n_in)
        assert np.array_equal(i0, r0) and np.array_equal(i1, r1), (n_in, n_out)
        assert np.abs(num / den - rw).max() <= 1e-12, (n_in, n_out)


@pytest.mark.parametrize("n", [1, 7, 224, 16384])
def test_equal_sizes_copy_through(n):
    i0, i1, num, den = resize_axis_table(n, n)
    assert np.array_equal(i0, np.arange(n)) and not num.any() and den == 2 * n


def test_terms_fit_32_bits_at_the_size_limit():
    for n_in, n_out in [(16384, 16384), (16384, 1), (1, 16384)]:
        i0, i1, num, den = resize_axis_table(n_out, n_in)
        i = np.arange(n_out, dtype=np.int64)
        assert np.abs((2 * i + 1) * n_in - n_out).max() < 2**31 and den < 2**31
        assert (0 <= num).all() and (num <= den).all()
        assert i0.min() >= 0 and i1.max() <= n_in - 1
