"""The host twin of K26 (libtcamd_host, compiled from csrc/kernels/compare_math.h)
against the numpy rule of tests/compare_cases.py: every record field, on every
case the GPU test runs through the kernel.  CPU only."""

import os

import numpy as np
import pytest

from tests import compare_cases as cc
from triton_client_amd.ops import dtypes, host_codec

pytestmark = pytest.mark.skipif(not os.path.exists(host_codec._PATH), reason="libtcamd_host.so not built")


def _run(cases, atol=0.0, rtol=0.0):
    codec = host_codec.load()
    for at in range(0, len(cases), dtypes.COMPARE_MAX_PAIRS):
        chunk = cases[at:at + dtypes.COMPARE_MAX_PAIRS]
        pairs = [(cc.place(c["got"], c["got_off"]), cc.place(c["exp"], c["exp_off"]), c["datatype"]) for c in chunk]
        got = codec.compare_expected(pairs, atol, rtol)
        for c, rec in zip(chunk, got):
            assert rec == cc.reference(c["got"], c["exp"], c["datatype"], atol, rtol), (c["name"], atol, rtol)


def test_reference_rule_by_hand():
    """The numpy rule itself, on values worked out by hand."""
    f = lambda *v: np.array(v, np.float32).view(np.uint32)  # noqa: E731
    nan2 = np.array([0x7fc00000, 0x7fc00001], np.uint32)
    assert cc.reference(f(0.0), f(-0.0), "FP32") == (1, 0, 0.0, 0, 0x80000000)
    assert cc.reference(f(0.0), f(-0.0), "FP32", 1e-9) == (0, cc.NO_INDEX, 0.0, 0, 0)
    assert cc.reference(nan2, nan2[::-1].copy(), "FP32")[:2] == (2, 0)
    assert cc.reference(nan2, nan2[::-1].copy(), "FP32", 0, 1e-3)[:2] == (0, cc.NO_INDEX)
    assert cc.reference(f(np.inf, np.inf, 3e38), f(-np.inf, 3e38, np.inf), "FP32", 0, 10.0)[:3] == (3, 0, 0.0)
    beyond = float(np.float32(3.2500002) - 2)
    assert cc.reference(f(3.25, 3.2500002), f(2.0, 2.0), "FP32", 0.25, 0.5)[:3] == (1, 1, beyond)
    assert cc.reference(np.array([1, 2, 3], np.uint8), np.array([1, 0, 0], np.uint8), "UINT8", 5.0) == (2, 1, 0.0, 2, 0)
    half = np.array([0x0001, 0x0000], np.uint16)  # the smallest FP16 subnormal is 2^-24
    assert cc.reference(half, half[::-1].copy(), "FP16", 2.0**-24) == (0, cc.NO_INDEX, 2.0**-24, 0, 0)
    assert cc.reference(half, half[::-1].copy(), "FP16", 2.0**-25)[:2] == (2, 0)


def test_layout_cases():
    _run(cc.layout_cases())


def test_count_cases():
    _run(cc.count_cases())


@pytest.mark.parametrize("atol,rtol", [(0.0, 0.0), (cc.FLOAT_ATOL, cc.FLOAT_RTOL), (0.0, cc.FLOAT_RTOL),
                                       (cc.FLOAT_ATOL, 0.0)])
def test_float_cases(atol, rtol):
    cases = cc.float_cases()
    _run(cases, atol, rtol)
    if atol == cc.FLOAT_ATOL and rtol == cc.FLOAT_RTOL:
        # the cases hold what they are named after: at the bound passes, one ulp beyond fails
        for dt in cc.FLOATS:
            c = next(x for x in cases if x["name"] == dt + "-specials")
            ok = [cc.reference(c["got"][i:i + 1], c["exp"][i:i + 1], dt, atol, rtol)[0] == 0 for i in range(19)]
            assert ok == [True, True, True, False, False, True, True, True, True, False, False, False, False, True,
                          True, False, True, True, False], dt


def test_noise_cases():
    cases = cc.noise_cases()
    _run(cases, cc.NOISE_ATOL, cc.NOISE_RTOL)
    _run(cases)
    for c in cases:  # the noise straddles the tolerance: some elements pass on it, some fail
        n = cc.reference(c["got"], c["exp"], c["datatype"], cc.NOISE_ATOL, cc.NOISE_RTOL)[0]
        assert 0 < n < cc.reference(c["got"], c["exp"], c["datatype"])[0], c["name"]


def test_mixed_launch():
    cases = cc.mixed_launch()
    assert len(cases) == 64 and cases[31]["got"].size == 0
    _run(cases)
    _run(cases, 1e-2, 1e-2)


def test_refused_arguments():
    codec = host_codec.load()
    a = np.zeros(4, np.float32)
    assert codec.compare_expected([]) == []
    for atol, rtol in ((-1.0, 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(ValueError):
            codec.compare_expected([(a, a, "FP32")], atol, rtol)
    with pytest.raises(ValueError):
        codec.compare_expected([(a, a, "FP32")] * 65)
    with pytest.raises(ValueError):
        codec.compare_expected([(a, a, "BYTES")])
    with pytest.raises(ValueError):  # misaligned for its element
        codec.compare_expected([(cc.place(np.zeros(8, np.uint8), 1), np.zeros(8, np.uint8), "INT32")])
