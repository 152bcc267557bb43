"""The host references of tests/data_kernel_cases.py against independent
implementations (torch CPU casts, the philox_ref stream), so that a failure
of test_data_kernels_edges_gpu points at a kernel and not at its reference.
No GPU."""

import numpy as np
import pytest

from tests import data_kernel_cases as dk
from tests.philox_ref import raw_u32, uniform_f32

torch = pytest.importorskip("torch")

_T8 = {"FP8_E4M3": "float8_e4m3fn", "FP8_E5M2": "float8_e5m2"}


def _t32(bits):
    return torch.from_numpy(dk.f32(bits).copy())


def _u16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_case_set_sizes():
    assert dk.fp32_cases_for("BF16").size == 262144
    assert dk.fp32_cases_for("FP16").size == 253946 + 15
    for fmt, finite in (("FP8_E4M3", 127), ("FP8_E5M2", 124)):
        n = dk.fp32_cases_for(fmt).size
        assert n == 2 * (finite + 3 * (finite - 1)) + 2 * len(dk._FP8_EDGE[fmt]) + 6 + 4 + 4
        assert 900 < n < 1100


def test_bf16_rne_matches_torch_on_every_case():
    bits = dk.fp32_cases_for("BF16")
    got = dk.ref_bf16_rne(bits)
    want = _u16(_t32(bits).to(torch.bfloat16))
    nan = dk.is_nan32(bits)
    np.testing.assert_array_equal(got[~nan], want[~nan])
    # torch canonicalises the payload, the kernel keeps its high bits: compare by class and sign
    assert dk.is_nan_code(got[nan], "BF16").all() and dk.is_nan_code(want[nan], "BF16").all()
    np.testing.assert_array_equal(got[nan] >> 15, (bits[nan] >> 31).astype(np.uint16))
    np.testing.assert_array_equal(got[nan] & 0x7F, ((bits[nan] >> 16) & 0x7F | 0x40).astype(np.uint16))


def test_bf16_trunc_is_the_wire_codec():
    from tritonclient.utils import serialize_bf16_tensor

    bits = dk.fp32_cases_for("BF16")
    wire = np.frombuffer(serialize_bf16_tensor(dk.f32(bits)).item(), dtype="<u2")
    np.testing.assert_array_equal(dk.ref_bf16_trunc(bits), wire)
    # a NaN whose payload sits in the low half only truncates to Inf: that is the wire format
    assert dk.ref_bf16_trunc(np.array([0x7F800001], np.uint32))[0] == 0x7F80


def test_fp16_matches_torch_on_every_case():
    bits = dk.fp32_cases_for("FP16")
    got = dk.ref_fp16(dk.f32(bits))
    want = _u16(_t32(bits).to(torch.float16))
    nan = dk.is_nan32(bits)
    np.testing.assert_array_equal(got[~nan], want[~nan])
    assert dk.is_nan_code(got[nan], "FP16").all() and dk.is_nan_code(want[nan], "FP16").all()
    # subnormal results are kept, the first value above half the smallest one rounds up to it
    x = np.array([2.0 ** -24, 2.0 ** -25], dtype=np.float32)
    np.testing.assert_array_equal(dk.ref_fp16(x), [1, 0])
    assert dk.ref_fp16(dk.f32(dk.bits32(x[1:]) + np.uint32(1)))[0] == 1


@pytest.mark.parametrize("fmt,limit", [("FP8_E4M3", 464.0), ("FP8_E5M2", 61440.0)])
def test_fp8_encode_matches_torch_below_saturation(fmt, limit):
    bits = dk.fp32_cases_for(fmt)
    x = dk.f32(bits)
    with np.errstate(invalid="ignore"):
        sel = np.abs(x) < limit  # saturating and non-saturating casts agree here; NaN compares false
    assert sel.sum() > 900
    got = dk.ref_fp8(x[sel], fmt)
    want = _t32(bits[sel]).to(getattr(torch, _T8[fmt])).view(torch.uint8).numpy()
    np.testing.assert_array_equal(got, want)
    # above it the codec saturates, and a NaN is a NaN code
    top = 0x7E if fmt == "FP8_E4M3" else 0x7B
    big = np.array([limit, 1e30, np.inf, -limit, -np.inf], dtype=np.float32)
    np.testing.assert_array_equal(dk.ref_fp8(big, fmt), [top, top, top, top | 0x80, top | 0x80])
    assert dk.is_nan_code(dk.ref_fp8(x[dk.is_nan32(bits)], fmt), fmt).all()


@pytest.mark.parametrize("fmt", ["BF16", "FP16", "FP8_E4M3", "FP8_E5M2"])
def test_widen_tables_match_torch(fmt):
    table = dk.widen_table(fmt)
    if fmt in _T8:
        codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
        want = codes.view(getattr(torch, _T8[fmt])).float().numpy().view(np.uint32)
        nan = dk.is_nan_code(np.arange(256), fmt)
    else:
        codes = torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.int16).copy())
        want = codes.view(torch.bfloat16 if fmt == "BF16" else torch.float16).float().numpy().view(np.uint32)
        nan = dk.is_nan_code(np.arange(1 << 16), fmt)
    assert table.size == want.size
    np.testing.assert_array_equal(table[~nan], want[~nan])
    assert dk.is_nan32(table[nan]).all() and dk.is_nan32(want[nan]).all()
    assert not dk.is_nan32(table[~nan]).any()
    if fmt == "BF16":  # exact widening, payloads included
        np.testing.assert_array_equal(table, np.arange(1 << 16, dtype=np.uint32) << 16)


@pytest.mark.parametrize("fmt", ["BF16", "FP16", "FP8_E4M3", "FP8_E5M2"])
def test_encode_of_decode_is_identity_on_finite_codes(fmt):
    table = dk.widen_table(fmt)
    codes = np.arange(table.size)
    finite = np.isfinite(dk.f32(table))
    back = dk.narrow(dk.f32(table[finite]), fmt)
    np.testing.assert_array_equal(back, codes[finite])
    if fmt == "BF16":
        np.testing.assert_array_equal(dk.narrow(dk.f32(table[finite]), fmt, "trunc"), codes[finite])


def _tie_parities(fmt, mbits):
    """{binade of the lower neighbour: set of its mantissa parities} over the ties in the case set."""
    cases = dk.fp32_cases_for(fmt)
    have = set(cases.tolist())
    if fmt == "BF16":
        out = {}
        for b in cases[(cases & 0xFFFF) == 0x8000].tolist():
            if (b & 0x7FFFFFFF) < 0x7F800000:
                out.setdefault((b >> 23) & 0xFF, set()).add((b >> 16) & 1)
        return out
    table = dk.f32(dk.widen_table(fmt))
    ncodes = table.size // 2
    pos = [c for c in range(ncodes) if np.isfinite(table[c])]
    out = {}
    for lo, hi in zip(pos[:-1], pos[1:]):
        mid = np.float32((float(table[lo]) + float(table[hi])) / 2)
        if int(mid.view(np.uint32)) in have:
            out.setdefault(lo >> mbits, set()).add(lo & 1)
    return out


@pytest.mark.parametrize("fmt,mbits,binades", [("BF16", 7, 255), ("FP16", 10, 31), ("FP8_E4M3", 3, 16),
                                               ("FP8_E5M2", 2, 31)])
def test_case_sets_hold_what_they_claim(fmt, mbits, binades):
    cases = dk.fp32_cases_for(fmt)
    ties = _tie_parities(fmt, mbits)
    assert len(ties) == binades
    assert all(p == {0, 1} for p in ties.values()), "a binade lacks a tie to even or to odd"
    nan = dk.is_nan32(cases)
    assert (cases[nan] >> 31).min() == 0 and (cases[nan] >> 31).max() == 1  # both NaN signs
    x = dk.f32(cases)
    finite_in = np.isfinite(x)
    if fmt in dk.FP8_FORMATS:
        # saturating: nothing rounds to Inf, but values past the largest code are there, and both zeros
        top = float(dk.f32(dk.widen_table(fmt))[0x7E if fmt == "FP8_E4M3" else 0x7B])
        assert (np.abs(x[finite_in]) > top).sum() >= 6
        assert 0 in cases and 0x80000000 in cases
    else:
        out = dk.narrow(x, fmt)
        inf_code = 0x7F80 if fmt == "BF16" else 0x7C00
        assert (((out & 0x7FFF) == inf_code) & finite_in).any(), "no finite value that rounds to Inf"
    if fmt == "BF16":
        assert 0x7F7F8000 in cases and dk.ref_bf16_rne(np.array([0x7F7F8000], np.uint32))[0] == 0x7F80
    # fp32 subnormal inputs
    assert ((cases & 0x7F800000) == 0).sum() > 2
    assert not cases.flags.writeable


def test_tile_to_cycles_from_start():
    cases = dk.fp32_cases_for("FP8_E4M3")
    data, idx = dk.tile_to(cases, cases.size + 5, start=7)
    assert idx[0] == 7 and idx[-1] == (7 + cases.size + 4) % cases.size
    np.testing.assert_array_equal(data, cases[idx])


def test_synth_ref_uniform_matches_the_philox_stream():
    n = 1001
    got = dk.synth_ref(n, "FP32", dk.UNIFORM, -2.0, 3.0, seed=99, stream_id=5)
    np.testing.assert_array_equal(got, uniform_f32(n, -2.0, 3.0, seed=99, stream_id=5))
    got = dk.synth_ref(n, "INT32", dk.UNIFORM, 0, 30521, seed=3)
    np.testing.assert_array_equal(got, (raw_u32(n, 4, seed=3).astype(np.int64) % 30522).astype(np.int32))
    for dt in dk.SIZES:
        lo, hi = (0, 1) if dt == "BOOL" else (-2.0, 3.0) if dt in dk.FLOATS else (-5, 99) if dt[0] == "I" else (3, 202)
        out = dk.synth_ref(n, dt, dk.UNIFORM, lo, hi, seed=1)
        assert out.dtype == np.dtype(dk.STORAGE[dt]) and out.size == n
        if dt not in dk.FLOATS:
            assert out.min() >= lo and out.max() <= hi and np.unique(out).size > 1
    assert dk.synth_ref(4, "INT8", dk.UNIFORM, -5, -5).tolist() == [-5] * 4
    assert dk.synth_ref(3, "FP16", dk.CONST, 2.5).tolist() == [0x4100] * 3
    assert dk.synth_ref(3, "FP8_E5M2", dk.CONST, 2.5).tolist() == [0x41] * 3
    assert dk.synth_ref(3, "BOOL", dk.CONST, 1).tolist() == [1] * 3


def test_synth_ref_normal_is_a_normal():
    x = dk.synth_ref(200001, "FP32", dk.NORMAL, 1.0, 2.0, seed=4)
    assert x.dtype == np.float64 and abs(x.mean() - 1.0) < 0.02 and abs(x.std() - 2.0) < 0.02
    # |m| stays under the bound the device tolerance is derived from
    assert np.abs(x - 1.0).max() <= 2.0 * 5.68
