"""Edge values and every code path of the client data kernels against the
host references of tests/data_kernel_cases.py: K4/K5 convert
(csrc/kernels/convert.hip), K1 synth_fill (synth.hip), K6 layout_pack
(layout.hip) and K7 batched_copy (gather.hip).

Every destination sits inside a buffer filled with a fixed byte, with at
least 64 such bytes in front of and behind it, and every read-back asserts
that those bytes are untouched.  Comparisons are bitwise unless a test says
otherwise: affine coefficients and fill ranges are dyadic, so a fused
multiply-add and two separate roundings give the same bits."""

import functools

import numpy as np
import pytest

from tests import data_kernel_cases as dk

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def env():
    import torch

    from triton_client_amd.ops import hip

    torch.cuda.set_device(0)
    return torch, hip


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


class Guarded:
    """``nbytes`` of device memory at ``ptr`` (16-byte aligned plus ``offset``)
    with canary bytes around it."""

    def __init__(self, torch, nbytes, offset=0):
        self.nbytes, self.offset = int(nbytes), offset
        self.buf = torch.full((PAD + offset + self.nbytes + PAD + 16,), CANARY, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + PAD + offset

    def read(self, dtype=np.uint8):
        raw = self.buf.cpu().numpy()
        a = PAD + self.offset
        assert (raw[:a] == CANARY).all(), "bytes in front of the destination were written"
        behind = raw[a + self.nbytes:]
        assert (behind == CANARY).all(), "bytes behind the destination were written: first at +%d" % int(
            np.flatnonzero(behind != CANARY)[0])
        return raw[a:a + self.nbytes].copy().view(dtype)


def _upload(torch, arr, offset=0):
    """Device copy of a numpy array's bytes, ``offset`` bytes past a 16-byte boundary."""
    raw = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
    t = torch.zeros(offset + raw.size + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    if raw.size:
        t[offset:offset + raw.size] = torch.from_numpy(raw.copy()).cuda()
    return t, t.data_ptr() + offset


def _first_bad(bad):
    return int(np.flatnonzero(bad)[0])


# ---------------------------------------------------------------------------
# K4 / K5 convert
# ---------------------------------------------------------------------------
ROUTES = {
    "fp32-bf16-trunc": ("FP32", "BF16", "trunc"),
    "fp32-bf16-rne": ("FP32", "BF16", "rne"),
    "fp32-fp16": ("FP32", "FP16", "rne"),
    "fp32-e4m3": ("FP32", "FP8_E4M3", "rne"),
    "fp32-e5m2": ("FP32", "FP8_E5M2", "rne"),
    "bf16-fp32": ("BF16", "FP32", "rne"),
    "fp16-fp32": ("FP16", "FP32", "rne"),
    "e4m3-fp32": ("FP8_E4M3", "FP32", "rne"),
    "e5m2-fp32": ("FP8_E5M2", "FP32", "rne"),
    "bf16-e4m3": ("BF16", "FP8_E4M3", "rne"),
}
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32}
# where the short runs start in each case set, so that 1..15 elements are all special:
# BF16 from 0x7f7f0000 (the last finite binade's ties into Inf, then Inf and NaN payloads)
_SHORT_START = {"fp32-bf16-trunc": 0x7F7F * 4, "fp32-bf16-rne": 0x7F7F * 4, "bf16-fp32": 0x7F7A, "fp16-fp32": 0x7BFA,
                "e4m3-fp32": 0x78, "e5m2-fp32": 0x78, "bf16-e4m3": 0x7F7A}
BIG_N = 8 * (2048 * 256 + 300) + 5  # a second grid-stride pass, a partial one, and a tail


@functools.lru_cache(maxsize=None)
def _route(name):
    """(source patterns, reference patterns, which inputs are compared by NaN class)."""
    src, dst, rounding = ROUTES[name]
    if src == "FP32":
        cases = dk.fp32_cases_for(dst)
        ref = dk.narrow(dk.f32(cases), dst, rounding)
        # truncation is the wire format, bit for bit: a NaN with a low-half payload becomes Inf
        nan = np.zeros(cases.size, bool) if rounding == "trunc" else dk.is_nan32(cases)
    else:
        table = dk.widen_table(src)
        cases = np.arange(table.size, dtype=_UINT[dk.SIZES[src]])
        nan = dk.is_nan_code(cases, src)
        if dst == "FP32":
            ref = table
            if src == "BF16":
                nan = np.zeros(cases.size, bool)  # exact widening keeps every payload
        else:
            ref = dk.ref_fp8(dk.f32(table), dst)
    ref = np.ascontiguousarray(ref)
    for a in (ref, nan):
        a.setflags(write=False)
    return cases, ref, nan


def _convert(env, name, data, src_off=0, dst_off=0):
    torch, hip = env
    src, dst, rounding = ROUTES[name]
    keep, sptr = _upload(torch, data, src_off)
    out = Guarded(torch, data.size * dk.SIZES[dst], dst_off)
    hip.convert(sptr, src, out.ptr, dst, data.size, rounding, _stream(torch))
    return out.read(_UINT[dk.SIZES[dst]])


def _assert_route(name, got, data, idx):
    src, dst, _ = ROUTES[name]
    _, ref_all, nan_all = _route(name)
    ref, nan = ref_all[idx], nan_all[idx]
    width = 2 * dk.SIZES[dst]
    bad = (got != ref) & ~nan
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: element %d (case %d, input 0x%x): got 0x%0*x, want 0x%0*x; %d of %d wrong" % (
            name, i, idx[i], int(data[i]), width, int(got[i]), width, int(ref[i]), int(bad.sum()), got.size))
    is_nan = dk.is_nan32(got) if dst == "FP32" else dk.is_nan_code(got, dst)
    bad = nan & ~is_nan
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: element %d (case %d, NaN input 0x%x) gave 0x%0*x, not a NaN of %s" % (
            name, i, idx[i], int(data[i]), width, int(got[i]), dst))


@pytest.mark.parametrize("name", list(ROUTES))
def test_convert_full_case_set(env, name):
    """Every stress input of the route: all ties, NaN payloads, subnormals,
    the saturation edge and the values that round to Inf (FP32 sources), every
    code (narrow sources).  Non-NaN inputs are bitwise equal to the reference,
    NaN inputs give a NaN code of the destination.  BF16 truncation is bitwise
    equal to serialize_bf16_tensor on NaNs too, so a NaN whose payload sits
    only in the low 16 bits becomes Inf: that is the reference's wire format."""
    cases, _, _ = _route(name)
    got = _convert(env, name, cases)
    src, dst, _ = ROUTES[name]
    if src == "FP32" and dst in dk.FP8_FORMATS:
        for sign, label in ((0, "+NaN"), (1, "-NaN")):
            sel = dk.is_nan32(cases) & ((cases >> 31) == sign)
            print("MEASURED %s of %s -> codes %s" % (dst, label, sorted("0x%02x" % c for c in set(got[sel].tolist()))))
    if name == "fp32-fp16":
        sub = (dk.ref_fp16(dk.f32(cases)) & 0x7C00 == 0) & (dk.ref_fp16(dk.f32(cases)) & 0x3FF != 0)
        print("MEASURED FP32->FP16 subnormal results kept: %d of %d" % (int((got[sub] & 0x3FF != 0).sum()), int(sub.sum())))
    if name == "fp16-fp32":
        sub = (cases & 0x7C00 == 0) & (cases & 0x3FF != 0)
        print("MEASURED FP16->FP32 subnormal inputs kept: %d of %d" % (int((got[sub] & 0x7FFFFFFF != 0).sum()), int(sub.sum())))
    _assert_route(name, got, cases, np.arange(cases.size))


@pytest.mark.parametrize("name", list(ROUTES))
def test_convert_short_lengths(env, name):
    """n below, at and just above one 8-element group: the tail kernel alone,
    the vector kernel alone, and both; every element a special value."""
    cases, _, _ = _route(name)
    for n in (1, 7, 8, 9, 15):
        data, idx = dk.tile_to(cases, n, _SHORT_START.get(name, 0))
        _assert_route(name, _convert(env, name, data), data, idx)


@pytest.mark.parametrize("name", list(ROUTES))
def test_convert_second_grid_stride_pass(env, name):
    """More groups than the 2048 x 256 lanes of the capped grid: a full second
    pass, a partial third one and a 5-element tail, on the tiled case set."""
    cases, _, _ = _route(name)
    data, idx = dk.tile_to(cases, BIG_N, 3)
    _assert_route(name, _convert(env, name, data), data, idx)


def test_convert_error_returns(env):
    """Misaligned pointers and unsupported pairs are refused before any launch;
    n = 0 returns without one."""
    torch, hip = env
    x = dk.f32(dk.fp32_cases_for("FP8_E4M3")[:64])
    keep, sptr = _upload(torch, x)
    for soff, doff in ((4, 0), (0, 2), (8, 8)):
        out = Guarded(torch, 64, doff)
        with pytest.raises(hip.HipError):
            hip.convert(sptr + soff, "FP32", out.ptr, "BF16", 8, "rne", _stream(torch))
        out.read()
    for src, dst in (("FP16", "BF16"), ("FP8_E5M2", "FP8_E4M3"), ("FP32", "FP32"), ("BF16", "FP16"),
                     ("FP32", "INT8"), ("UINT8", "FP32")):
        out = Guarded(torch, 256)
        with pytest.raises(hip.HipError):
            hip.convert(sptr, src, out.ptr, dst, 16, "rne", _stream(torch))
        out.read()
    out = Guarded(torch, 64)
    hip.convert(sptr, "FP32", out.ptr, "FP16", 0, "rne", _stream(torch))
    torch.cuda.synchronize()
    assert (out.buf.cpu().numpy() == CANARY).all()


# ---------------------------------------------------------------------------
# K1 synth_fill
# ---------------------------------------------------------------------------
ALL_DTYPES = list(dk.SIZES)
_SIGNED = ("INT8", "INT16", "INT32", "INT64")


def _default_range(dt):
    if dt == "BOOL":
        return 0, 1
    if dt in dk.FLOATS:
        return -2.0, 3.0  # dyadic: lo + u * 5 is exact in the kernel's double arithmetic
    return (-5, 5) if dt in _SIGNED else (3, 202)


def _fill(env, n, dt, mode, lo=0.0, hi=1.0, seed=0, stream_id=0):
    torch, hip = env
    out = Guarded(torch, n * dk.SIZES[dt])
    hip.synth_fill(out.ptr, n, dt, mode, lo, hi, seed=seed, stream_id=stream_id, stream=_stream(torch))
    return out.read(_UINT.get(dk.SIZES[dt], np.uint64))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(_UINT.get(a.dtype.itemsize, np.uint64))


def _assert_fill(got, ref, what):
    ref = _bits(ref)
    bad = got != ref
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: element %d: got 0x%x, want 0x%x; %d of %d wrong" % (
            what, i, int(got[i]), int(ref[i]), int(bad.sum()), got.size))


def _second_pass_n(dt):
    return 16 * (2048 * 256 + 77) // dk.SIZES[dt] + 1


@pytest.mark.parametrize("dt", ALL_DTYPES)
def test_synth_uniform_every_dtype_matches_reference(env, dt):
    """UNIFORM for all 15 datatypes, element for element: less than one
    16-byte chunk, whole chunks with a tail, and (one type per element size of
    1, 4 and 8 bytes) more chunks than the capped grid has lanes."""
    from triton_client_amd.ops import dtypes

    assert set(dtypes.CODES) == set(ALL_DTYPES)
    lo, hi = _default_range(dt)
    sizes = [3, 4099] + ([_second_pass_n(dt)] if dt in ("INT8", "FP32", "FP64") else [])
    for n in sizes:
        got = _fill(env, n, dt, dk.UNIFORM, lo, hi, seed=0x1234567887654321, stream_id=(7 << 32) | 9)
        ref = dk.synth_ref(n, dt, dk.UNIFORM, lo, hi, seed=0x1234567887654321, stream_id=(7 << 32) | 9)
        _assert_fill(got, ref, "%s n=%d" % (dt, n))


@pytest.mark.parametrize("dt", [d for d in ALL_DTYPES if d not in dk.FLOATS and d != "BOOL"])
def test_synth_integer_ranges(env, dt):
    """Inclusive integer ranges: a negative lo (signed types), lo == hi, spans
    that are no power of two, and a span wider than 16 bits where the type has one."""
    ranges = [(7, 7), (0, 2), (10, 109)]
    if dt in _SIGNED:
        ranges += [(-128, 127) if dt == "INT8" else (-1000, 30521), (-9, -9), (-7, -3)]
    else:
        ranges += [(0, 254)]
    if dk.SIZES[dt] >= 4:
        ranges += [(5, 3000000004) if dt in ("UINT32", "UINT64", "INT64") else (-70001, 1999999)]
    if dt == "UINT64":
        ranges += [(1 << 40, (1 << 40) + 999)]
    for lo, hi in ranges:
        got = _fill(env, 1029, dt, dk.UNIFORM, lo, hi, seed=3, stream_id=1)
        _assert_fill(got, dk.synth_ref(1029, dt, dk.UNIFORM, lo, hi, seed=3, stream_id=1), "%s [%d, %d]" % (dt, lo, hi))


@pytest.mark.parametrize("dt", ALL_DTYPES)
def test_synth_zero_and_const_every_dtype(env, dt):
    n = 4099
    _assert_fill(_fill(env, n, dt, dk.ZERO, 9.0, 9.0), dk.synth_ref(n, dt, dk.ZERO), "%s ZERO" % dt)
    value = 1 if dt == "BOOL" else 2.5 if dt in dk.FLOATS else 3
    ref = dk.synth_ref(n, dt, dk.CONST, value)
    _assert_fill(_fill(env, n, dt, dk.CONST, value), ref, "%s CONST" % dt)
    # the reference is the value itself, not just something the codec produced
    if dt in ("FP32", "FP64"):
        assert (ref == 2.5).all()
    elif dt in dk.FLOATS:
        assert (dk.f32(dk.widen_table(dt))[_bits(ref)] == 2.5).all()
    else:
        assert (ref == value).all()


def test_synth_is_repeatable_and_counts_from_the_start_of_each_call(env):
    """What the fan-out relies on: the same (seed, stream_id, n) fills the same
    bytes on every launch.  The Philox counter is the chunk index inside the
    call, so a buffer filled by two calls at a chunk-aligned split is NOT the
    one-call fill: its second part is again the start of the stream."""
    n, split = 4099, 1024
    one = _fill(env, n, "FP32", dk.UNIFORM, -2.0, 3.0, seed=21, stream_id=4)
    again = _fill(env, n, "FP32", dk.UNIFORM, -2.0, 3.0, seed=21, stream_id=4)
    np.testing.assert_array_equal(one, again)
    torch, hip = env
    out = Guarded(torch, n * 4)
    hip.synth_fill(out.ptr, split, "FP32", dk.UNIFORM, -2.0, 3.0, seed=21, stream_id=4, stream=_stream(torch))
    hip.synth_fill(out.ptr + 4 * split, n - split, "FP32", dk.UNIFORM, -2.0, 3.0, seed=21, stream_id=4,
                   stream=_stream(torch))
    two = out.read(np.uint32)
    print("MEASURED one call == two calls at a chunk-aligned split: %s" % bool((one == two).all()))
    np.testing.assert_array_equal(two[:split], one[:split])
    np.testing.assert_array_equal(two[split:], one[:n - split])
    assert (one != two).any()
    # another stream id or seed is another stream
    assert (_fill(env, n, "FP32", dk.UNIFORM, -2.0, 3.0, seed=21, stream_id=5) != one).mean() > 0.99
    assert (_fill(env, n, "FP32", dk.UNIFORM, -2.0, 3.0, seed=22, stream_id=4) != one).mean() > 0.99


@pytest.mark.parametrize("lo,hi", [(1.0, 2.0), (-3.0, 0.5)])
def test_synth_normal_fp32_matches_box_muller_elementwise(env, lo, hi):
    """NORMAL against Box-Muller in float64 on the same Philox words.  The bound
    is derived: m = sqrt(-2 ln u) <= 5.68 under the 1e-7 clamp; about eight fp32
    roundings along the chain (8 * 2^-24 * 5.68 = 2.7e-6) plus the rounding of
    the angle 2*pi*u (5.68 * 2*pi * 2^-24 = 2.1e-6) stay below 4.8e-6 * |hi|,
    and the final sum rounds once more relative to lo + hi * m.
    The measured maxima are in profiles/r8_data_kernel_edges.md."""
    n = 262147
    got = _fill(env, n, "FP32", dk.NORMAL, lo, hi, seed=4, stream_id=2).view(np.float32)
    ref = dk.synth_ref(n, "FP32", dk.NORMAL, lo, hi, seed=4, stream_id=2)
    err = np.abs(got.astype(np.float64) - ref)
    atol = 1e-5 * abs(hi) + 2.0 ** -22 * abs(lo)
    print("MEASURED NORMAL lo=%g hi=%g: max |err| %.3g (bound %.3g), mean %.4f std %.4f" % (
        lo, hi, err.max(), atol, got.mean(), got.std()))
    assert np.isfinite(got).all()
    assert err.max() <= atol, "element %d: got %r want %r" % (int(err.argmax()), got[err.argmax()], ref[err.argmax()])


# ---------------------------------------------------------------------------
# K6 layout_pack
# ---------------------------------------------------------------------------
_STORE = {"FP32": np.uint32, "BF16": np.uint16, "FP16": np.uint16, "UINT8": np.uint8}


def _affine(C):
    """Distinct per-channel dyadic coefficients: with 8-bit pixels every product
    and sum is a multiple of 1/64 below 2^9, exact in fp32 fused or not."""
    return [(c + 1) / 64.0 for c in range(C)], [(c - 20) / 2.0 for c in range(C)]


@functools.lru_cache(maxsize=None)
def _value_pool():
    """Finite fp32 values (no NaN, no fp32 subnormal) that are hard to narrow to 16 bits."""
    pool = np.concatenate([dk.fp32_cases_for("BF16")[::37], dk.fp32_cases_for("FP16")[::41]])
    ok = ~dk.is_nan32(pool) & (((pool & 0x7F800000) != 0) | ((pool & 0x7FFFFFFF) == 0))
    return pool[ok]


def _source(rng, dt, shape, pixels):
    """(stored bits, the fp32 values they widen to) of a canonical [N, C, H, W] batch."""
    if dt == "UINT8" or pixels:
        v = rng.integers(0, 256, shape).astype(np.float32)
        bits = v.astype(np.uint8) if dt == "UINT8" else dk.narrow(v.reshape(-1), dt).reshape(shape)
        return bits, v
    if dt == "FP32":
        bits = rng.choice(_value_pool(), shape)
        return bits, dk.f32(bits).reshape(shape)
    codes = rng.integers(0, 1 << 16, shape).astype(np.uint16)
    codes = np.where(dk.is_nan_code(codes, dt), np.uint16(0x3C00), codes)
    return codes, dk.f32(dk.widen_table(dt)[codes]).reshape(shape)


def _to_layout(a, layout):
    return np.ascontiguousarray(a if layout == "NCHW" else a.transpose(0, 2, 3, 1))


def _expected(vals, dst_dt, dst_layout, scale, bias, rounding):
    v = vals.astype(np.float64)
    if scale is not None:
        C = vals.shape[1]
        v = v * np.asarray(scale, np.float32).astype(np.float64).reshape(1, C, 1, 1) + np.asarray(
            bias, np.float32).astype(np.float64).reshape(1, C, 1, 1)
        assert (v.astype(np.float32).astype(np.float64) == v).all(), "the affine must be exact in fp32"
    out = _to_layout(v.astype(np.float32), dst_layout)
    return dk.narrow(out.reshape(-1), dst_dt, rounding)


def _pack(env, bits, src_dt, sl, dst_dt, dl, scale=None, bias=None, rounding="rne", offsets=None, ptrs=None):
    """Run layout_pack on a canonical [N, C, H, W] batch of stored bits, one
    device buffer per image (``offsets``: bytes past 16-byte alignment, per image)."""
    torch, hip = env
    N, C, H, W = bits.shape
    src = _to_layout(bits, sl)
    keep = []
    if ptrs is None:
        ptrs = []
        for i in range(N):
            t, p = _upload(torch, src[i], offsets[i] if offsets else 0)
            keep.append(t)
            ptrs.append(p)
    out = Guarded(torch, len(ptrs) * C * H * W * dk.SIZES[dst_dt])
    hip.layout_pack(ptrs, src_dt, sl, out.ptr, dst_dt, dl, C, H, W, scale=scale, bias=bias, rounding=rounding,
                    stream=_stream(torch))
    return out.read(_STORE[dst_dt])


def _assert_pack(got, want, what):
    bad = got != want
    if bad.any():
        i = _first_bad(bad)
        pytest.fail("%s: output element %d: got 0x%x, want 0x%x; %d of %d wrong" % (
            what, i, int(got[i]), int(want[i]), int(bad.sum()), got.size))


_DIRS = [("NCHW", "NHWC"), ("NHWC", "NCHW")]
_DSTS = [("FP32", "rne"), ("BF16", "rne"), ("BF16", "trunc"), ("FP16", "rne")]


@pytest.mark.parametrize("sl,dl", _DIRS)
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_layout_register_path_every_c_and_type(env, C, sl, dl):
    """C <= 4 at 8 x 8 with 3 images: every source type to every destination
    type, BF16 by rounding and by truncation, plain (hard-to-round values) and
    with a distinct affine per channel (pixels)."""
    rng = np.random.default_rng(100 + C)
    scale, bias = _affine(C)
    for src_dt in ("FP32", "UINT8", "BF16", "FP16"):
        for pixels in (False, True):
            bits, vals = _source(rng, src_dt, (3, C, 8, 8), pixels)
            sc, bi = (scale, bias) if pixels else (None, None)
            for dst_dt, rounding in _DSTS:
                got = _pack(env, bits, src_dt, sl, dst_dt, dl, sc, bi, rounding)
                _assert_pack(got, _expected(vals, dst_dt, dl, sc, bi, rounding),
                             "%s %s -> %s %s (%s) C=%d affine=%s" % (src_dt, sl, dst_dt, dl, rounding, C, pixels))


@pytest.mark.parametrize("sl,dl", _DIRS)
def test_layout_small_c_falls_back_to_tiles(env, sl, dl):
    """C = 3 leaves the register path when HW % 4 != 0 (7 x 7) or a source is
    off its 4-element alignment (8 x 8, the middle image one element off): the
    result is the reference, and bitwise the aligned register-path result."""
    rng = np.random.default_rng(7)
    scale, bias = _affine(3)
    for src_dt, dst_dt, pixels in (("FP32", "BF16", False), ("UINT8", "FP32", True), ("BF16", "FP16", True)):
        sc, bi = (scale, bias) if pixels else (None, None)
        bits, vals = _source(rng, src_dt, (3, 3, 7, 7), pixels)
        _assert_pack(_pack(env, bits, src_dt, sl, dst_dt, dl, sc, bi), _expected(vals, dst_dt, dl, sc, bi, "rne"),
                     "7x7 %s -> %s" % (src_dt, dst_dt))
        bits, vals = _source(rng, src_dt, (3, 3, 8, 8), pixels)
        aligned = _pack(env, bits, src_dt, sl, dst_dt, dl, sc, bi)
        shifted = _pack(env, bits, src_dt, sl, dst_dt, dl, sc, bi, offsets=[0, dk.SIZES[src_dt], 0])
        _assert_pack(aligned, _expected(vals, dst_dt, dl, sc, bi, "rne"), "8x8 aligned %s -> %s" % (src_dt, dst_dt))
        _assert_pack(shifted, aligned, "8x8 with image 1 one element off %s -> %s" % (src_dt, dst_dt))


@pytest.mark.parametrize("sl,dl", _DIRS)
@pytest.mark.parametrize("C,H,W", [(5, 65, 65), (64, 9, 13), (33, 9, 13)])
def test_layout_tiled_path_with_per_channel_affine(env, C, H, W, sl, dl):
    """The LDS-tiled transpose: 65 x 65 gives 67 tiles along HW for a 64-block
    grid (the tile loop runs twice, the last tile ragged); C = 64 fills a
    tile, C = 33 does not.  Every channel has its own scale and bias, so taking
    the channel from the wrong tile axis shows."""
    rng = np.random.default_rng(C * 1000 + H)
    scale, bias = _affine(C)
    for src_dt, dst_dt, pixels in (("UINT8", "FP32", True), ("FP32", "FP16", True), ("BF16", "FP32", False),
                                   ("FP16", "BF16", True)):
        sc, bi = (scale, bias) if pixels else (None, None)
        bits, vals = _source(rng, src_dt, (2, C, H, W), pixels)
        _assert_pack(_pack(env, bits, src_dt, sl, dst_dt, dl, sc, bi), _expected(vals, dst_dt, dl, sc, bi, "rne"),
                     "%s %s -> %s %s C=%d %dx%d" % (src_dt, sl, dst_dt, dl, C, H, W))


def test_layout_rejects_more_than_64_channels(env):
    torch, hip = env
    keep, p = _upload(torch, np.zeros(65 * 16, np.float32))
    out = Guarded(torch, 65 * 16 * 4)
    for sl, dl in _DIRS + [("NCHW", "NCHW")]:
        with pytest.raises(hip.HipError):
            hip.layout_pack([p], "FP32", sl, out.ptr, "FP32", dl, 65, 4, 4, stream=_stream(torch))
    with pytest.raises(hip.HipError):
        hip.layout_pack([p], "INT32", "NCHW", out.ptr, "FP32", "NHWC", 3, 4, 4, stream=_stream(torch))
    with pytest.raises(hip.HipError):
        hip.layout_pack([p], "FP32", "NCHW", out.ptr, "UINT8", "NHWC", 3, 4, 4, stream=_stream(torch))
    out.read()


@pytest.mark.parametrize("layout", ["NCHW", "NHWC"])
@pytest.mark.parametrize("C,H,W,N", [(3, 5, 6, 2), (37, 5, 6, 2), (3, 224, 224, 4)])
def test_layout_same_layout_convert_and_affine(env, layout, C, H, W, N):
    """No transpose: convert plus the per-channel affine, the channel taken from
    the flat index ((i / HW) % C for NCHW, i % C for NHWC).  3 x 224 x 224 x 4 is
    602,112 elements, past the 524,288 lanes of the capped grid."""
    rng = np.random.default_rng(C + H)
    scale, bias = _affine(C)
    for src_dt, dst_dt in (("UINT8", "FP32"), ("FP32", "BF16")):
        bits, vals = _source(rng, src_dt, (N, C, H, W), True)
        _assert_pack(_pack(env, bits, src_dt, layout, dst_dt, layout, scale, bias),
                     _expected(vals, dst_dt, layout, scale, bias, "rne"),
                     "%s -> %s %s C=%d" % (src_dt, dst_dt, layout, C))


def test_layout_more_than_64_images(env):
    """70 pointers (two launches of 64 and 6) into 10 image buffers, so most
    alias; image 64 is not the image 0 holds."""
    torch, hip = env
    rng = np.random.default_rng(70)
    bits, vals = _source(rng, "FP32", (10, 3, 8, 8), False)
    which = [(3 * i + i // 64) % 10 for i in range(70)]
    assert which[64] != which[0] and which[69] != which[5]
    keep = [_upload(torch, bits[k]) for k in range(10)]
    got = _pack(env, bits[:1], "FP32", "NCHW", "BF16", "NHWC", ptrs=[keep[k][1] for k in which]).reshape(70, -1)
    want = _expected(vals, "BF16", "NHWC", None, None, "rne").reshape(10, -1)
    for i in (63, 64, 69):
        _assert_pack(got[i], want[which[i]], "image %d" % i)
    _assert_pack(got.reshape(-1), want[which].reshape(-1), "70 images")


def test_layout_register_path_second_grid_stride_pass(env):
    """9 images of 3 x 512 x 512: 589,824 quads for 524,288 lanes."""
    torch, hip = env
    rng = np.random.default_rng(512)
    scale, bias = [1 / 128.0, 1 / 64.0, 1 / 32.0], [-1.0, 0.5, 2.0]
    bits, vals = _source(rng, "UINT8", (9, 3, 512, 512), True)
    src = _to_layout(bits, "NHWC")
    keep, base = _upload(torch, src)
    got = _pack(env, bits, "UINT8", "NHWC", "FP32", "NCHW", scale, bias,
                ptrs=[base + i * 3 * 512 * 512 for i in range(9)])
    _assert_pack(got, _expected(vals, "FP32", "NCHW", scale, bias, "rne"), "9 x 3x512x512")


@pytest.mark.parametrize("C,sl,dl", [(3, "NHWC", "NCHW"), (3, "NCHW", "NHWC"), (5, "NHWC", "NCHW"), (3, "NHWC", "NHWC")])
def test_layout_inception_coefficients_within_one_or_two_roundings(env, C, sl, dl):
    """The real INCEPTION scaling (1/127.5, -1) is not dyadic: v * scale + bias
    is one fused rounding or two separate ones.  Against the float64 result with
    the fp32 coefficients the error is at most 2^-24 * (|v * scale| + |ref|),
    which covers both forms, cancellation near zero included."""
    v = np.resize(np.arange(256, dtype=np.uint8), (2, C, 16, 16))
    v = np.ascontiguousarray(np.random.default_rng(C).permuted(v.reshape(2, -1), axis=1).reshape(2, C, 16, 16))
    scale, bias = [1 / 127.5] * C, [-1.0] * C
    got = _pack(env, v, "UINT8", sl, "FP32", dl, scale, bias).view(np.float32).astype(np.float64)
    s64 = float(np.float32(1 / 127.5))
    prod = _to_layout(v.astype(np.float64) * s64, dl).reshape(-1)
    ref = prod - 1.0
    err = np.abs(got - ref)
    bound = 2.0 ** -24 * (np.abs(prod) + np.abs(ref))
    assert (err <= bound).all(), "worst element %d: err %.3g bound %.3g" % (
        int((err - bound).argmax()), err[(err - bound).argmax()], bound[(err - bound).argmax()])


# ---------------------------------------------------------------------------
# K7 batched_copy
# ---------------------------------------------------------------------------
def _copy_case(env, sizes, src_offs, dst_offs):
    """Copy sizes[i] bytes for every i from one source buffer into ranges
    carved from one canary-filled destination with gaps of 32 bytes or more;
    returns (destination bytes, what they must be)."""
    torch, hip = env
    rng = np.random.default_rng(len(sizes))
    spos, dpos, s, d = [], [], 0, PAD
    for n, so, do in zip(sizes, src_offs, dst_offs):
        s = (s + 15) // 16 * 16 + 16
        spos.append(s + so)
        s = s + so + n
        d = (d + 15) // 16 * 16 + 32
        dpos.append(d + do)
        d = d + do + n
    src = rng.integers(0, 256, s + PAD, dtype=np.uint8)
    src[src == CANARY] = 0  # a copied byte never looks like an untouched one
    want = np.full(d + PAD, CANARY, dtype=np.uint8)
    for n, a, b in zip(sizes, spos, dpos):
        want[b:b + n] = src[a:a + n]
    d_src = torch.from_numpy(src).cuda()
    d_dst = torch.full((want.size,), CANARY, dtype=torch.uint8, device="cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    hip.batched_copy([d_src.data_ptr() + a for a in spos], [d_dst.data_ptr() + b for b in dpos], sizes,
                     _stream(torch))
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    bad = got != want
    if bad.any():
        i = _first_bad(bad)
        k = int(np.searchsorted(np.asarray(dpos), i, side="right")) - 1
        pytest.fail("destination byte %d (descriptor %d: %d bytes at +%d, %s): got 0x%02x, want 0x%02x; %d wrong" % (
            i, k, sizes[k], i - dpos[k], "inside" if i - dpos[k] < sizes[k] else "in the gap behind it",
            int(got[i]), int(want[i]), int(bad.sum())))
    return got, want


def test_batched_copy_block_cap_alignments_and_gaps(env):
    """32 descriptors in one launch: 1 MiB + 5 bytes (above the 64-block cap of
    2048 / 32 blocks x 8 KiB, so its blocks stride over it) next to 0, 1, 15,
    16, 17 and 4097 bytes; sources and destinations at every offset 0..15, in
    all four aligned / unaligned pairings; every gap stays untouched."""
    small = [0, 1, 15, 16, 17, 4097]
    sizes = [(1 << 20) + 5] + [small[i % 6] for i in range(31)]
    src_offs = [i if i < 16 else 0 for i in range(32)]
    dst_offs = [(i if i % 2 else 0) if i < 16 else i - 16 for i in range(32)]
    pairs = {(s % 16 == 0, d % 16 == 0) for s, d in zip(src_offs, dst_offs)}
    assert len(pairs) == 4 and set(src_offs) == set(range(16)) and set(dst_offs) == set(range(16))
    assert sizes[0] > 2048 // 32 * 8192
    _copy_case(env, sizes, src_offs, dst_offs)
    # the large descriptor off alignment as well: the byte loop under the block cap
    _copy_case(env, sizes, [3] + src_offs[1:], [0] + dst_offs[1:])


def test_batched_copy_chunks_of_32_and_empty_batches(env):
    """33 descriptors are two launches; the first 32 are empty and are skipped,
    the 33rd (its 16-byte count an odd multiple of the grid's lanes plus a
    tail, which ends the two-loads-in-flight loop exactly at the boundary) is
    copied.  A batch of only empty descriptors launches nothing."""
    n33 = 3 * 4096 + 5
    _copy_case(env, [0] * 32 + [n33], [0] * 33, [0] * 33)
    _copy_case(env, [0] * 32 + [n33], [i % 16 for i in range(33)], [0] * 33)
    _copy_case(env, [0] * 5, [0, 1, 2, 3, 4], [4, 3, 2, 1, 0])
    _copy_case(env, [0] * 40, [0] * 40, [0] * 40)
