"""Inputs and host references for the client data kernels (K1 synth_fill,
K4/K5 convert, K6 layout_pack): the fp32 bit patterns at which a narrowing
conversion can go wrong, and plain numpy references of every operation.
Shared by test_data_kernel_cases (CPU checks of these references) and
test_data_kernels_edges_gpu (the kernels against them).  numpy only."""

import functools

import numpy as np

from tests.philox_ref import raw_u32
from tritonclient.utils import (
    deserialize_bf16_tensor,
    deserialize_fp8_tensor,
    serialize_bf16_tensor,
    serialize_fp8_tensor,
)

FP8_FORMATS = ("FP8_E4M3", "FP8_E5M2")
# first code above the finite ones, per sign (E4M3: 0x7f is the NaN; E5M2: 0x7c is Inf)
_FP8_FINITE = {"FP8_E4M3": 0x7F, "FP8_E5M2": 0x7C}
_FP8_EDGE = {"FP8_E4M3": (448.0, 449.0, 464.0, 465.0, 480.0), "FP8_E5M2": (57344.0, 61440.0, 65536.0)}

SIZES = {
    "BOOL": 1, "INT8": 1, "UINT8": 1, "FP8_E4M3": 1, "FP8_E5M2": 1,
    "INT16": 2, "UINT16": 2, "FP16": 2, "BF16": 2,
    "INT32": 4, "UINT32": 4, "FP32": 4,
    "INT64": 8, "UINT64": 8, "FP64": 8,
}
# numpy container of one element's bits
STORAGE = {
    "BOOL": np.uint8, "INT8": np.int8, "UINT8": np.uint8, "FP8_E4M3": np.uint8, "FP8_E5M2": np.uint8,
    "INT16": np.int16, "UINT16": np.uint16, "FP16": np.uint16, "BF16": np.uint16,
    "INT32": np.int32, "UINT32": np.uint32, "FP32": np.float32,
    "INT64": np.int64, "UINT64": np.uint64, "FP64": np.float64,
}
FLOATS = ("FP16", "FP32", "FP64", "BF16", "FP8_E4M3", "FP8_E5M2")

ZERO, CONST, UNIFORM, NORMAL = 0, 1, 2, 3


def f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def bits32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def is_nan32(bits):
    return (np.asarray(bits, dtype=np.uint32) & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


# ---------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------
def _with_neighbours(pos_vals):
    """Both signs of: the values, the midpoints of neighbours (exact in fp32),
    and each midpoint's fp32 predecessor and successor."""
    v = np.asarray(pos_vals, dtype=np.float64)
    mid = ((v[:-1] + v[1:]) * 0.5).astype(np.float32)
    assert (mid.astype(np.float64) * 2 == v[:-1] + v[1:]).all()  # midpoints are exact
    mb = mid.view(np.uint32)
    pos = np.concatenate([v.astype(np.float32).view(np.uint32), mb, mb - np.uint32(1), mb + np.uint32(1)])
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


_NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFC12345], dtype=np.uint32)
_SUBNORMALS = bits32(np.array([1e-45, -1e-45], dtype=np.float32))


@functools.lru_cache(maxsize=None)
def fp32_cases_for(dst):
    """fp32 bit patterns (uint32, read-only) that stress FP32 -> ``dst``.  The
    hand-picked edge values come first, so a short prefix is already special."""
    if dst == "BF16":
        b = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
        out = np.stack([b, b | np.uint32(0x7FFF), b | np.uint32(0x8000), b | np.uint32(0x8001)], axis=1).reshape(-1)
    elif dst == "FP16":
        finite = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
        extra = np.array([65519.996, 65520.0, 65536.0, 1e38, np.inf, -np.inf, 2.0 ** -25, 0, 1e-45, -65520.0,
                          -65519.996], dtype=np.float32).view(np.uint32).copy()
        extra[7] = extra[6] + 1  # the successor of 2^-25: the smallest value that rounds up to 2^-24
        out = np.concatenate([extra, _NANS[:4], _with_neighbours(finite)])
    elif dst in FP8_FORMATS:
        finite = deserialize_fp8_tensor(np.arange(_FP8_FINITE[dst], dtype=np.uint8).tobytes(), dst)
        edge = np.array(_FP8_EDGE[dst], dtype=np.float32)
        extra = np.concatenate([edge, -edge, np.array([1e30, -1e30, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)])
        sub = np.concatenate([_SUBNORMALS, np.array([0x007FFFFF, 0x807FFFFF], dtype=np.uint32)])
        out = np.concatenate([extra.view(np.uint32), _NANS[:4], sub, _with_neighbours(finite)])
    else:
        raise ValueError(dst)
    out = np.ascontiguousarray(out, dtype=np.uint32)
    out.setflags(write=False)
    return out


def tile_to(cases, n, start=0):
    """``n`` cases, cycling through the set from index ``start``; also returns
    the case index of every element (for failure messages)."""
    idx = (np.arange(n, dtype=np.int64) + start) % cases.size
    return cases[idx], idx


# ---------------------------------------------------------------------------
# conversion references
# ---------------------------------------------------------------------------
def ref_bf16_trunc(bits):
    """The wire format: the high half of the fp32 word, whatever it is."""
    return (np.asarray(bits, dtype=np.uint32) >> np.uint32(16)).astype(np.uint16)


def ref_bf16_rne(bits):
    """Round to nearest even on the integer pattern; a NaN keeps its high
    payload bits and gets the quiet bit."""
    u = np.asarray(bits, dtype=np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    r = np.where(is_nan32(bits), (u >> np.uint64(16)) | np.uint64(0x40), r)
    return (r & np.uint64(0xFFFF)).astype(np.uint16)


def ref_fp16(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def ref_fp8(x, fmt):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if not x.size:
        return np.empty(0, np.uint8)
    with np.errstate(invalid="ignore"):  # signalling NaN inputs
        return np.frombuffer(serialize_fp8_tensor(x, fmt).item(), dtype=np.uint8)


def is_nan_code(codes, fmt):
    """True where a 16-bit (BF16 / FP16) or 8-bit (FP8) code is a NaN."""
    c = np.asarray(codes)
    if fmt == "BF16":
        return (c & 0x7FFF) > 0x7F80
    if fmt == "FP16":
        return (c & 0x7FFF) > 0x7C00
    if fmt == "FP8_E4M3":
        return (c & 0x7F) == 0x7F
    if fmt == "FP8_E5M2":
        return (c & 0x7F) > 0x7C
    raise ValueError(fmt)


@functools.lru_cache(maxsize=None)
def widen_table(fmt):
    """fp32 bits of every code of ``fmt`` (65,536 for BF16 / FP16, 256 for FP8)."""
    if fmt == "BF16":
        out = deserialize_bf16_tensor(np.arange(1 << 16, dtype="<u2").tobytes()).view(np.uint32)
    elif fmt == "FP16":
        out = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
    else:
        out = deserialize_fp8_tensor(np.arange(256, dtype=np.uint8).tobytes(), fmt).view(np.uint32)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def narrow(x32, dt, rounding="rne"):
    """fp32 values -> the bits the kernels store for ``dt``."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    if dt == "FP32":
        return x32.view(np.uint32)
    if dt == "BF16":
        return (ref_bf16_rne if rounding == "rne" else ref_bf16_trunc)(x32.view(np.uint32))
    if dt == "FP16":
        return ref_fp16(x32)
    return ref_fp8(x32, dt)


# ---------------------------------------------------------------------------
# K1 synth_fill
# ---------------------------------------------------------------------------
def unit(raw):
    """u32_to_unit: the top 24 bits as a fp32 in [0, 1)."""
    return (np.asarray(raw, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def normal_f64(n, lo, hi, seed=0, stream_id=0):
    """NORMAL mode for a 4-byte type in float64: Box-Muller on the four words
    of each 16-byte chunk, paired as gen_values pairs them:
    (x, y) -> lo + hi * m1 * (cos, sin), (z, w) -> lo + hi * m2 * (cos, sin)."""
    nch = (n + 3) // 4
    r = raw_u32(nch * 4, 4, seed, stream_id).reshape(nch, 4)
    u = unit(r).astype(np.float64)
    tiny = float(np.float32(1e-7))
    out = np.empty((nch, 4), dtype=np.float64)
    for a, b, k in ((0, 1, 0), (2, 3, 2)):
        m = np.sqrt(-2.0 * np.log(np.maximum(u[:, a], tiny)))
        ang = 2.0 * np.pi * u[:, b]
        out[:, k] = float(np.float32(lo)) + float(np.float32(hi)) * m * np.cos(ang)
        out[:, k + 1] = float(np.float32(lo)) + float(np.float32(hi)) * m * np.sin(ang)
    return out.reshape(-1)[:n]


def synth_ref(n, dtype, mode, lo=0.0, hi=1.0, seed=0, stream_id=0):
    """What synth_fill writes: ``n`` elements in the STORAGE container of
    ``dtype`` (floats narrower than fp32 as their bit patterns)."""
    st = STORAGE[dtype]
    if mode == ZERO:
        return np.zeros(n, dtype=st)
    if mode == CONST:
        if dtype == "BOOL":
            return np.full(n, int(lo != 0), dtype=st)
        if dtype in FLOATS:
            if dtype == "FP64":
                return np.full(n, lo, dtype=np.float64)
            v = narrow(np.full(1, lo, dtype=np.float32), dtype)
            return np.full(n, v[0], dtype=v.dtype).view(st)
        return np.full(n, int(lo), dtype=np.int64).astype(st)
    if mode == NORMAL:
        if dtype != "FP32":
            raise ValueError("NORMAL reference is for FP32")
        return normal_f64(n, lo, hi, seed, stream_id)
    raw = raw_u32(n, SIZES[dtype], seed, stream_id)
    if dtype == "BOOL":
        return (raw & np.uint32(1)).astype(st)
    if dtype in FLOATS:
        v = float(lo) + unit(raw).astype(np.float64) * (float(hi) - float(lo))
        if dtype == "FP64":
            return v
        return narrow(v.astype(np.float32), dtype).view(st)
    span = int(hi) - int(lo) + 1
    v = (raw.astype(np.uint64) % np.uint64(span)).astype(np.int64) + np.int64(int(lo))
    return v.astype(st)
