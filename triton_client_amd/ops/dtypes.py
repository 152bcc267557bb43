"""Datatype codes shared with csrc/kernels/common.h, and the table / record
layouts of the compare rule (csrc/kernels/compare_math.h)."""

import ctypes

CODES = {
    "BOOL": 0,
    "INT8": 1,
    "INT16": 2,
    "INT32": 3,
    "INT64": 4,
    "UINT8": 5,
    "UINT16": 6,
    "UINT32": 7,
    "UINT64": 8,
    "FP16": 9,
    "FP32": 10,
    "FP64": 11,
    "BF16": 12,
    "FP8_E4M3": 13,
    "FP8_E5M2": 14,
}

SIZES = {
    "BOOL": 1, "INT8": 1, "UINT8": 1, "FP8_E4M3": 1, "FP8_E5M2": 1,
    "INT16": 2, "UINT16": 2, "FP16": 2, "BF16": 2,
    "INT32": 4, "UINT32": 4, "FP32": 4,
    "INT64": 8, "UINT64": 8, "FP64": 8,
}


def code(dt):
    try:
        return CODES[dt]
    except KeyError:
        raise ValueError("unsupported datatype for device kernels: %s" % dt) from None


COMPARE_MAX_PAIRS = 64  # tcamd_cmp::kMaxPairs
COMPARE_NO_INDEX = 2**64 - 1  # tcamd_cmp::kNoIndex


class ComparePair(ctypes.Structure):
    """TcamdComparePair: ``count`` elements of ``dtype`` (a code) at ``got`` against those at ``expected``."""

    _fields_ = [("got", ctypes.c_void_p), ("expected", ctypes.c_void_p), ("count", ctypes.c_uint64),
                ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class CompareRecord(ctypes.Structure):
    """TcamdCompareRecord: what one pair's comparison found."""

    _fields_ = [("mismatches", ctypes.c_uint64), ("first_index", ctypes.c_uint64), ("max_abs_diff", ctypes.c_double),
                ("got_bits", ctypes.c_uint64), ("expected_bits", ctypes.c_uint64)]

    def astuple(self):
        return (self.mismatches, self.first_index, self.max_abs_diff, self.got_bits, self.expected_bits)


def compare_table(pairs):
    """``[(got, expected, count, datatype)]`` (pointers as ints) -> a ctypes table of :class:`ComparePair`."""
    n = len(pairs)
    if n > COMPARE_MAX_PAIRS:
        raise ValueError("a compare call takes at most %d pairs, not %d" % (COMPARE_MAX_PAIRS, n))
    tab = (ComparePair * max(n, 1))()
    for i, (got, exp, count, dt) in enumerate(pairs):
        tab[i].got = int(got) or None
        tab[i].expected = int(exp) or None
        tab[i].count = int(count)
        tab[i].dtype = code(dt)
    return tab
