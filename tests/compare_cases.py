"""The compare rule in numpy (independently of csrc/kernels/compare_math.h, which
the host library and K26 ``compare_expected`` both compile) and the case lists
of the compare tests.  Needs numpy only.

The rule.  Exact mode (``atol == 0 and rtol == 0``; always for the integer
types, BOOL and the FP8 types): an element passes iff its bytes are identical.
Tolerance mode (FP16, BF16, FP32, FP64 when a tolerance is above 0): an element
passes when its bits are equal, or both values are NaN, or both are finite and
``|got - exp| <= atol + rtol * |exp|`` in fp32 (fp64 for FP64), product and sum
each rounded.  The record of a pair is ``(mismatches, lowest mismatching index
or NO_INDEX, largest |got - exp| over the finite pairs of a float type as a
double, bits of got there, bits of exp there)``.
"""

import numpy as np

NO_INDEX = 2**64 - 1
UNIT = 16  # bytes K26 reads per lane and step (ops.hip.compare_geometry()[0]); head and tail lie around whole units
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
WIDTH = {"BOOL": 1, "INT8": 1, "UINT8": 1, "FP8_E4M3": 1, "FP8_E5M2": 1, "INT16": 2, "UINT16": 2, "FP16": 2, "BF16": 2,
         "INT32": 4, "UINT32": 4, "FP32": 4, "INT64": 8, "UINT64": 8, "FP64": 8}
FLOATS = ("FP16", "BF16", "FP32", "FP64")
BY_WIDTH = {1: ("UINT8", "INT8", "BOOL", "FP8_E4M3"), 2: ("INT16", "FP16", "BF16"), 4: ("INT32", "FP32"),
            8: ("INT64", "FP64")}
COUNTS = (0, 1, 15, 16, 17, 255, 256, 257, 4099)
OFFSETS = ((0, 0), (1, 0), (0, 3), (1, 3))  # elements (got, expected) past a 16-byte boundary


def widen(bits, datatype):
    """The values of a float datatype's bit patterns, in the type the rule works in."""
    if datatype == "FP16":
        return bits.view(np.float16).astype(np.float32)
    if datatype == "BF16":
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return bits.view(np.float32 if datatype == "FP32" else np.float64)


def reference(got, exp, datatype, atol=0.0, rtol=0.0):
    """The record of ``got`` against ``exp``, two equal-sized arrays of the
    datatype's unsigned bit patterns."""
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1)
    assert got.dtype == exp.dtype == UINT[WIDTH[datatype]] and got.size == exp.size
    ok = got == exp
    maxd = 0.0
    if datatype in FLOATS:
        g, e = widen(got, datatype), widen(exp, datatype)
        t = g.dtype.type
        fin = np.isfinite(g) & np.isfinite(e)
        with np.errstate(all="ignore"):
            d = np.abs(g - e)
            if fin.any():
                maxd = float(d[fin].max())
            if atol > 0 or rtol > 0:
                bound = t(atol) + t(rtol) * np.abs(e)
                ok = ok | (np.isnan(g) & np.isnan(e)) | (fin & (d <= bound))
    bad = np.flatnonzero(~ok)
    if bad.size == 0:
        return (0, NO_INDEX, maxd, 0, 0)
    i = int(bad[0])
    return (int(bad.size), i, maxd, int(got[i]), int(exp[i]))


def edges(count, width, got_off):
    """Element indices around the parts K26 splits ``count`` elements into when
    got starts ``got_off`` elements past a 16-byte boundary: the first and the
    last element, the last element of the 16-byte body and the first of the tail."""
    nbytes = count * width
    head = min(nbytes, -(got_off * width) % UNIT)
    units = (nbytes - head) // UNIT
    tail0 = head // width + units * (UNIT // width)
    out = {0, count - 1}
    if units:
        out.add(tail0 - 1)
    if tail0 < count:
        out.add(tail0)
    if head:
        out.add(head // width - 1)
        out.add(min(head // width, count - 1))
    return sorted(i for i in out if 0 <= i < count)


def _random_bits(rng, datatype, count):
    w = WIDTH[datatype]
    if datatype == "BOOL":
        return rng.integers(0, 2, count).astype(np.uint8)
    if datatype in FLOATS:  # finite values of mixed magnitude
        v = (rng.standard_normal(count) * np.exp(rng.uniform(-6, 6, count))).astype(np.float32)
        if datatype == "FP16":
            return v.astype(np.float16).view(np.uint16)
        if datatype == "BF16":
            return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
        return v.view(np.uint32) if datatype == "FP32" else v.astype(np.float64).view(np.uint64)
    return rng.integers(0, 2**(8 * w), count, dtype=np.uint64, endpoint=False).astype(UINT[w]) if w < 8 else \
        rng.integers(0, 2**64, count, dtype=np.uint64, endpoint=False)


def _case(name, datatype, got, exp, got_off=0, exp_off=0):
    return {"name": name, "datatype": datatype, "got": got, "exp": exp, "got_off": got_off, "exp_off": exp_off}


def layout_cases(seed=26):
    """Every width at every count and alignment: a clean pair, and pairs with one
    flipped bit at each edge element (edges()).  Exact mode."""
    rng = np.random.default_rng(seed)
    out = []
    for w in (1, 2, 4, 8):
        for n, count in enumerate(COUNTS):
            for go, eo in OFFSETS:
                dt = BY_WIDTH[w][(n + go + eo) % len(BY_WIDTH[w])]
                exp = _random_bits(rng, dt, count)
                tag = "%s-n%d-g%d-e%d" % (dt, count, go, eo)
                out.append(_case(tag + "-clean", dt, exp.copy(), exp, go, eo))
                for i in edges(count, w, go):
                    got = exp.copy()
                    got[i] ^= UINT[w](1)
                    out.append(_case("%s-at%d" % (tag, i), dt, got, exp, go, eo))
    return out


def count_cases(seed=27):
    """Several mismatches: the count and the lowest index, on one workgroup and on several."""
    rng = np.random.default_rng(seed)
    out = []
    for dt, count in (("UINT8", 4099), ("INT16", 4099), ("INT32", 4099), ("INT64", 4099), ("INT32", 30011),
                      ("UINT8", 70001), ("FP32", 30011), ("FP64", 9001)):
        w = WIDTH[dt]
        exp = _random_bits(rng, dt, count)
        for k, (go, eo) in zip((2, 7, 64, 1000), OFFSETS):
            got = exp.copy()
            idx = rng.choice(count, size=k, replace=False)
            got[idx] ^= UINT[w](1 << (8 * w - 2))  # a float stays finite or turns non-finite: both are mismatches
            out.append(_case("%s-n%d-k%d-g%d-e%d" % (dt, count, k, go, eo), dt, got, exp, go, eo))
    return out


def _from_values(datatype, values):
    v = np.asarray(values, dtype=np.float64)
    if datatype == "FP16":
        return v.astype(np.float16).view(np.uint16)
    if datatype == "BF16":
        b = v.astype(np.float32).view(np.uint32)
        assert not (b & np.uint32(0xffff)).any(), "not a BF16 value"
        return (b >> np.uint32(16)).astype(np.uint16)
    return v.astype(np.float32).view(np.uint32) if datatype == "FP32" else v.view(np.uint64)


# exponent all ones, a payload bit below the quiet bit: two NaNs of different bits per format
_NAN = {"FP16": (0x7e00, 0x7e01), "BF16": (0x7fc0, 0x7fc1), "FP32": (0x7fc00000, 0x7fc00001),
        "FP64": (0x7ff8000000000000, 0x7ff8000000000001)}
_SUB = {"FP16": (0x0001, 0x0002, 0x03ff), "BF16": (0x0001, 0x0002, 0x007f)}  # subnormal bit patterns
_EPS = {"FP16": 2.0**-10, "BF16": 2.0**-7, "FP32": 2.0**-23, "FP64": 2.0**-52}
_MAX = {"FP16": 65504.0, "BF16": float(np.array([0x7f7f0000], np.uint32).view(np.float32)[0]),
        "FP32": float(np.finfo(np.float32).max), "FP64": float(np.finfo(np.float64).max)}
FLOAT_ATOL, FLOAT_RTOL = 0.25, 0.5  # exact in every format: at exp = 2 the bound is 1.25


def float_cases():
    """Special values pair by pair, the same arrays for both modes (the caller
    runs them with (0, 0) and with (FLOAT_ATOL, FLOAT_RTOL)): NaNs of equal and
    of different bits, NaN against a number, the two zeros, the infinities
    against each other and against the largest finite value, subnormals, and a
    difference exactly at the bound and one ulp beyond it."""
    out = []
    for dt in FLOATS:
        u = UINT[WIDTH[dt]]
        one, inf = _from_values(dt, [1.0])[0], _from_values(dt, [np.inf])[0]
        ninf, big = _from_values(dt, [-np.inf])[0], _from_values(dt, [_MAX[dt]])[0]
        pz, nz = _from_values(dt, [0.0])[0], _from_values(dt, [-0.0])[0]
        n0, n1 = u(_NAN[dt][0]), u(_NAN[dt][1])
        at = _from_values(dt, [3.25])[0]  # 3.25 - 2 = 1.25 = the bound at exp = 2
        two = _from_values(dt, [2.0])[0]
        pairs = [(n0, n0), (n0, n1), (n1, n0), (n0, one), (one, n0), (pz, nz), (nz, pz), (inf, inf), (ninf, ninf),
                 (inf, ninf), (ninf, inf), (inf, big), (big, inf), (big, big), (at, two), (u(at + 1), two),
                 (u(at - 1), two), (_from_values(dt, [0.75])[0], two), (_from_values(dt, [0.5])[0], two),
                 (one, one), (_from_values(dt, [1.0 + 2 * _EPS[dt]])[0], one)]
        for s in _SUB.get(dt, ()):
            pairs += [(u(s), pz), (pz, u(s)), (u(s), u(s)), (u(s | 0x8000), u(s))]
        if dt in ("FP32", "FP64"):  # the format's own subnormals
            pairs += [(u(1), pz), (u(1), u(3)), (u(1) | nz, u(1))]
        got = np.array([p[0] for p in pairs], dtype=u)
        exp = np.array([p[1] for p in pairs], dtype=u)
        out.append(_case(dt + "-specials", dt, got, exp))
        # each special alone as the only mismatch candidate after a run of equal elements: lowest index and bits
        for k, (g, e) in enumerate(pairs):
            base = _from_values(dt, np.arange(-18, 19) / 4.0)  # quarters: exact in every format
            out.append(_case("%s-special%d" % (dt, k), dt, np.append(base, g).astype(u), np.append(base, e).astype(u),
                             k % 2, (3 * k) % 4))
    return out


def noise_cases(seed=28):
    """Random finite values against themselves plus relative noise around the
    tolerance (NOISE_ATOL, NOISE_RTOL), on one workgroup and on several."""
    rng = np.random.default_rng(seed)
    out = []
    for dt, count in (("FP16", 4099), ("BF16", 4099), ("FP32", 4099), ("FP64", 4099), ("FP32", 30011), ("FP16", 70001)):
        exp = _random_bits(rng, dt, count)
        v = widen(exp, dt).astype(np.float64)
        noisy = v * (1.0 + rng.uniform(-2, 2, count) * NOISE_RTOL) + rng.uniform(-2, 2, count) * NOISE_ATOL
        got = np.where(rng.random(count) < 0.5, exp, _round_to(dt, noisy))
        for go, eo in ((0, 0), (1, 3)):
            out.append(_case("%s-noise-n%d-g%d-e%d" % (dt, count, go, eo), dt, got, exp, go, eo))
    return out


NOISE_ATOL, NOISE_RTOL = 1e-3, 2.0**-6


def _round_to(datatype, values):
    if datatype == "FP16":
        return values.astype(np.float16).view(np.uint16)
    if datatype == "BF16":
        return (values.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    return values.astype(np.float32).view(np.uint32) if datatype == "FP32" else values.view(np.uint64)


def mixed_launch(seed=29):
    """64 pairs of mixed datatypes, sizes and alignments for one launch, an empty
    pair in the middle."""
    rng = np.random.default_rng(seed)
    dts = ("UINT8", "FP16", "INT32", "FP64", "BF16", "INT64", "FP32", "INT16", "BOOL", "FP8_E5M2")
    out = []
    for i in range(64):
        dt = dts[i % len(dts)]
        count = 0 if i == 31 else int(rng.integers(1, 700))
        exp = _random_bits(rng, dt, count)
        got = exp.copy()
        if count and i % 3:
            idx = rng.choice(count, size=min(count, 1 + i % 5), replace=False)
            got[idx] ^= UINT[WIDTH[dt]](1)
        out.append(_case("mixed%d-%s-n%d" % (i, dt, count), dt, got, exp, i % 2, (i // 2) % 4))
    return out


def place(bits, off, align=64):
    """A copy of ``bits`` that starts ``off`` elements past an ``align``-byte
    boundary of its own buffer (so that a host pointer is misaligned as asked)."""
    w = bits.dtype.itemsize
    raw = np.zeros(bits.nbytes + off * w + align, dtype=np.uint8)
    start = -raw.ctypes.data % align + off * w
    view = raw[start:start + bits.nbytes].view(bits.dtype)
    view[:] = bits
    return view
