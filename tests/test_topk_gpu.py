"""K19 topk_rows (csrc/kernels/topk.hip) against numpy: row r gets its
min(k_row[r], C) best {score, index} pairs in the order of
np.argsort(-row, kind="stable"), scores bit-equal, and nothing else in the
pairs buffer is written."""

import numpy as np
import pytest

from .classify_cases import special_rows

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


@pytest.fixture(scope="module")
def hip():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from triton_client_amd.ops import hip as h

    h.lib()
    return h


def _expected(x, k_row, kmax):
    """The whole pairs buffer as uint32 [rows, kmax, 2], untouched slots = SENTINEL."""
    rows, C = x.shape
    exp = np.full((rows, kmax, 2), SENTINEL, dtype=np.uint32)
    for r in range(rows):
        k = min(int(k_row[r]), C)
        if k <= 0:
            continue
        idx = np.argsort(-x[r], kind="stable")[:k]
        # the stable tie rule makes the reference unambiguous: equal scores ascend in index
        order = -x[r][idx].astype(np.float64)
        for a, b in zip(range(k - 1), range(1, k)):
            if order[a] == order[b]:
                assert idx[a] < idx[b]
        exp[r, :k, 0] = x[r][idx].view(np.uint32)
        exp[r, :k, 1] = idx.astype(np.uint32)
    return exp


def _run(hip, x, k_row, kmax, stride_elems=None, base_offset_elems=0):
    """x: numpy fp32 [rows, C] placed on the device with the given row stride / base offset."""
    rows, C = x.shape
    stride = C if stride_elems is None else stride_elems
    buf = torch.zeros(rows * stride + base_offset_elems + 4, dtype=torch.float32, device="cuda")
    host = np.zeros(rows * stride, dtype=np.float32)
    for r in range(rows):
        host[r * stride: r * stride + C] = x[r]
    # copy bit patterns, not values: NaN payloads must survive
    buf[base_offset_elems: base_offset_elems + rows * stride].view(torch.int32).copy_(
        torch.from_numpy(host.view(np.int32)))
    kd = torch.from_numpy(np.asarray(k_row, dtype=np.int32)).cuda()
    pairs = torch.from_numpy(np.full((rows, kmax, 2), SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    s = torch.cuda.current_stream().cuda_stream
    hip.topk_rows(buf.data_ptr() + 4 * base_offset_elems, stride * 4, rows, C, kd.data_ptr(), kmax, pairs.data_ptr(),
                  stream=s)
    torch.cuda.synchronize()
    return pairs.cpu().numpy().view(np.uint32)


def _k_mix(rows, kmax):
    # 0 skips a row; kmax exceeds C wherever C < kmax
    return [(kmax, 0, 1, max(1, kmax // 2), kmax)[r % 5] for r in range(rows)]


_DATA = {}


def _rows_of(C):
    """33 seeded rows of C values, computed once per C: odd rows are quantized so ties are common."""
    if C not in _DATA:
        x = np.random.default_rng(1000 + C).standard_normal((33, C)).astype(np.float32)
        x[1::2] = np.round(x[1::2] * 4) / 4
        x.setflags(write=False)
        _DATA[C] = x
    return _DATA[C]


@pytest.mark.parametrize("C", [1, 3, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4096, 4097, 5000])
def test_topk_rows_matches_numpy(hip, C):
    for rows in (1, 4, 5, 33):
        x = _rows_of(C)[:rows]
        for kmax in (1, 3, 64):
            k_row = _k_mix(rows, kmax)
            got = _run(hip, x, k_row, kmax)
            np.testing.assert_array_equal(got, _expected(x, k_row, kmax), err_msg="C=%d rows=%d kmax=%d" % (C, rows, kmax))


def test_topk_rows_single_row_all_k(hip):
    # rows=1 starts at k_row = kmax in the mix above; a lone skipped row must stay untouched too
    x = _rows_of(1000)[:1]
    got = _run(hip, x, [0], 3)
    np.testing.assert_array_equal(got, _expected(x, [0], 3))


@pytest.mark.parametrize("name", sorted(special_rows()))
def test_topk_rows_special_values(hip, name):
    row = special_rows()[name]
    C = row.shape[0]
    x = np.stack([row, row[::-1]])
    for kmax in sorted({1, 3, min(C, 64), min(C + 5, 64)}):
        got = _run(hip, x, [kmax, kmax], kmax)
        np.testing.assert_array_equal(got, _expected(x, [kmax, kmax], kmax), err_msg="%s kmax=%d" % (name, kmax))


def test_topk_rows_misaligned_base_takes_dword_path(hip):
    x = np.random.default_rng(5).standard_normal((5, 1001)).astype(np.float32)
    k_row = _k_mix(5, 64)
    got = _run(hip, x, k_row, 64, base_offset_elems=1)
    np.testing.assert_array_equal(got, _expected(x, k_row, 64))


@pytest.mark.parametrize("C,stride", [(1000, 1024), (1000, 1001), (4000, 4100), (5000, 5004)])
def test_topk_rows_strided_rows(hip, C, stride):
    x = np.random.default_rng(C + stride).standard_normal((5, C)).astype(np.float32)
    k_row = _k_mix(5, 3)
    got = _run(hip, x, k_row, 3, stride_elems=stride)
    np.testing.assert_array_equal(got, _expected(x, k_row, 3))


def test_topk_rows_rejects_kmax_above_limit(hip):
    assert hip.TOPK_KMAX == 64
    x = torch.zeros(4, 100, device="cuda")
    kd = torch.full((4,), 65, dtype=torch.int32, device="cuda")
    pairs = torch.from_numpy(np.full((4, 65, 2), SENTINEL, dtype=np.uint32).view(np.int32)).cuda()
    with pytest.raises(hip.HipError) as e:
        hip.topk_rows(x.data_ptr(), 400, 4, 100, kd.data_ptr(), 65, pairs.data_ptr(),
                      stream=torch.cuda.current_stream().cuda_stream)
    assert e.value.code == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (pairs.cpu().numpy().view(np.uint32) == SENTINEL).all()  # nothing was launched
