"""K34 ``search_topk_q8`` (csrc/kernels/embed_search_q8.hip): exact on integers, K33's bits for every pair it
returns, within the bf16x3 bound of fp64 on unit vectors with nothing better left out by the int8 shortlist, and
the same bits for a query whatever the batch around it."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_embed_search_gpu import FLT_MAX, SENT_I, SENT_S, _search, _unit  # noqa: E402  K33's helper and vectors

pytestmark = pytest.mark.gpu

K_CYCLE = (10, 0, 1, 16, 7)  # k_row by row: a skipped row, 1, the most, and values above the small N


@functools.lru_cache(maxsize=None)
def _unit_q8(n, seed):  # the int8 index of K33's cached unit vectors
    from triton_client_amd.ops import hip

    return hip.search_index_q8(_unit(n, seed)[0])


def _search_q8(q, q8, index, N, k_row, kmax, q_off=0, stride=None, **over):
    """(indices, scores) [rows + 1, slots], sentinel-filled before the call; ``over`` replaces its scalar
    arguments (``rows=``, ``n=``, ``D=``, ``kmax=``, ``slots=``), ``error=[]`` collects a HipError."""
    from triton_client_amd.ops import hip

    rows, D = q.shape
    qd = torch.zeros(q.size + 4, dtype=torch.float32, device="cuda")
    qd[q_off:q_off + q.size] = torch.from_numpy(np.array(q)).cuda().reshape(-1)
    kd = torch.tensor(list(k_row) + [16], dtype=torch.int32, device="cuda")
    a = dict(rows=rows, n=N, D=D, kmax=kmax, slots=kmax, error=None)
    a.update(over)
    ws = torch.zeros(max(8, hip.search_q8_workspace(min(a["rows"], 128), max(a["n"], 1))), dtype=torch.uint8,
                     device="cuda")
    width = max(a["slots"], 1)
    idx = torch.full((rows + 1, width), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((rows + 1, width), float(SENT_S), dtype=torch.float32, device="cuda")
    try:
        hip.search_topk_q8(qd.data_ptr() + 4 * q_off, D * 4 if stride is None else stride, a["rows"],
                           q8[0].data_ptr(), q8[1].data_ptr(), index[0].data_ptr(), index[1].data_ptr(), a["n"],
                           a["D"], kd.data_ptr(), a["kmax"], a["slots"], ws.data_ptr(), idx.data_ptr(), sc.data_ptr())
    except hip.HipError as e:
        if a["error"] is None:
            raise
        a["error"].append(e)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def _planned_n(rows, multi):
    """The smallest N whose q8 plan has >= 2 slices and a short last one; ``multi``: slices of several tiles."""
    from triton_client_amd.ops import hip

    for n in range(65, 1 << 16):
        slices = hip.search_q8_plan(rows, n)[0]
        tiles = (n + 63) // 64
        per = (tiles + slices - 1) // slices
        if slices >= 2 and n < slices * per * 64 and (per >= 2 or not multi):
            return n


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@pytest.mark.parametrize("shape", [(1, 128), (63, 128), (65, 128), (257, 1024), "plan", "plan_multi"])
@pytest.mark.parametrize("rows", [1, 16, 17, 64, 65, 128])
def test_exact_on_integers(rows, shape):
    from triton_client_amd.ops import hip

    N, D = shape if isinstance(shape, tuple) else (_planned_n(rows, shape == "plan_multi"), 128)
    rng = np.random.default_rng(rows * 100000 + N)

    def rows_of(n):  # integers in [-127, 127], one +-127 a row, the row times 2^-2 .. 2^2: scales with no rounding
        x = rng.integers(-127, 128, size=(n, D))
        x[np.arange(n), rng.integers(0, D, size=n)] = rng.choice([-127, 127], size=n)
        return (x * np.exp2(rng.integers(-2, 3, size=(n, 1)))).astype(np.float32)

    q, c = rows_of(rows), rows_of(N)
    q8 = hip.search_index_q8(c)
    assert q8[0].shape == ((N + 63) // 64 * 64, D) and q8[1].shape == q8[0].shape[:1]
    np.testing.assert_array_equal(q8[1][:N].cpu().numpy(), np.abs(c).max(1) / 127)
    np.testing.assert_array_equal(q8[0][:N].cpu().numpy() * q8[1][:N, None].cpu().numpy(), c)  # the codes are the data
    assert not q8[0][N:].any() and not q8[1][N:].any()
    k_row = [K_CYCLE[r % len(K_CYCLE)] for r in range(rows)]
    idx, sc = _search_q8(q, q8, hip.search_index(c), N, k_row, 16)
    score = q.astype(np.float64) @ c.astype(np.float64).T  # exact: integers below 2^24 times a power of two
    order = np.argsort(-score, kind="stable", axis=1)
    want_i = np.full((rows + 1, 16), SENT_I, dtype=np.int32)
    want_s = np.full((rows + 1, 16), SENT_S, dtype=np.float32)
    for r, k in enumerate(k_row):
        n = min(k, N)
        want_i[r, :n], want_s[r, :n] = order[r, :n], score[r, order[r, :n]]
        want_i[r, n:k], want_s[r, n:k] = -1, -FLT_MAX
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(sc, want_s)


@pytest.mark.parametrize("rows", [1, 17])
def test_a_corpus_within_the_shortlist_gives_k33s_answer(rows):
    from triton_client_amd.ops import hip

    rng = np.random.default_rng(40 + rows)
    q, c = (rng.standard_normal((n, 1024)).astype(np.float32) for n in (rows, 40))
    index = hip.search_index(c)
    want = _search(q, index, 40, [64] * rows, 64)
    idx, sc = _search_q8(q, hip.search_index_q8(c), index, 40, [16] * rows, 16, slots=24)  # a row stride above kmax
    np.testing.assert_array_equal(idx[:rows, :16], want[0][:rows, :16])
    np.testing.assert_array_equal(_bits(sc[:rows, :16]), _bits(want[1][:rows, :16]))
    assert (idx[:, 16:] == SENT_I).all() and (idx[rows] == SENT_I).all() and (sc[:, 16:] == SENT_S).all()


@pytest.mark.parametrize("N", [300, 2100])
@pytest.mark.parametrize("rows", [1, 17, 128])
def test_against_fp64_and_k33_on_unit_vectors(rows, N):
    (c, index), q = _unit(N, 1), _unit(128, 2)[0][:rows]
    idx, sc = _search_q8(q, _unit_q8(N, 1), index, N, [16] * rows, 16)
    k33_i, k33_s = _search(q, index, N, [64] * rows, 64)
    ref = q.astype(np.float64) @ c.astype(np.float64).T
    tol = 1e-5 * np.abs(ref).max()  # the project's bf16x3 bound (test_embed_search_gpu)
    for r in range(rows):
        i, s = idx[r], sc[r]
        assert len(set(i)) == 16 and i.min() >= 0 and i.max() < N  # distinct, in the corpus
        assert np.abs(s - ref[r, i]).max() <= tol
        assert all(s[j] > s[j + 1] or (s[j] == s[j + 1] and i[j] < i[j + 1]) for j in range(15))  # key order
        assert np.delete(ref[r], i).max() <= ref[r, i[15]] + 2 * tol  # the shortlist lost nothing that counts
        both, at, at33 = np.intersect1d(i, k33_i[r], return_indices=True)
        assert len(both) >= 1
        np.testing.assert_array_equal(_bits(s[at]), _bits(k33_s[r][at33]))  # a pair's score is K33's


@pytest.mark.parametrize("b", [17, 128])
def test_a_query_and_a_corpus_row_give_the_same_bits_anywhere(b):
    from triton_client_amd.ops import hip

    N = 2100
    c = _unit(N, 1)[0].copy()
    c[[40, 70, 2000]] = c[5]  # copies in the same tile, the next tile and another slice
    per = -(-((N + 63) // 64) // hip.search_q8_plan(b, N)[0])  # tiles per slice
    assert 70 // 64 // per != 2000 // 64 // per
    index, q8 = hip.search_index(c), hip.search_index_q8(c)
    probe = np.stack([_unit(128, 2)[0][7], c[5]])
    alone = [_search_q8(probe[j:j + 1], q8, index, N, [16], 16) for j in range(2)]
    for j in range(2):
        q = _unit(128, 3)[0][:b].copy()
        at = [r for r in (0, 15, 16, 63, 64, b - 1) if r < b]
        q[at] = probe[j]
        idx, sc = _search_q8(q, q8, index, N, [16] * b, 16)
        for r in at:
            np.testing.assert_array_equal(idx[r], alone[j][0][0])
            np.testing.assert_array_equal(_bits(sc[r]), _bits(alone[j][1][0]))
    i, s = alone[1]
    assert list(i[0, :4]) == [5, 40, 70, 2000] and len(set(_bits(s[0, :4]))) == 1


@pytest.mark.parametrize("bad", [dict(rows=129), dict(D=64), dict(D=1088), dict(kmax=17, slots=17), dict(kmax=0, slots=16),
                                 dict(kmax=8, slots=7), dict(slots=65), dict(n=0), dict(q_off=1),
                                 dict(stride=128 * 4 + 4), dict(rows=0)], ids=str)
def test_a_bad_argument_raises_and_writes_nothing(bad):
    from triton_client_amd.ops import hip

    q = np.ones((2, 128), dtype=np.float32)
    error = []
    idx, sc = _search_q8(q, hip.search_index_q8(q), hip.search_index(q), 2, [1, 1], error=error, **{"kmax": 16, **bad})
    assert len(error) == (0 if bad == dict(rows=0) else 1)  # no rows: success without a launch
    assert (idx == SENT_I).all() and (sc == SENT_S).all()
