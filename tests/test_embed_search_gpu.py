"""K33 ``search_topk`` (csrc/kernels/embed_search.hip) against numpy: exact on integers, within the
bf16x3 bound of fp64 on unit vectors, and the same bits for a query whatever the batch around it."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

FLT_MAX = np.float32(np.finfo(np.float32).max)
SENT_I, SENT_S = -7, np.float32(123.0)  # what the output buffers hold before the call
K_CYCLE = (10, 0, 1, 64, 37)  # k_row by row: a skipped row, 1, and values above the small N


def _search(q, index, N, k_row, kmax, q_off=0, stride=None, **over):
    """(indices, scores) [rows + 1, kmax], sentinel-filled before the call; ``over`` replaces its scalar
    arguments (``rows=``, ``n=``, ``D=``, ``slots=`` for kmax), ``error=[]`` collects a HipError."""
    from triton_client_amd.ops import hip

    rows, D = q.shape
    qd = torch.zeros(q.size + 4, dtype=torch.float32, device="cuda")
    qd[q_off:q_off + q.size] = torch.from_numpy(np.array(q)).cuda().reshape(-1)
    kd = torch.tensor(list(k_row) + [64], dtype=torch.int32, device="cuda")
    a = dict(rows=rows, n=N, D=D, slots=kmax, error=None)
    a.update(over)
    ws = torch.zeros(max(8, hip.search_workspace(min(a["rows"], 128), max(a["n"], 1))), dtype=torch.uint8, device="cuda")
    idx = torch.full((rows + 1, kmax), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((rows + 1, kmax), float(SENT_S), dtype=torch.float32, device="cuda")
    try:
        hip.search_topk(qd.data_ptr() + 4 * q_off, D * 4 if stride is None else stride, a["rows"], index[0].data_ptr(),
                        index[1].data_ptr(), a["n"], a["D"], kd.data_ptr(), a["slots"], ws.data_ptr(), idx.data_ptr(),
                        sc.data_ptr())
    except hip.HipError as e:
        if a["error"] is None:
            raise
        a["error"].append(e)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def _planned_n(rows, multi):
    """The smallest N whose plan has >= 2 slices and a short last one; ``multi``: slices of several tiles."""
    from triton_client_amd.ops import hip

    for n in range(65, 1 << 16):
        slices = hip.search_plan(rows, n)[0]
        tiles = (n + 63) // 64
        per = (tiles + slices - 1) // slices
        if slices >= 2 and n < slices * per * 64 and (per >= 2 or not multi):
            return n


@pytest.mark.parametrize("shape", [(1, 64), (63, 64), (64, 64), (65, 128), (257, 1024), "plan", "plan_multi"])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33, 128])
def test_exact_on_integers(rows, shape):
    from triton_client_amd.ops import hip

    N, D = shape if isinstance(shape, tuple) else (_planned_n(rows, shape == "plan_multi"), 64)
    rng = np.random.default_rng(rows * 1000 + N)
    q = rng.integers(-3, 4, size=(rows, D)).astype(np.float32)
    c = rng.integers(-3, 4, size=(N, D)).astype(np.float32)
    index = hip.search_index(c)
    assert index[0].shape == ((N + 63) // 64 * 64, D) and not index[1].any()  # exact in bf16: lo is zero
    k_row = [K_CYCLE[r % len(K_CYCLE)] for r in range(rows)]
    idx, sc = _search(q, index, N, k_row, 64)
    score = q.astype(np.int64) @ c.astype(np.int64).T
    order = np.argsort(-score, kind="stable", axis=1)
    want_i = np.full((rows + 1, 64), SENT_I, dtype=np.int32)
    want_s = np.full((rows + 1, 64), SENT_S, dtype=np.float32)
    for r, k in enumerate(k_row):
        n = min(k, N)
        want_i[r, :n], want_s[r, :n] = order[r, :n], score[r, order[r, :n]]
        want_i[r, n:k], want_s[r, n:k] = -1, -FLT_MAX
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(sc, want_s)


@functools.lru_cache(maxsize=None)
def _unit(n, seed):  # (fp32 unit rows [n, 1024], their index), made once
    from triton_client_amd.ops import hip

    x = np.random.default_rng(seed).standard_normal((n, 1024))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    x.setflags(write=False)
    return x, hip.search_index(x)


@pytest.mark.parametrize("N", [300, 2100])
@pytest.mark.parametrize("rows", [1, 17, 128])
def test_against_fp64_on_unit_vectors(rows, N):
    (c, index), q = _unit(N, 1), _unit(128, 2)[0][:rows]
    idx, sc = _search(q, index, N, [64] * rows, 64)
    ref = q.astype(np.float64) @ c.astype(np.float64).T
    tol = 1e-5 * np.abs(ref).max()  # the project's bf16x3 bound (test_densenet_head_gpu, test_gemm_gpu)
    for r in range(rows):
        i, s = idx[r], sc[r]
        assert len(set(i)) == 64 and i.min() >= 0 and i.max() < N  # distinct, in the corpus
        assert np.abs(s - ref[r, i]).max() <= tol
        assert all(s[j] > s[j + 1] or (s[j] == s[j + 1] and i[j] < i[j + 1]) for j in range(63))  # key order
        assert np.delete(ref[r], i).max() <= ref[r, i[63]] + 2 * tol


@pytest.mark.parametrize("b", [17, 128])
def test_a_query_and_a_corpus_row_give_the_same_bits_anywhere(b):
    from triton_client_amd.ops import hip

    N = 2100
    c = _unit(N, 1)[0].copy()
    c[[40, 70, 2000]] = c[5]  # copies in the same tile, the next tile and another slice
    per = -(-((N + 63) // 64) // hip.search_plan(b, N)[0])  # tiles per slice
    assert 70 // 64 // per != 2000 // 64 // per
    index = hip.search_index(c)
    probe = np.stack([_unit(128, 2)[0][7], c[5]])
    alone = [_search(probe[j:j + 1], index, N, [64], 64) for j in range(2)]
    for j in range(2):
        q = _unit(128, 3)[0][:b].copy()
        at = [0, 15, 16, b - 1]
        q[at] = probe[j]
        idx, sc = _search(q, index, N, [64] * b, 64)
        for r in at:
            np.testing.assert_array_equal(idx[r], alone[j][0][0])
            np.testing.assert_array_equal(sc[r].view(np.uint32), alone[j][1][0].view(np.uint32))
    i, s = alone[1]
    assert list(i[0, :4]) == [5, 40, 70, 2000] and len(set(s[0, :4].view(np.uint32))) == 1


@pytest.mark.parametrize("bad", [dict(rows=129), dict(D=96), dict(D=1088), dict(slots=65), dict(slots=0), dict(n=0),
                                 dict(q_off=1), dict(stride=64 * 4 + 4), dict(rows=0)], ids=str)
def test_a_bad_argument_raises_and_writes_nothing(bad):
    from triton_client_amd.ops import hip

    q = np.ones((2, 64), dtype=np.float32)
    error = []
    idx, sc = _search(q, hip.search_index(q), 2, [1, 1], 64, error=error, **bad)
    assert len(error) == (0 if bad == dict(rows=0) else 1)  # no rows: success without a launch
    assert (idx == SENT_I).all() and (sc == SENT_S).all()
