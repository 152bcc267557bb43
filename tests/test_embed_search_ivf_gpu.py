"""K35 ``search_topk_ivf`` (csrc/kernels/embed_search_ivf.hip): exact on integers over lists of every awkward length,
K33's indices and score bits over the probed lists on unit vectors, and the same bits whatever the batch."""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_embed_search_gpu import FLT_MAX, K_CYCLE, SENT_I, SENT_S, _search, _unit  # noqa: E402  K33's helper

pytestmark = pytest.mark.gpu

LENGTHS = (1, 63, 0, 65, 130, 64)  # list starts 0, 1, 64, 64, 129, 259: off the 64-row grid; the last ends at N = 323
NP_CYCLE = (6, 1, 3, 2)  # nprobe_row by row, nlist among them
PMAX = 6  # parts: 4 at 1 row, 2 at 17, 1 at 128


def _ivf(q, ivf, k_row, nprobe_row, kmax=64, pmax=PMAX, error=None, **over):
    """(indices, scores) [rows + 1, kmax], sentinel-filled before the call; ``over`` replaces fields of the index."""
    from triton_client_amd.ops import hip

    rows = len(q)
    qd = torch.from_numpy(np.array(q)).cuda()
    kd, pd = (torch.tensor(list(v) + [64], dtype=torch.int32, device="cuda") for v in (k_row, nprobe_row))
    ws = torch.zeros(hip.search_ivf_workspace(rows, ivf["nlist"]), dtype=torch.uint8, device="cuda")
    idx = torch.full((rows + 1, min(kmax, 64)), SENT_I, dtype=torch.int32, device="cuda")
    sc = torch.full((rows + 1, min(kmax, 64)), float(SENT_S), dtype=torch.float32, device="cuda")
    try:
        hip.search_topk_ivf(qd.data_ptr(), q.shape[1] * 4, rows, dict(ivf, **over), kd.data_ptr(), pd.data_ptr(), kmax,
                            pmax, ws.data_ptr(), idx.data_ptr(), sc.data_ptr())
    except hip.HipError as e:
        if error is None:
            raise
        error.append(e)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _integers():  # (corpus, centroids, assign, index): D = 64, entries in [-3, 3]
    from triton_client_amd.ops import hip

    rng = np.random.default_rng(35)
    assign = rng.permutation(np.repeat(np.arange(len(LENGTHS)), LENGTHS))
    c = rng.integers(-3, 4, size=(len(assign), 64)).astype(np.float32)
    cent = rng.integers(-3, 4, size=(len(LENGTHS), 64)).astype(np.float32)
    return c, cent, assign, hip.search_index_ivf(c, len(LENGTHS), centroids=cent, assign=assign)


@pytest.mark.parametrize("rows", [1, 17, 128])
def test_exact_on_integers(rows):
    from triton_client_amd.ops import hip

    c, cent, assign, ivf = _integers()
    assert len(c) == 323 and ivf["offsets"].tolist() == [0, 1, 64, 64, 129, 259, 323]
    assert ivf["planes"][0].shape == (448, 64) and not ivf["planes"][1].any()
    assert [hip.search_ivf_plan(r, PMAX) for r in (1, 17, 128)] == [4, 2, 1]
    q = np.random.default_rng(rows).integers(-3, 4, size=(rows, 64)).astype(np.float32)
    k_row = [K_CYCLE[r % len(K_CYCLE)] for r in range(rows)]
    nprobe_row = [NP_CYCLE[r % len(NP_CYCLE)] for r in range(rows)]
    idx, sc = _ivf(q, ivf, k_row, nprobe_row)
    lists = np.argsort(-(q.astype(np.int64) @ cent.astype(np.int64).T), kind="stable", axis=1)
    score = q.astype(np.int64) @ c.astype(np.int64).T
    want_i = np.full((rows + 1, 64), SENT_I, dtype=np.int32)
    want_s = np.full((rows + 1, 64), SENT_S, dtype=np.float32)
    for r, k in enumerate(k_row):
        cand = np.flatnonzero(np.isin(assign, lists[r, :nprobe_row[r]]))  # ascending index
        best = cand[np.argsort(-score[r, cand], kind="stable")][:k]
        want_i[r, :len(best)], want_s[r, :len(best)] = best, score[r, best]
        want_i[r, len(best):k], want_s[r, len(best):k] = -1, -FLT_MAX
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(sc, want_s)


@functools.lru_cache(maxsize=None)
def _trained():  # 2100 unit vectors in 8 trained lists
    from triton_client_amd.ops import hip

    return hip.search_index_ivf(_unit(2100, 1)[0], 8, iters=4, seed=5)


def test_the_trained_index_puts_every_row_in_the_list_k33_ranks_first():
    ivf, c = _trained(), _unit(2100, 1)[0]
    perm, offsets = ivf["perm"].cpu().numpy(), ivf["offsets"].cpu().numpy()
    assert sorted(perm) == list(range(2100))
    assert offsets[0] == 0 and offsets[-1] == 2100 and (np.diff(offsets) >= 0).all()
    first = np.concatenate([_search(c[at:at + 128], ivf["cent"], 8, [1] * len(c[at:at + 128]), 1)[0][:-1, 0]
                            for at in range(0, 2100, 128)])
    for l in range(8):
        members = perm[offsets[l]:offsets[l + 1]]
        assert (np.diff(members) > 0).all() and (first[members] == l).all()


@pytest.mark.parametrize("rows", [1, 17])
def test_k33s_bits_on_unit_vectors(rows):
    from triton_client_amd.ops import hip

    ivf, (c, index), q = _trained(), _unit(2100, 1), _unit(128, 2)[0][:rows]
    idx, sc = _ivf(q, ivf, [64] * rows, [8] * rows, pmax=8)  # every list: K33 over the whole corpus
    want = _search(q, index, 2100, [64] * rows, 64)
    np.testing.assert_array_equal(idx, want[0])
    np.testing.assert_array_equal(sc.view(np.uint32), want[1].view(np.uint32))
    idx, sc = _ivf(q, ivf, [64] * rows, [2] * rows, pmax=2)
    probed = _search(q, ivf["cent"], 8, [2] * rows, 2)[0]
    perm, offsets = ivf["perm"].cpu().numpy(), ivf["offsets"].cpu().numpy()
    for r in range(rows):
        sub = np.sort(np.concatenate([perm[offsets[l]:offsets[l + 1]] for l in probed[r]]))
        i, s = _search(q[r:r + 1], hip.search_index(c[sub]), len(sub), [64], 64)
        np.testing.assert_array_equal(idx[r], np.where(i[0] >= 0, sub[np.maximum(i[0], 0)], -1))
        np.testing.assert_array_equal(sc[r].view(np.uint32), s[0].view(np.uint32))


@pytest.mark.parametrize("b", [17, 128])
def test_a_query_gives_the_same_bits_in_any_batch(b):
    ivf, probe = _trained(), _unit(128, 2)[0][7:8]
    alone = _ivf(probe, ivf, [64], [3], pmax=3)
    q, at = _unit(128, 3)[0][:b].copy(), [0, 16, b - 1]
    q[at] = probe[0]
    idx, sc = _ivf(q, ivf, [64] * b, [3] * b, pmax=3)
    assert (alone[0][0] >= 0).all()
    for r in at:
        np.testing.assert_array_equal(idx[r], alone[0][0])
        np.testing.assert_array_equal(sc[r].view(np.uint32), alone[1][0].view(np.uint32))


@pytest.mark.parametrize("bad", [dict(pmax=0), dict(pmax=65), dict(kmax=65), dict(perm=1), dict(nlist=0)], ids=str)
def test_a_bad_argument_raises_and_writes_nothing(bad):
    ivf = _integers()[3]
    if "perm" in bad:  # the same values one byte off the 4-byte grid
        raw = torch.zeros(ivf["N"] * 4 + 4, dtype=torch.uint8, device="cuda")
        raw[1:-3] = ivf["perm"].view(torch.uint8)
        bad = dict(perm=raw[1:])
    error = []
    idx, sc = _ivf(np.ones((2, 64), dtype=np.float32), ivf, [1, 1], [1, 1], error=error, **bad)
    assert len(error) == 1 and (idx == SENT_I).all() and (sc == SENT_S).all()
