"""``embed_search`` with ``index="ivf"``: requests of ``nprobe`` = every list, 0 and 1 share one ``execute``; the first
two get the default model's answer, the third what K35 ``search_topk_ivf`` gives it directly."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.test_embed_search_served_gpu import CORPUS, QUERIES, _request  # noqa: E402  300 rows, 3 queries

pytestmark = pytest.mark.gpu


def _loaded(**options):
    from triton_client_amd.server.gpu_models import EmbedSearch

    m = EmbedSearch(corpus=CORPUS, **options)
    m.load()
    return m


def _direct(m, q, k, nprobe):  # K35 called directly on the model's index: (indices, scores) [1, k]
    from triton_client_amd.ops import hip

    qd = torch.from_numpy(q).cuda()
    kd, pd = (torch.tensor([v], dtype=torch.int32, device="cuda") for v in (k, nprobe))
    ws = torch.zeros(hip.search_ivf_workspace(1, 4), dtype=torch.uint8, device="cuda")
    idx, sc = (torch.zeros((1, k), dtype=dt, device="cuda") for dt in (torch.int32, torch.float32))
    hip.search_topk_ivf(qd.data_ptr(), 4096, 1, m.index_ivf, kd.data_ptr(), pd.data_ptr(), k, nprobe, ws.data_ptr(),
                        idx.data_ptr(), sc.data_ptr())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy()


def _mixed_nprobe(m):
    from triton_client_amd.server.types import ServerError

    default = _loaded(index="x3")  # K33 alone, whatever the environment says
    try:
        assert default.index_ivf is None and m.index_ivf["nlist"] == 4 and m.nprobe == 8
        asked = ((4, 5), (0, 40), (1, 12), (65, 3))  # (nprobe, top_k)
        got = m.execute([_request(QUERIES[j % 3:j % 3 + 1], top_k=k, nprobe=p) for j, (p, k) in enumerate(asked)])
        assert isinstance(got[3], ServerError) and "nprobe" in got[3].msg  # it fails alone
        want = [default.execute([_request(QUERIES[j:j + 1], top_k=k)])[0] for j, (_, k) in enumerate(asked[:2])]
        want = [(w[0].data, w[1].data) for w in want] + [_direct(m, QUERIES[2:3], 12, 1)]
        for g, w, (_, k) in zip(got, want, asked):
            assert g[0].data.shape == (1, k)
            np.testing.assert_array_equal(g[0].data, w[0])
            np.testing.assert_array_equal(g[1].data.view(np.uint32), w[1].view(np.uint32))
        assert (want[2][0] >= 0).all() and not np.array_equal(  # one list of four is not the whole corpus
            want[2][0], default.execute([_request(QUERIES[2:3], top_k=12)])[0][0].data)
    finally:
        default.unload()


def test_mixed_nprobe_in_one_execute():
    m = _loaded(index="ivf", nlist=4)
    try:
        _mixed_nprobe(m)
    finally:
        m.unload()


def test_the_index_comes_from_the_environment(monkeypatch):
    monkeypatch.setenv("TCAMD_SEARCH_INDEX", "ivf")
    m = _loaded(nlist=4)
    try:
        _mixed_nprobe(m)
    finally:
        m.unload()
