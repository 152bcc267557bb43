"""``embed_search`` with ``index="q8"``: rows of ``top_k <= 16`` take K34, the others K33, in one ``execute``, and
every request gets what the default model gives it alone."""

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


@pytest.fixture(scope="module")
def default_model():
    m = _loaded()
    yield m
    m.unload()


def _same_as_alone(m, default_model):
    ks = (3, 16, 40)
    got = m.execute([_request(QUERIES[j:j + 1], top_k=k) for j, k in enumerate(ks)])
    for j, k in enumerate(ks):
        want = default_model.execute([_request(QUERIES[j:j + 1], top_k=k)])[0]
        assert got[j][0].data.shape == (1, k)
        np.testing.assert_array_equal(got[j][0].data, want[0].data)
        np.testing.assert_array_equal(got[j][1].data.view(np.uint32), want[1].data.view(np.uint32))


def test_mixed_top_k_in_one_execute_equals_the_default_model(default_model):
    m = _loaded(index="q8")
    try:
        assert default_model.index_q8 is None and m.index_q8[0].dtype == torch.int8
        _same_as_alone(m, default_model)
    finally:
        m.unload()


def test_the_index_comes_from_the_environment(default_model, monkeypatch):
    monkeypatch.setenv("TCAMD_SEARCH_INDEX", "q8")
    m = _loaded()
    try:
        assert m.index_q8 is not None
        _same_as_alone(m, default_model)
    finally:
        m.unload()
