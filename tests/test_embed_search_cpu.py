"""``embed_search`` off the GPU: the served model's ``top_k`` check, K33's host-only plan and workspace size."""

import numpy as np
import pytest


@pytest.mark.parametrize("parameters, want", [
    ({}, 10), ({"top_k": 1}, 1), ({"top_k": 64, "pooling": "cls"}, 64), ({"top_k": np.int64(7)}, 7),
    ({"top_k": 0}, None), ({"top_k": 65}, None), ({"top_k": -1}, None), ({"top_k": True}, None),
    ({"top_k": 5.0}, None), ({"top_k": "5"}, None)])
def test_request_top_k(parameters, want):
    from triton_client_amd.server.gpu_models import EmbedSearch
    from triton_client_amd.server.types import ServerError

    if want is not None:
        assert EmbedSearch.request_top_k(parameters) == want
        return
    with pytest.raises(ServerError, match="request parameter top_k must be an int in \\[1, 64\\]"):
        EmbedSearch.request_top_k(parameters)


@pytest.mark.parametrize("rows, N, slices", [(1, 1, 1), (1, 65, 2), (16, 16384, 256), (17, 16384, 128),
                                            (112, 2100, 33), (128, 2100, 17), (128, (1 << 31) - 1, 32), (0, 5, 0)])
def test_the_plan_is_a_function_of_rows_and_n(rows, N, slices):
    from triton_client_amd.ops import hip

    assert hip.search_plan(rows, N) == (slices, 16)
    with pytest.raises(hip.HipError):
        hip.search_plan(129, N)


@pytest.mark.parametrize("N", [1, 300, 2100, 2560, 4032, 65536, (1 << 31) - 1])
def test_a_workspace_for_the_largest_batch_covers_every_smaller_one(N):
    """rows * slices is not monotone in rows (2,100 corpus rows: 3,696 key lists at 112, 2,176 at 128)."""
    from triton_client_amd.ops import hip

    sizes = [hip.search_workspace(r, N) for r in range(129)]
    assert sizes == sorted(sizes) and sizes[128] <= 4096 * hip.SEARCH_KMAX * 8
    assert all(sizes[r] >= r * hip.search_plan(r, N)[0] * hip.SEARCH_KMAX * 8 for r in range(129))
    assert hip.search_workspace(128, max(1, N // 2)) <= sizes[128]
