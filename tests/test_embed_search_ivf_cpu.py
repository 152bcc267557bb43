"""K35 off the GPU: the host-only plan and workspace size of ``search_topk_ivf``, the served model's ``nprobe`` check."""

import numpy as np
import pytest


@pytest.mark.parametrize("rows, pmax, parts", [(1, 1, 4), (1, 64, 4), (2, 64, 2), (3, 32, 2), (4, 21, 3), (16, 16, 1),
                                               (128, 64, 1), (0, 8, 0)])
def test_the_plan_is_a_function_of_rows_and_pmax(rows, pmax, parts):
    from triton_client_amd.ops import hip

    assert hip.search_ivf_plan(rows, pmax) == parts and pmax * parts <= 256
    for bad in ((129, pmax), (rows, 0), (rows, 65)):
        with pytest.raises(hip.HipError):
            hip.search_ivf_plan(*bad)


@pytest.mark.parametrize("nlist", [1, 8, 1024, 1 << 20])
def test_a_workspace_for_the_largest_batch_covers_every_smaller_one(nlist):
    from triton_client_amd.ops import hip

    sizes = [hip.search_ivf_workspace(r, nlist) for r in range(129)]
    assert sizes == sorted(sizes)
    # the probed lists and their scores, then the coarse step's workspace or the scan's key lists
    keys = [r * 64 * hip.search_ivf_plan(r, 64) * 64 * 8 for r in range(129)]  # pmax = 64, kmax = 64
    assert all(sizes[r] >= r * 64 * 8 + max(hip.search_workspace(r, nlist), keys[r]) for r in range(1, 129))


@pytest.mark.parametrize("parameters, want", [({}, 8), ({"nprobe": 0}, 0), ({"nprobe": 64}, 64),
                                              ({"nprobe": np.int32(3)}, 3), ({"nprobe": True}, None),
                                              ({"nprobe": 65}, None), ({"nprobe": -1}, None), ({"nprobe": 4.0}, None)])
def test_request_nprobe(parameters, want):
    from triton_client_amd.server.gpu_models import EmbedSearch
    from triton_client_amd.server.types import ServerError

    if want is not None:
        assert EmbedSearch.request_nprobe(parameters) == want
    else:
        with pytest.raises(ServerError, match="nprobe"):
            EmbedSearch.request_nprobe(parameters)
