"""K34 off the GPU: the host-only plan and workspace size of ``search_topk_q8``, and the knob that routes to it."""

import pytest


@pytest.mark.parametrize("rows, N, want", [(1, 1, (1, 16)), (1, 65, (2, 16)), (16, 16384, (256, 16)),
                                           (17, 16384, (256, 64)), (64, 16385, (129, 64)), (65, 16384, (128, 64)),
                                           (128, 2100, (33, 64)), (128, (1 << 31) - 1, (128, 64)), (0, 5, (0, 16))])
def test_the_plan_is_a_function_of_rows_and_n(rows, N, want):
    from triton_client_amd.ops import hip

    assert hip.search_q8_plan(rows, N) == want
    with pytest.raises(hip.HipError):
        hip.search_q8_plan(129, N)


@pytest.mark.parametrize("N", [1, 300, 2100, 8192, 16384, 65536, (1 << 31) - 1])
def test_a_workspace_for_the_largest_batch_covers_every_smaller_one(N):
    """rows * slices is not monotone in rows (16,384 corpus rows: 16,384 key lists at 64 rows, 8,320 at 65)."""
    from triton_client_amd.ops import hip

    sizes = [hip.search_q8_workspace(r, N) for r in range(129)]
    assert sizes == sorted(sizes)
    assert all(sizes[r] >= r * hip.search_q8_plan(r, N)[0] * 64 * 8 + r * 64 * 4 for r in range(129))
    assert hip.search_q8_workspace(128, max(1, N // 2)) <= sizes[128]


def test_the_knob_is_registered():
    from triton_client_amd.utils import knobs

    knob = {k.name: k for k in knobs.KNOBS}["TCAMD_SEARCH_INDEX"]
    assert knob.default == "x3" and knob.test.startswith("tests/test_embed_search_q8_served_gpu.py::")
