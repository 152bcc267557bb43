"""K11w probe (tools/probes/k11w.hip) against the K11x test of the suite: the
same 13 shapes and the same assertions as tests/test_densenet_fp32_gpu.py's
test_x3_dense_fused (fp64 torch < 3e-5, untouched columns, two-kernel path
< 2e-5), plus K11w's own: bit for bit K11x v1's output.

K11w is not in the production library.  Build the probe library and run this
file against it:

    python tools/probes/build_variant.py --unit k11w tools/probes/k11w.hip
    TCAMD_HIP_LIB=$PWD/k12ab/libtcamd_hip_k11w.so python -m pytest tools/probes/test_k11w.py -v

Skips without a GPU, and when the loaded library has no tcamd_x3_dense_fused_ws.
"""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), HERE]

from tests.test_densenet_fp32_gpu import X3_FUSED_SHAPES, check_x3_dense_fused  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("imgs,H,K", X3_FUSED_SHAPES)
def test_x3_dense_fused_ws(imgs, H, K):
    """K11w = v1 on producer / consumer waves: bitwise v1's output."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import k11w

    if not k11w.available():
        pytest.skip(k11w.MISSING % k11w.hip.loaded_path())
    check_x3_dense_fused(k11w.x3_dense_fused_ws, imgs, H, K, bitwise_v1=True)
