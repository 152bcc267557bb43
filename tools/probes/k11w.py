"""Python binding of the K11w probe entry point, tcamd_x3_dense_fused_ws.

The symbol is not in the production library.  Build the probe library and
point TCAMD_HIP_LIB at it:

    python tools/probes/build_variant.py --unit k11w tools/probes/k11w.hip
    TCAMD_HIP_LIB=$PWD/k12ab/libtcamd_hip_k11w.so python ...
"""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from triton_client_amd.ops import hip  # noqa: E402

_SYM = "tcamd_x3_dense_fused_ws"
MISSING = ("%s is not in %%s: K11w lives in tools/probes/k11w.hip; build k12ab/libtcamd_hip_k11w.so with "
           "tools/probes/build_variant.py --unit k11w tools/probes/k11w.hip and set TCAMD_HIP_LIB to it" % _SYM)


def available():
    """Whether the loaded library exports the K11w entry point."""
    return hasattr(hip.lib(), _SYM)


def require():
    """The K11w layer function; exits saying how to build the library when the symbol is missing."""
    if not available():
        sys.exit(MISSING % hip.loaded_path())
    return x3_dense_fused_ws


def _fn():
    lib = hip.lib()
    if not hasattr(lib, _SYM):
        raise RuntimeError(MISSING % hip.loaded_path())
    fn = getattr(lib, _SYM)
    # tcamd_x3_dense_fused's signature
    fn.argtypes = ([ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_void_p])
    fn.restype = ctypes.c_int
    return fn


def x3_dense_fused_ws(x, ldx, imgs, H, W, K, s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, ldy, stream=None):
    """K11w: v1's layer (same fragments, same products in the same order) on
    768 threads: producer waves convert X into LDS stages, consumer waves run
    the MFMAs (tools/probes/k11w.hip).  Arguments as hip.x3_dense_fused."""
    rc = _fn()(x, int(ldx), int(imgs), int(H), int(W), int(K), s1, t1, w1_hi, w1_lo, b1, w2_hi, w2_lo, y, int(ldy),
               None if not stream else ctypes.c_void_p(int(stream)))
    if rc != 0:
        raise hip.HipError(rc, "x3_dense_fused_ws")
