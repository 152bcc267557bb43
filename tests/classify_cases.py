"""Rows with the values a top-K ordering can get wrong; shared by the host
(test_classify_native) and device (test_topk_gpu) classification tests."""

import numpy as np


def special_rows():
    rng = np.random.default_rng(19)
    dup = rng.standard_normal(1000).astype(np.float32)
    dup[7] = dup[500] = np.float32(9.5)
    nan_neg = np.array([0x7FC00001, 0xFFC00002], dtype=np.uint32).view(np.float32)  # +NaN, sign-negative NaN
    nans = rng.standard_normal(9).astype(np.float32)
    nans[0], nans[-1] = nan_neg[1], nan_neg[0]
    den = np.array([1e-45, -1e-45, 3e-39, 0.0, -3e-39, 1.1754942e-38], dtype=np.float32)
    return {
        "normal": rng.standard_normal(1000).astype(np.float32),
        "all_equal": np.full(17, 2.5, dtype=np.float32),
        "dup_max": dup,
        "zeros": np.array([-0.0, 0.0, -0.0], dtype=np.float32),
        "inf": np.array([1.0, -np.inf, np.inf, 3.0, -np.inf, np.inf, -7.0], dtype=np.float32),
        "nan": nans,
        "denormal": den,
        "negative": -np.abs(rng.standard_normal(33).astype(np.float32)) - 1,
        "one": np.array([4.25], dtype=np.float32),
    }
