"""The ensemble scheduler's hand-off contract (server/core._infer_ensemble):
sub-requests are marked as accepting device tensors, a direct request is not,
and what a step attaches to its output stays alive until the ensemble is done.
CPU only: the steps are tiny host models."""

import asyncio
import gc
import weakref

import numpy as np

from triton_client_amd.server.core import InferenceServer
from triton_client_amd.server.model_base import Model, TensorSpec
from triton_client_amd.server.types import InferRequest, InputTensor

SEEN = {}


class _Owner:
    pass


class _First(Model):
    name = "handoff_first"
    max_batch_size = 4
    inputs = (TensorSpec("X", "INT32", [2]),)
    outputs = (TensorSpec("Y", "INT32", [2]),)

    def execute(self, requests):
        res = []
        for r in requests:
            SEEN["first_flag"] = getattr(r, "accepts_device_outputs", False)
            o = self.out("Y", r.input("X").numpy() + 1)
            o.owner = _Owner()
            SEEN["owner"] = weakref.ref(o.owner)
            res.append([o])
        return res


class _Second(Model):
    name = "handoff_second"
    max_batch_size = 4
    inputs = (TensorSpec("Y", "INT32", [2]),)
    outputs = (TensorSpec("Z", "INT32", [2]),)

    def execute(self, requests):
        gc.collect()
        SEEN["owner_alive_in_second"] = SEEN["owner"]() is not None
        return [[self.out("Z", r.input("Y").numpy() * 2)] for r in requests]


class _Ensemble(Model):
    name = "handoff_ensemble"
    platform = "ensemble"
    max_batch_size = 4
    inputs = (TensorSpec("X", "INT32", [2]),)
    outputs = (TensorSpec("Z", "INT32", [2]),)
    ensemble_steps = [
        ("handoff_first", {"X": "X"}, {"Y": "mid"}),
        ("handoff_second", {"Y": "mid"}, {"Z": "Z"}),
    ]


def _infer(server, model, name, x):
    req = InferRequest(model_name=model, inputs=[InputTensor(name, "INT32", list(x.shape), x)])
    resp = asyncio.run(server.infer(req))
    return {o.name: o.data for o, _ in resp.outputs}


def test_ensemble_steps_may_hand_off_device_tensors_and_direct_requests_may_not():
    server = InferenceServer([_First, _Second, _Ensemble])
    server.load_all()
    try:
        x = np.array([[1, 2]], dtype=np.int32)
        SEEN.clear()
        out = _infer(server, "handoff_ensemble", "X", x)
        np.testing.assert_array_equal(out["Z"], (x + 1) * 2)
        assert SEEN["first_flag"] is True
        assert SEEN["owner_alive_in_second"] is True
        gc.collect()
        assert SEEN["owner"]() is None  # released once the ensemble has answered
        SEEN.clear()
        out = _infer(server, "handoff_first", "X", x)
        np.testing.assert_array_equal(out["Y"], x + 1)
        assert SEEN["first_flag"] is False
    finally:
        server.executor.shutdown(wait=False)
