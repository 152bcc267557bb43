"""What the GPU models of the bench server (server/gpu_models.py) share on the
host side: the pool of per-instance slots, the base classes that own it, and
the staging helpers of the host-twin stages (pinned views, input and text
staging, the output download).  Importable without a GPU: torch and
``ops.hip`` are imported inside the functions that need them.
"""

import ctypes
import threading

import numpy as np

from .model_base import Model
from .types import DeviceView, ServerError


class SlotPool:
    """The slots of a model's instances (a stream and its buffers each) and the
    free list that hands them out: a sequence of slot dicts for readers, and
    ``with pool.slot() as (i, slot)`` for a batch."""

    def __init__(self):
        self._slots = []
        self._free = []
        self._cv = threading.Condition()

    def add(self, slot):
        with self._cv:
            self._free.append(len(self._slots))
            self._slots.append(slot)
            self._cv.notify()

    def __len__(self):
        return len(self._slots)

    def __getitem__(self, i):
        return self._slots[i]

    def acquire(self):
        """The index of a free slot; blocks while there is none."""
        with self._cv:
            while not self._free:
                self._cv.wait()
            return self._free.pop()

    def release(self, i):
        with self._cv:
            self._free.append(i)
            self._cv.notify()

    def slot(self):
        """``with pool.slot() as (i, slot)``: a slot held for the body, released however it ends."""
        return _HeldSlot(self)

    def close(self, free):
        """``free(slot)`` for every slot, whatever it raises, then no slots."""
        for s in self._slots:
            try:
                free(s)
            except Exception:  # noqa: BLE001 - unloading goes on past a buffer that does not free
                pass
        self._slots = []
        self._free = []


class _HeldSlot:
    """The context manager of ``SlotPool.slot`` (a class: a generator-based one
    costs every batch 2 us more than the acquire / try / finally it replaces)."""

    __slots__ = ("pool", "i")

    def __init__(self, pool):
        self.pool = pool

    def __enter__(self):
        self.i = i = self.pool.acquire()
        return i, self.pool[i]

    def __exit__(self, *exc):
        self.pool.release(self.i)


class DeviceModel(Model):
    """A model that runs on one GPU out of a pool of slots.  The host-twin
    stages (a CPU model of the same name does the checks and, with the knob
    off, the work) also use ``_load_twin``, ``_add_stage_slots`` and the
    functions below."""

    def __init__(self, version=1, device_id=0, **kw):
        super().__init__(version, **kw)
        self.device_id = int(kw.get("device", device_id))
        self._slots = SlotPool()
        self._host = None

    def _gpu(self, error=None):
        """(torch, hip, device) once there is a GPU and the native library loads."""
        import torch

        from triton_client_amd.ops import hip

        if not torch.cuda.is_available():
            raise ServerError(error or "%s (GPU) requires a GPU" % self.name)
        hip.lib()  # fail loudly if the native kernels are missing
        self.torch = torch
        return torch, hip, torch.device("cuda", self.device_id)

    def _pinned(self, slot, key, nbytes):
        """Pinned host memory under ``slot[key]``, freed by ``unload``."""
        from triton_client_amd.ops import hip

        slot[key] = hip.host_alloc(nbytes)
        slot.setdefault("pinned", []).append(slot[key])
        return slot[key]

    def unload(self):
        from triton_client_amd.ops import hip

        def free(slot):
            for ptr in slot.pop("pinned", ()):
                hip.host_free(ptr)

        self._slots.close(free)

    def _load_twin(self, host_cls, device_path):
        """Build and load the CPU twin; ``device_path`` is the model's knob, as
        read by the caller.  Returns it: False means the twin does the work."""
        self._host = host_cls(self.version)
        self._host.load()
        self.device_path = device_path
        return device_path

    def _add_stage_slots(self, dev, in_bytes, out_bytes, **extra):
        """One slot per instance: a stream, pinned and device staging of
        ``in_bytes`` and ``out_bytes``, and a device buffer per ``extra`` name."""
        torch = self.torch
        for _ in range(max(1, self.instance_count)):
            slot = {"stream": torch.cuda.Stream(device=dev)}
            self._pinned(slot, "in_host", in_bytes)
            self._pinned(slot, "out_host", out_bytes)
            for key, nbytes in dict(in_dev=in_bytes, out_dev=out_bytes, **extra).items():
                slot[key] = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
            self._slots.add(slot)

    def _per_request(self, requests, one, wrapped=()):
        """``one(r)`` per request; a ServerError is that request's result, and so
        is a HipError or one of ``wrapped`` under the model's name."""
        from triton_client_amd.ops import hip

        out = []
        for r in requests:
            try:
                out.append(one(r))
            except ServerError as e:
                out.append(e)
            except (hip.HipError,) + wrapped as e:
                out.append(ServerError("%s: %s" % (self.name, e)))
        return out


class Ensemble(Model):
    """A model the server runs step by step (``ensemble_steps``)."""

    platform = "ensemble"
    backend = ""

    def load(self):
        pass

    def execute(self, requests):  # pragma: no cover - the server runs ensembles step by step
        raise ServerError("ensemble models are scheduled by the server")


def plan_errors(plan, name, e):
    """A batch that failed with ``e``: every request gets it (a HipError under
    the model's name), except those whose plan entry is already their error."""
    err = e if isinstance(e, ServerError) else ServerError("%s: %s" % (name, e))
    return [p if isinstance(p, Exception) else err for p in plan]


def pinned_view(ptr, dtype, count):
    """``count`` items of ``dtype`` at the host address ``ptr`` as a numpy array
    that aliases the memory."""
    dt = np.dtype(dtype)
    return np.frombuffer((ctypes.c_uint8 * (count * dt.itemsize)).from_address(ptr), dtype=dt)


def place_input(slot, tensor, name, dtype, nbytes, host_off):
    """Where the kernel reads an input of ``nbytes``, and whether that is the
    slot's staging area: a ``DeviceView`` is checked for size and read in place,
    host data is written into the pinned stage at ``host_off`` and has yet to go
    up to the same offset of ``in_dev``."""
    data = tensor.data
    if isinstance(data, DeviceView):
        if data.nbytes < nbytes:
            raise ServerError("input region too small for %s" % name)
        return data.ptr, False
    dt = np.dtype(dtype)
    pinned_view(slot["in_host"] + host_off, dt, nbytes // dt.itemsize)[:] = np.asarray(data, dtype=dt).reshape(-1)
    return slot["in_dev"].data_ptr() + host_off, True


def stage_input(hip, slot, tensor, name, dtype, nbytes, host_off, stream):
    """``place_input``, and the upload of what it staged.  Returns the device pointer."""
    ptr, staged = place_input(slot, tensor, name, dtype, nbytes, host_off)
    if staged:
        hip.memcpy_async(ptr, slot["in_host"] + host_off, nbytes, stream)
    return ptr


def stage_texts(slot, table, pairs, head_bytes):
    """Copy each row's (question, context) end to end into the pinned stage
    behind its first ``head_bytes`` and fill ``table[row]`` with ``{off, len,
    off, len}``.  Returns the bytes of text."""
    at = 0
    base = slot["in_host"] + head_bytes
    for r, pair in enumerate(pairs):
        for f, s in enumerate(pair):
            table[r, 2 * f], table[r, 2 * f + 1] = at, len(s)
            ctypes.memmove(base + at, s, len(s))
            at += len(s)
    return at


def download(hip, slot, nbytes, stream):
    """The first ``nbytes`` of the slot's device outputs, once the stream is
    through: a uint8 array of the caller's own."""
    hip.memcpy_async(slot["out_host"], slot["out_dev"].data_ptr(), nbytes, stream)
    hip.stream_synchronize(stream)
    return pinned_view(slot["out_host"], np.uint8, nbytes).copy()
