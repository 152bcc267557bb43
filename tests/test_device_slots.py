"""The host-side plumbing the GPU models share (server/device_slots.py): the
slot pool, pinned views, input and text staging, the ensemble base.  No GPU:
the pinned memory is a ctypes buffer and ``hip`` a recorder."""

import ctypes
import threading

import numpy as np
import pytest

from triton_client_amd.server.device_slots import (Ensemble, SlotPool, pinned_view, place_input, plan_errors,
                                                   stage_input, stage_texts)
from triton_client_amd.server.types import DeviceView, ServerError

WAIT = 5.0  # seconds a thread may take before the test calls it stuck


def pool_of(n):
    pool = SlotPool()
    for k in range(n):
        pool.add({"id": k})
    return pool


def test_pool_is_a_sequence_of_its_slots():
    pool = pool_of(3)
    assert len(pool) == 3
    assert [pool[i]["id"] for i in range(3)] == [0, 1, 2]
    assert [s["id"] for s in pool] == [0, 1, 2]


def test_third_thread_blocks_until_a_release():
    pool = pool_of(2)
    got, entered, leave, third_in = [], [threading.Event(), threading.Event()], threading.Event(), threading.Event()
    waiting = threading.Event()

    class Watched(threading.Condition):
        def wait(self, timeout=None):
            waiting.set()
            return super().wait(timeout)

    pool._cv = Watched()

    def holder(k):
        with pool.slot() as (i, slot):
            got.append(i if slot is pool[i] else -1)
            entered[k].set()
            leave.wait(WAIT)

    def third():
        with pool.slot() as (i, _):
            got.append(i)
            third_in.set()

    threads = [threading.Thread(target=holder, args=(k,)) for k in range(2)] + [threading.Thread(target=third)]
    for t in threads[:2]:
        t.start()
    assert entered[0].wait(WAIT) and entered[1].wait(WAIT)
    assert sorted(got) == [0, 1]  # both slots handed out once before any release
    threads[2].start()
    assert waiting.wait(WAIT)  # no slot is free: the third thread waits on the pool's condition
    assert not third_in.is_set() and len(got) == 2
    leave.set()
    assert third_in.wait(WAIT)
    for t in threads:
        t.join(WAIT)
        assert not t.is_alive()
    assert len(got) == 3 and got[2] in (0, 1)
    assert sorted(pool.acquire() for _ in range(2)) == [0, 1]  # every slot came back


def test_slot_is_released_when_the_body_raises():
    pool = pool_of(1)
    with pytest.raises(KeyError):
        with pool.slot():
            raise KeyError("boom")
    i = pool.acquire()  # would block for ever had the slot leaked
    assert i == 0
    pool.release(i)


def test_close_frees_every_slot_once_and_survives_a_free_that_raises():
    pool = pool_of(3)
    seen = []

    def free(slot):
        seen.append(slot["id"])
        if slot["id"] == 1:
            raise RuntimeError("does not free")

    pool.close(free)
    assert seen == [0, 1, 2]
    assert len(pool) == 0
    pool.close(free)
    assert seen == [0, 1, 2]


@pytest.mark.parametrize("dtype,ctype", [(np.int32, ctypes.c_int32), (np.uint32, ctypes.c_uint32),
                                         (np.float32, ctypes.c_float), (np.uint8, ctypes.c_uint8)])
def test_pinned_view_aliases_the_buffer(dtype, ctype):
    buf = (ctype * 7)()
    v = pinned_view(ctypes.addressof(buf) + ctypes.sizeof(ctype), dtype, 5)
    assert v.dtype == np.dtype(dtype) and v.shape == (5,)
    v[:] = np.arange(1, 6)
    assert list(buf) == [0, 1, 2, 3, 4, 5, 0]
    buf[2] = 9
    assert v[1] == 9


class FakeTensor:
    def __init__(self, data):
        self.data = data


class FakeDev:
    """The ``in_dev`` of a slot: only its address matters."""

    def data_ptr(self):
        return 0x7000


class FakeHip:
    def __init__(self):
        self.copies = []

    def memcpy_async(self, dst, src, nbytes, stream):
        self.copies.append((dst, src, nbytes, stream))


def stage_slot(nbytes):
    buf = (ctypes.c_uint8 * nbytes)()
    return {"in_host": ctypes.addressof(buf), "in_dev": FakeDev()}, buf


def test_stage_texts_lays_rows_end_to_end_behind_the_head():
    slot, buf = stage_slot(64)
    table = np.full((4, 4), 99, dtype=np.uint32)
    used = stage_texts(slot, table, [(b"", b"abc"), (b"de", b"")], 16)
    assert used == 5
    assert table[:2].tolist() == [[0, 0, 0, 3], [3, 2, 5, 0]]
    assert table[2:].tolist() == [[99] * 4] * 2
    assert bytes(buf[16:21]) == b"abcde"
    assert not any(buf[:16]) and not any(buf[21:])


def test_stage_input_reads_a_device_view_in_place():
    slot, buf = stage_slot(32)
    hip = FakeHip()
    assert stage_input(hip, slot, FakeTensor(DeviceView(0x1234, 16, 0)), "x", np.int32, 16, 8, 5) == 0x1234
    assert hip.copies == [] and not any(buf)


def test_stage_input_refuses_a_device_view_one_byte_short():
    slot, _ = stage_slot(32)
    hip = FakeHip()
    with pytest.raises(ServerError) as e:
        stage_input(hip, slot, FakeTensor(DeviceView(0x1234, 15, 0)), "start_logits", np.int32, 16, 8, 5)
    assert str(e.value) == "input region too small for start_logits"
    assert hip.copies == []


def test_stage_input_writes_host_data_at_the_offset_and_uploads_it_once():
    slot, buf = stage_slot(32)
    hip = FakeHip()
    data = np.array([[1.5, -2.0], [3.25, 4.0]], dtype=np.float64)  # converted to the stage's dtype
    ptr = stage_input(hip, slot, FakeTensor(data), "x", np.float32, 16, 8, 5)
    assert ptr == 0x7000 + 8
    assert hip.copies == [(0x7000 + 8, slot["in_host"] + 8, 16, 5)]
    assert np.frombuffer(bytes(buf[8:24]), dtype=np.float32).tolist() == [1.5, -2.0, 3.25, 4.0]
    assert not any(buf[:8]) and not any(buf[24:])


def test_place_input_leaves_the_upload_to_the_caller():
    slot, buf = stage_slot(32)
    assert place_input(slot, FakeTensor(np.arange(4, dtype=np.int32)), "x", np.int32, 16, 16) == (0x7000 + 16, True)
    assert np.frombuffer(bytes(buf[16:]), dtype=np.int32).tolist() == [0, 1, 2, 3]
    assert place_input(slot, FakeTensor(DeviceView(0x99, 16, 0)), "x", np.int32, 16, 0) == (0x99, False)


def test_plan_errors_keeps_a_request_its_own_error():
    own, batch = ServerError("mine"), ServerError("the batch's")
    assert plan_errors([own, (0, 1)], "m", batch) == [own, batch]
    wrapped = plan_errors([(0, 1)], "m", RuntimeError("hipErrorX"))
    assert isinstance(wrapped[0], ServerError) and str(wrapped[0]) == "m: hipErrorX"


def test_ensemble_is_not_executed():
    class Two(Ensemble):
        name = "two"

    m = Two()
    assert (m.platform, m.backend) == ("ensemble", "")
    m.load()
    with pytest.raises(ServerError) as e:
        m.execute([])
    assert str(e.value) == "ensemble models are scheduled by the server"
