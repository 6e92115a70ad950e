"""oadg_amd/staging.py: the pinned staging ring, upload() and readback().

Every GPU test first queues a few milliseconds of real work on the stream (eight 8192 x 8192 bf16 matmuls), so the copies
sit queued while the host runs ahead: a missing wait then shows as a stale table every time, not as a rare race."""
import threading

import numpy as np
import pytest
import torch

from oadg_amd import staging


@pytest.fixture(scope='module')
def busy(dev):
    a = torch.ones((8192, 8192), dtype=torch.bfloat16, device=dev)
    out = torch.empty_like(a)
    torch.mm(a, a, out=out)                   # (the BLAS library's start-up is not part of any test)
    torch.cuda.synchronize(dev)

    def queue(n=8):
        for _ in range(n):
            torch.mm(a, a, out=out)
    return queue


def _tables(n, nbytes=64):
    return [np.full(nbytes, i, np.uint8) for i in range(n)]


def _check(tensors, tables):
    for t, a in zip(tensors, tables):
        assert t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), a)


@pytest.mark.gpu
def test_slot_reuse_waits(dev, busy):
    ring = staging.Ring(2, 64)
    tabs = _tables(6)
    busy()
    got = [ring.upload(a, dev) for a in tabs]
    torch.cuda.synchronize(dev)
    _check(got, tabs)
    assert len(ring) == 2


@pytest.mark.gpu
def test_growth_in_place_of_waiting(dev, busy):
    ring = staging.Ring(2, 64, grow_when_busy=True)
    tabs = _tables(6)
    busy()
    got = [ring.upload(a, dev) for a in tabs]
    torch.cuda.synchronize(dev)
    _check(got, tabs)
    grown = len(ring)
    assert grown > 2
    more = [ring.upload(a, dev) for a in tabs]
    torch.cuda.synchronize(dev)
    _check(more, tabs)
    assert len(ring) == grown


@pytest.mark.gpu
def test_reserve_now_fill_later(dev, busy):
    ring = staging.Ring(3, 64)
    tabs = _tables(3)
    busy()
    a = ring.reserve(64)
    got = [ring.upload(t, dev) for t in tabs[1:]]
    got += [ring.upload(t, dev) for t in tabs[1:]]          # (a second lap: the reserved slot is stepped over)
    th = threading.Thread(target=lambda: a.host.numpy().__setitem__(slice(0, 64), tabs[0]))
    th.start()
    th.join()
    first = a.commit(64, dev)
    torch.cuda.synchronize(dev)
    _check([first] + got, [tabs[0]] + tabs[1:] + tabs[1:])
    assert len(ring) == 3

    ring = staging.Ring(2, 64)
    a, b = ring.reserve(64), ring.reserve(64)
    assert a is not b
    with pytest.raises(RuntimeError):
        ring.reserve(64)
    b.release()
    assert ring.reserve(64) is b


@pytest.mark.gpu
def test_packed_upload(dev, busy):
    rs = np.random.RandomState(0)
    f = rs.rand(3, 5).astype(np.float32)
    i = rs.randint(-2 ** 40, 2 ** 40, size=7).astype(np.int64)
    tab = np.zeros(3, dtype=np.dtype([('p', np.uint64), ('n', np.int32), ('x', np.float32)]))
    tab['p'], tab['n'], tab['x'] = [2 ** 63, 5, 7], [-1, 2, 3], [0.5, -1.5, 2.5]
    e = np.zeros(0, np.int32)
    ring = staging.Ring(2, 64)
    busy()
    df, di, dt, de = ring.upload([f, i, tab, e], dev)
    torch.cuda.synchronize(dev)
    assert len(ring) == 1
    assert (df.dtype, tuple(df.shape)) == (torch.float32, (3, 5)) and np.array_equal(df.cpu().numpy(), f)
    assert (di.dtype, tuple(di.shape)) == (torch.int64, (7,)) and np.array_equal(di.cpu().numpy(), i)
    assert (dt.dtype, tuple(dt.shape)) == (torch.uint8, (tab.nbytes,))
    assert np.array_equal(dt.cpu().numpy().view(tab.dtype), tab)
    assert (de.dtype, tuple(de.shape)) == (torch.int32, (0,)) and de.device == df.device
    ptrs = [df.data_ptr(), di.data_ptr(), dt.data_ptr()]
    assert all(p % 256 == 0 for p in ptrs) and ptrs == sorted(ptrs) and ptrs[2] - ptrs[0] == 512      # one slot, one copy
    # a single array comes back as a tensor, a CPU tensor is taken like an array, nothing to copy takes no slot
    one = ring.upload(torch.from_numpy(i), dev)
    none = ring.upload(e, dev)
    torch.cuda.synchronize(dev)
    assert np.array_equal(one.cpu().numpy(), i) and none.numel() == 0 and none.is_cuda and len(ring) == 2


@pytest.mark.gpu
def test_thread_local_default_ring(dev, busy):
    n, got, rings, errors = 200, [None, None], [None, None], []

    def tables(tid):
        return [np.full(1024, tid * 1000 + i, np.int32) for i in range(n)]

    def worker(tid):
        try:
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                busy()
                got[tid] = [staging.upload(a, dev) for a in tables(tid)]
            rings[tid] = staging.local_ring(dev, 4096)
            stream.synchronize()
        except BaseException as exc:                # noqa: B902 (reported by the assertion below)
            errors.append(exc)

    threads = [threading.Thread(target=worker, args=(tid,)) for tid in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert rings[0] is not rings[1] and staging.local_ring(dev, 4096) not in rings
    for tid in range(2):
        assert got[tid][0].dtype == torch.int32
        assert np.array_equal(torch.stack(got[tid]).cpu().numpy(), np.stack(tables(tid)))


@pytest.mark.gpu
def test_readback(dev, busy):
    t = torch.arange(1000, device=dev)
    busy()
    h = staging.readback(t)
    assert not h.done()
    host = h.wait()
    assert h.done() and host.is_pinned() and torch.equal(host, t.cpu())
    c = torch.arange(5)
    hc = staging.readback(c)
    assert hc.wait() is c and hc.done() and hc.event is None


def test_cpu_upload_passes_through():
    cpu = torch.device('cpu')
    a = np.arange(5)
    out = staging.upload(a, cpu)
    assert out.device == cpu and out.dtype == torch.int64 and np.array_equal(out.numpy(), a)
    assert not out.is_pinned() and len(staging.local_ring(cpu, a.nbytes)) == 0
