"""Pinned host memory for every small host <-> device hand-off of the package: descriptor tables, draws and filter
weights on their way to a kernel, counts and scores on their way back.

THE INVARIANT: a slot's pinned bytes are not rewritten until the event recorded behind the last copy out of them has
completed, and that event is recorded on the stream that carries the copy, immediately after the copy.  ``Slot.commit``
records the event, ``Ring.reserve`` is the one place that waits for it (or steps around it); a caller writes into
``slot.host`` between the two and nowhere else, so the host may run ahead of the device as far as the ring has slots
without corrupting a table a queued copy has not read yet.

A ring owns host memory only.  The device side of an upload is an ordinary tensor of torch's caching allocator: the
kernel that reads it is launched on the same current stream, so dropping the tensor after the launch call leaves the
reuse of its memory stream-ordered.

(device_rng.py pins its own two state buffers: a one-in-flight protocol with its own assertion, not a ring.)
"""
import threading

import numpy as np
import torch


class Slot:
    """one pinned buffer of a ring: ``host`` is its uint8 view, rewritable from reserve() until commit()"""
    __slots__ = ('host', '_event', '_event_dev', '_reserved')

    def __init__(self):
        self.host, self._event, self._event_dev, self._reserved = None, None, None, False

    def commit(self, n, device):
        """enqueue ``host[:n]`` -> a new uint8 tensor on ``device`` on the current stream, the slot's event right behind it
        (a device that is not a GPU: a copy now, no event)"""
        device = torch.device(device)
        if device.type != 'cuda':
            dst = self.host[:n].clone()
        else:
            stream = torch.cuda.current_stream(device)
            dst = torch.empty((n,), dtype=torch.uint8, device=device)
            dst.copy_(self.host[:n], non_blocking=True)
            if self._event is None or self._event_dev != stream.device:
                self._event, self._event_dev = torch.cuda.Event(), stream.device
            self._event.record(stream)
        self._reserved = False
        return dst

    def release(self):
        """give a reserved slot back without a copy (nothing turned out to be uploaded)"""
        self._reserved = False


class Ring:
    """``slots`` pinned buffers of at least ``min_bytes``, created as they are first needed and handed out in turn.
    When the copy last committed from the next slot has not completed, reserve() waits for it - or, with
    ``grow_when_busy``, inserts a new slot at that position and hands that out.  ``slots`` may be raised later: it holds
    for the slots not yet created.  reserve() may be called from several threads; a slot belongs to the thread that
    reserved it until it is committed (from whichever thread)."""

    def __init__(self, slots, min_bytes, grow_when_busy=False):
        self.slots, self.min_bytes, self.grow_when_busy = int(slots), int(min_bytes), grow_when_busy
        self._slots, self._next, self._lock = [], 0, threading.Lock()

    def __len__(self):
        return len(self._slots)

    def reserve(self, nbytes):
        """a slot whose ``host`` holds at least ``nbytes``; it is not handed out again before its commit() / release()"""
        with self._lock:
            if len(self._slots) < self.slots:
                slot = Slot()
                self._slots.append(slot)
            else:
                for _ in range(len(self._slots)):
                    k, self._next = self._next, (self._next + 1) % len(self._slots)
                    slot = self._slots[k]
                    if not slot._reserved:
                        break
                else:
                    raise RuntimeError(f'all {len(self._slots)} staging slots are reserved and not committed')
                if self.grow_when_busy and slot._event is not None and not slot._event.query():
                    # the copy issued from this slot one lap ago is still queued (behind the backward kernels of THIS pass):
                    # take a new slot instead of stalling the host's run-ahead on it
                    slot = Slot()
                    self._slots.insert(k, slot)
                    self._next = (k + 1) % len(self._slots)
            slot._reserved = True
        if slot._event is not None:
            slot._event.synchronize()           # THE wait of the invariant (outside the lock: other slots stay available)
        if slot.host is None or slot.host.numel() < nbytes:
            # (pinning allocates, ~2 ms for a 4096-box descriptor table: once per slot, then again only for a larger table)
            cap = self.min_bytes if nbytes <= self.min_bytes else 1 << (int(nbytes) - 1).bit_length()
            slot.host = torch.empty((cap,), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        return slot

    def upload(self, arrays, device):
        """one host array (numpy, or a CPU tensor) or a sequence of them -> device tensor(s) of the same dtype and shape
        (a table of a structured dtype: its bytes), through ONE slot and one copy: the arrays are packed at 256-byte
        aligned offsets.  Never blocks the host on the stream.  Nothing to copy: no slot; not a GPU: a plain ``.to``."""
        single = not isinstance(arrays, (list, tuple))
        arrs = [a.numpy() if torch.is_tensor(a) else np.ascontiguousarray(a) for a in ([arrays] if single else arrays)]
        device = torch.device(device)
        offs, total = [], 0
        for a in arrs:
            offs.append((total + 255) // 256 * 256)
            total = offs[-1] + a.nbytes
        if device.type != 'cuda' or total == 0:
            out = [_typed(torch.from_numpy(_bytes(a)).to(device), a) for a in arrs]
        else:
            slot = self.reserve(total)
            host = slot.host.numpy()
            for a, o in zip(arrs, offs):
                host[o:o + a.nbytes] = _bytes(a)
            dev = slot.commit(total, device)
            out = [_typed(dev[o:o + a.nbytes], a) for a, o in zip(arrs, offs)]
        return out[0] if single else out


def _bytes(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _typed(raw, like):
    """the uint8 tensor ``raw`` as a tensor of the dtype and shape of the array ``like``"""
    if like.dtype.fields is not None:
        return raw
    return raw.view(torch.from_numpy(np.empty(0, like.dtype)).dtype).view(like.shape)


_TLS = threading.local()
_SMALL = 1 << 20


def local_ring(device, nbytes):
    """the calling thread's own ring for uploads of ``nbytes`` to ``device``: thread-local and per device by construction,
    so worker threads (each on its own stream) and the pipeline thread never share slots.  96 slots from 4 KiB for the
    tables of up to 1 MiB (OA-Mix queues hundreds of them per batch before the device has read the first); 2 slots for
    anything larger (a batch of draws or pixels for a corruption: 96 of THOSE would pin gigabytes)."""
    rings = _TLS.__dict__.setdefault('rings', {})
    key = (torch.device(device), nbytes <= _SMALL)
    ring = rings.get(key)
    if ring is None:
        ring = rings[key] = Ring(96, 4096) if key[1] else Ring(2, _SMALL)
    return ring


def upload(arrays, device):
    """Ring.upload through the calling thread's ring for ``device``"""
    nbytes = sum(a.nbytes for a in arrays) if isinstance(arrays, (list, tuple)) else arrays.nbytes
    return local_ring(device, nbytes).upload(arrays, device)


class Readback:
    """a device -> host copy in flight: ``host`` is its pinned destination, valid once wait() has returned; ``event`` the
    event recorded behind the copy (None: nothing was copied)"""
    __slots__ = ('host', 'event')

    def __init__(self, host, event):
        self.host, self.event = host, event

    def done(self):
        return self.event is None or self.event.query()

    def wait(self):
        """blocks until THIS copy has landed (its own event: later work on the stream is not waited for) -> ``host``"""
        if self.event is not None:
            self.event.synchronize()
        return self.host


def readback(t):
    """enqueue the copy of the device tensor ``t`` to pinned memory on the current stream, an event right behind it -> its
    Readback.  A CPU tensor passes straight through: no copy, no event."""
    if not t.is_cuda:
        return Readback(t, None)
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    event = torch.cuda.Event()
    event.record(torch.cuda.current_stream(t.device))
    return Readback(host, event)
