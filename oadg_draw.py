"""Drawing and writing pictures on the device: the ctypes calls of ``oadg_draw_items_u8`` (csrc/draw.hip) and of the PNG
encoder (csrc/png_encode.hip), with the validation, upload and bookkeeping around them.  ``oadg_amd.visualization`` imports
this module lazily, so ``BaseDetector.show_result`` and ``single_gpu_test(show_dir=...)`` need nothing but the package, the
library and a GPU; tools/analysis_tools/get_corrupted_dataset.py takes ``PngEncoder`` and ``write_png`` from here.

WHERE THIS BELONGS: ``draw_items`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py, ``PngEncoder`` next to it.
They are here, next to the package's import shim (as oadg_voc_tpfp.py is), for one reason: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and the
change that added the rasteriser could add test files but not edit that one.  The suites that answer for these call sites
are tests/test_hip_draw.py (the rasteriser) and tests/test_png_encode.py (the encoder).  The follow-up is mechanical: add
'oadg_draw_items_u8', 'oadg_png_encode_rgb8' and 'oadg_png_write_rgb8' to that test's OWN_SUITES and
'oadg_draw_tile_capacity', 'oadg_png_encode_stream_capacity' and 'oadg_png_encode_workspace_bytes' to its
LAUNCHES_NOTHING, move the contents of this file into hip_ops.py, and delete it.
"""
import numpy as np
import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import DRAW_ITEM_INTS, DRAW_TEXT, check, ptr, require_cuda, stream_ptr

BATCH = 8                    # images per encode (8 x 1024 x 2048 x 3 bytes in, at most 8 x 6.4 MB of pinned memory out)
PINNED_SLOTS = 3             # one being filled by the device, one being written, one spare


def tile_capacity():
    """rows a workgroup of csrc/draw.hip lists for its tile before it paints and starts over (a test straddles it)"""
    return int(_lib.lib().oadg_draw_tile_capacity())


def _host_i32(a, what, shape_tail=None):
    if isinstance(a, torch.Tensor):
        if a.is_cuda:
            raise ValueError(f'{what} is validated on the host before upload: pass a CPU tensor or a numpy array')
        if a.dtype != torch.int32 or not a.is_contiguous():
            raise ValueError(f'{what} must be a contiguous int32 array')
        a = a.numpy()
    if not isinstance(a, np.ndarray) or a.dtype != np.int32 or not a.flags.c_contiguous:
        raise ValueError(f'{what} must be a contiguous int32 array')
    if shape_tail is not None and (a.ndim != 2 or a.shape[1] != shape_tail):
        raise ValueError(f'{what} must be [n_items, {shape_tail}]')
    return a


def check_display_list(n, items, item_off, text):
    """the host half of ``draw_items``: ValueError naming the argument, or (items, item_off, text) as numpy arrays"""
    items = _host_i32(items, 'items', DRAW_ITEM_INTS)
    item_off = _host_i32(item_off, 'item_off')
    if isinstance(text, (bytes, bytearray)):
        text = np.frombuffer(bytes(text), dtype=np.uint8)
    if isinstance(text, torch.Tensor) and not text.is_cuda and text.dtype == torch.uint8 and text.is_contiguous():
        text = text.numpy()
    if not isinstance(text, np.ndarray) or text.dtype != np.uint8 or text.ndim != 1 or not text.flags.c_contiguous:
        raise ValueError('text must be bytes or a contiguous 1-D uint8 array')
    n_items = items.shape[0]
    if item_off.ndim != 1 or item_off.shape[0] != n + 1:
        raise ValueError(f'item_off must hold n + 1 = {n + 1} entries')
    if item_off[0] != 0 or item_off[-1] != n_items or (np.diff(item_off) < 0).any():
        raise ValueError(f'item_off must start at 0, never decrease and end at n_items = {n_items}')
    runs = items[items[:, 0] == DRAW_TEXT]
    off, length = runs[:, 3].astype(np.int64), runs[:, 4].astype(np.int64)
    if ((off < 0) | (length < 0) | (off + length > text.shape[0])).any():
        raise ValueError(f'text: a run of items lies outside the {text.shape[0]} bytes of the buffer')
    return items, item_off, text


def draw_items(imgs, items, item_off, text=b''):
    """csrc/draw.hip on torch's current stream: paint the display list in place on the resident uint8 batch ``imgs``
    [n, H, W, 3] and return it.  ``items`` int32 [n_items, 8] rows (include/oadg_hip.h: OUTLINE, FILL, TEXT), ``item_off``
    int32 [n + 1] (image i owns rows item_off[i] .. item_off[i + 1] - 1), ``text`` the bytes the TEXT rows point into - all
    three on the host: they are checked there and uploaded through the staging path.  Painter's order, clipped to the image,
    any int32 coordinate."""
    if not isinstance(imgs, torch.Tensor) or not imgs.is_cuda:
        raise ValueError('imgs must be a resident tensor: the rasteriser runs on the MI355X only, there is no CPU fallback')
    require_cuda(imgs)
    if imgs.dtype != torch.uint8 or not imgs.is_contiguous():
        raise ValueError('imgs must be a contiguous uint8 tensor')
    if imgs.dim() != 4 or imgs.shape[3] != 3 or imgs.shape[1] < 1 or imgs.shape[2] < 1:
        raise ValueError('imgs must be [n, H, W, 3]')
    n, H, W, _ = imgs.shape
    items, item_off, text = check_display_list(n, items, item_off, text)
    if n == 0 or items.shape[0] == 0:
        return imgs
    with torch.cuda.device(imgs.device):
        d_items, d_off, d_text = staging.upload([items.reshape(-1), item_off, text if text.shape[0] else np.zeros(1, np.uint8)],
                                                imgs.device)
        check(_lib.lib().oadg_draw_items_u8(ptr(imgs), n, H, W, ptr(d_items), ptr(d_off), items.shape[0], ptr(d_text),
                                            text.shape[0], stream_ptr()), 'oadg_draw_items_u8')
    return imgs


# ------------------------------------------------------------------------------------------------------ PNG output
class PngEncoder:
    """csrc/png_encode.hip on resident uint8 [n, H, W, 3] batches: ``launch`` enqueues the encode and the copy of the
    streams into a pinned slot on the current stream, ``finish`` waits for that copy and returns per image (address, bytes)
    of its stream in the slot.  A slot is handed out again only after ``release`` (its files are written)."""

    def __init__(self, device, slots=PINNED_SLOTS, filter_mode=-1):
        self.L, self.device = _lib.lib(), torch.device(device)
        self.filter_mode, self.device_ms, self.images = filter_mode, 0.0, 0
        self._slots = [dict(host=None, sizes=None, busy=[]) for _ in range(slots)]
        self._next = 0

    def launch(self, imgs, bgr=True):
        L = self.L
        n, H, W, _ = imgs.shape
        cap = int(L.oadg_png_encode_stream_capacity(H, W))
        ws_bytes = int(L.oadg_png_encode_workspace_bytes(n, H, W))
        if cap == 0 or ws_bytes == 0:
            raise ValueError(f'a batch of {n} images of {H} x {W}: (3W + 1) * H must stay below 2^31')
        slot = self._slots[self._next]
        self._next = (self._next + 1) % len(self._slots)
        for f in slot['busy']:                                     # the writes that still read this slot
            f.result()
        slot['busy'] = []
        if slot['host'] is None or slot['host'].numel() < n * cap:
            slot['host'] = torch.empty((n * cap,), dtype=torch.uint8, pin_memory=True)
        if slot['sizes'] is None or slot['sizes'].numel() < n:
            slot['sizes'] = torch.empty((max(n, BATCH),), dtype=torch.int64, pin_memory=True)
        imgs = imgs.contiguous()
        streams = torch.empty((n * cap,), dtype=torch.uint8, device=self.device)
        sizes = torch.empty((n,), dtype=torch.int64, device=self.device)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=self.device)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        check(L.oadg_png_encode_rgb8(ptr(imgs), n, H, W, int(bool(bgr)), self.filter_mode, ptr(streams), cap, ptr(sizes),
                                     ptr(ws), ws_bytes, stream_ptr()), 'oadg_png_encode_rgb8')
        t1.record()
        slot['host'][:n * cap].copy_(streams, non_blocking=True)
        slot['sizes'][:n].copy_(sizes, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        return dict(slot=slot, n=n, H=H, W=W, cap=cap, t0=t0, t1=t1, done=done, keep=(imgs, streams, sizes, ws))

    def finish(self, job):
        """-> [(host address, bytes)] per image, valid until the slot's release()"""
        job['done'].synchronize()
        self.device_ms += job['t0'].elapsed_time(job['t1'])
        self.images += job['n']
        job['keep'] = None
        sizes = job['slot']['sizes'][:job['n']].tolist()
        if max(sizes) > job['cap']:
            raise RuntimeError(f'oadg_png_encode_rgb8 needs {max(sizes)} bytes, above its own bound {job["cap"]}')
        base = job['slot']['host'].data_ptr()
        return [(base + i * job['cap'], int(b)) for i, b in enumerate(sizes)]

    @staticmethod
    def release(job, futures):
        """the slot of ``job`` is reused once ``futures`` (the writes that read it) are done"""
        job['slot']['busy'] = list(futures)


def write_png(L, path, address, nbytes, H, W):
    rc = L.oadg_png_write_rgb8(path.encode(), address, nbytes, H, W)
    if rc == -3:
        raise OSError(f'{path}: cannot be written')
    if rc != 0:
        raise RuntimeError(f'{path}: oadg_png_write_rgb8 failed with {rc}')
    return nbytes
