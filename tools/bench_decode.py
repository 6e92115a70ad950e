"""JPEG decoding for the S-DGOD input path: PIL (what ``CocoDataset.decode_into`` does for a JPEG: Image.open -> convert
-> channel flip -> copy) against csrc/jpeg_decode.hip (host entropy stage + device pixel stage).  Prints one JSON line.

usage: python tools/bench_decode.py [--n 8] [--batch 4] [--reps 3] [--quality 95] [--workers 12]

Per size (720x1280 = a DWD frame, 1024x2048 = a Cityscapes frame), over --n generated JPEGs (4:2:0, lowpass noise):
  host_ms_per_image.{pil,native_entropy}.{one_thread,pool}: wall time per image on one thread and on a pool of
      --workers threads (the dataset's decode pool); 'native_entropy' is oadg_jpeg_entropy_decode alone
  host_twin_ms_per_image: oadg_jpeg_decode_bgr (the host twin of both stages, one thread)
  device_us_per_batch: the pixel stage (two launches) on a batch of --batch images, HIP events, median of 20
  device_bytes_per_batch / device_gbps: coefficients read + component planes written and read + BGR written
  byte_equal: the device batch equals PIL's decode
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))


def make_files(d, n, H, W, quality):
    from PIL import Image
    from inputs import lowpass_image
    paths = []
    for i in range(n):
        rs = np.random.RandomState(i)
        a = np.clip(lowpass_image(rs, H, W, 8).astype(np.int32) + rs.randint(-8, 9, (H, W, 3)), 0, 255).astype(np.uint8)
        p = os.path.join(d, f'{H}x{W}_{i}.jpg')
        Image.fromarray(a).save(p, quality=quality)
        paths.append(p)
    return paths


def pil_into(path, dst):
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert('RGB'))
    np.copyto(dst, np.ascontiguousarray(rgb[:, :, ::-1]))


def timed(fn, items, workers, reps):
    work = items * reps
    t = time.perf_counter()
    if workers == 1:
        for it in work:
            fn(it)
    else:
        with ThreadPoolExecutor(workers) as pool:
            list(pool.map(fn, work))
    return (time.perf_counter() - t) / len(work) * 1e3


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=8)
    p.add_argument('--batch', type=int, default=4)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--quality', type=int, default=95)
    p.add_argument('--workers', type=int, default=12)
    a = p.parse_args()
    import torch
    from oadg_amd import _lib, hip_ops
    L = _lib.lib()
    D = hip_ops.JPEG_DESC_BYTES
    res = dict(quality=a.quality, subsampling='4:2:0', workers=a.workers, sizes={})
    with tempfile.TemporaryDirectory() as tmp:
        for H, W in ((720, 1280), (1024, 2048)):
            paths = make_files(tmp, a.n, H, W, a.quality)
            slot = int(L.oadg_jpeg_coef_capacity(H, W))
            bufs = {}

            def native(path):
                import threading
                k = threading.get_ident()
                if k not in bufs:
                    bufs[k] = (np.empty(slot, np.int16), np.empty(D, np.uint8))
                c, d = bufs[k]
                assert L.oadg_jpeg_entropy_decode(path.encode(), H, W, c.ctypes.data, slot, d.ctypes.data) == 0

            dst = {}

            def pil(path):
                import threading
                k = threading.get_ident()
                if k not in dst:
                    dst[k] = np.empty((H, W, 3), np.uint8)
                pil_into(path, dst[k])

            out1 = np.empty((H, W, 3), np.uint8)
            r = dict(mb_per_file=round(sum(os.path.getsize(q) for q in paths) / len(paths) / 1e6, 3),
                     host_ms_per_image=dict(
                         pil=dict(one_thread=timed(pil, paths, 1, a.reps), pool=timed(pil, paths, a.workers, a.reps)),
                         native_entropy=dict(one_thread=timed(native, paths, 1, a.reps),
                                             pool=timed(native, paths, a.workers, a.reps))),
                     host_twin_ms_per_image=timed(
                         lambda q: L.oadg_jpeg_decode_bgr(q.encode(), out1.ctypes.data, H, W), paths, 1, 1))
            if torch.cuda.is_available():
                n = min(a.batch, len(paths))
                host = torch.zeros(n * D + 2 * n * slot, dtype=torch.uint8).pin_memory()
                base = host.numpy().ctypes.data
                for i in range(n):
                    assert L.oadg_jpeg_entropy_decode(paths[i].encode(), H, W, base + n * D + 2 * i * slot, slot,
                                                      base + i * D) == 0
                desc = host[:n * D].numpy().view(np.int32).reshape(n, D // 4)
                coefs = int(sum(desc[i, 16 + c] * desc[i, 20 + c] * 64 for i in range(n) for c in range(3)))
                dev = torch.device('cuda')
                d = host.to(dev)
                outd = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
                planes = torch.empty(n * slot, dtype=torch.uint8, device=dev)
                args = (d[n * D:].view(torch.int16), d[:n * D], outd, slot, planes)
                for _ in range(3):
                    hip_ops.jpeg_pixels_bgr(*args)
                ts = []
                for _ in range(20):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    hip_ops.jpeg_pixels_bgr(*args)
                    e1.record()
                    e1.synchronize()
                    ts.append(e0.elapsed_time(e1) * 1e3)
                us = float(np.median(ts))
                nbytes = coefs * 2 + coefs + coefs + n * H * W * 3 + n * D
                got = outd.cpu().numpy()
                eq = True
                for i in range(n):
                    pil_into(paths[i], out1)
                    eq = eq and bool(np.array_equal(got[i], out1))
                r.update(batch=n, device_us_per_batch=round(us, 1), device_us_min=round(min(ts), 1),
                         device_bytes_per_batch=nbytes, device_gbps=round(nbytes / us / 1e3, 1), byte_equal=eq)
            for k in ('pil', 'native_entropy'):
                r['host_ms_per_image'][k] = {t: round(v, 3) for t, v in r['host_ms_per_image'][k].items()}
            r['host_twin_ms_per_image'] = round(r['host_twin_ms_per_image'], 3)
            res['sizes'][f'{H}x{W}'] = r
    print(json.dumps(res))


if __name__ == '__main__':
    main()
