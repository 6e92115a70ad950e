"""Throughput and output size of the device PNG encoder (csrc/png_encode.hip behind tools/analysis_tools/
get_corrupted_dataset.py) against what the reference does - PIL's default save - and against the fastest host path of the
same format, zlib's Z_HUFFMAN_ONLY over Sub-filtered rows on 16 threads.  Prints one JSON line.  Needs the GPU.

usage: python tools/bench_png_encode.py [--n 16] [--rounds 64] [--workers 16] [--pil-images 2] [--height 1024] [--width 2048]

The batch is the first --n images tools/make_synthetic_coco.py writes (SyntheticCityscapes, B, G, R as the loaders hold
them), clean and under two device corruptions (gaussian_blur and brightness at severity 3).  Per variant:
  device.ms_per_image        HIP events around oadg_png_encode_rgb8 (three launches per batch of 8), per image
  device.copy_ms_per_image   the device -> pinned copy of the streams (the tool copies whole capacity slots), by events
  device.write_ms_per_image  oadg_png_write_rgb8 alone, wall clock over --workers threads (files into a temporary directory)
  device.images_per_s        batches -> files end to end, wall clock, as the tool pipelines them: the encode and copy of one
                             batch run while the files of the batch before are written (--rounds passes over the batch)
  device.bytes_per_image     mean stream length (the file adds 57 bytes); total_bytes: all streams of the timed passes
  pil                        PIL.Image.fromarray(rgb).save(path) - default level - of the first --pil-images, one thread
  zlib_huffman_only          zlib.compressobj(strategy=Z_HUFFMAN_ONLY) over the Sub-filtered scanlines of every image on 16
                             threads (the call releases the interpreter lock); numpy's filtering is NOT in the time
  ratio.bytes_vs_pil, ratio.images_per_s_vs_pil_1_thread, ratio.images_per_s_vs_zlib_16_threads
  round_trip                 every file of the timed pass decodes (oadg_png_decode_bgr) to the batch it was made from
  clocks                     sclk / power sampled during the device passes (bench.ClockSampler)
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_tool():
    spec = importlib.util.spec_from_file_location('get_corrupted_dataset_tool',
                                                  os.path.join(ROOT, 'tools', 'analysis_tools', 'get_corrupted_dataset.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def device_pass(T, enc, pool, batches, out_dir, H, W):
    """the tool's pipeline over ``batches`` -> (paths, stream bytes of the pass)"""
    pending, futures_all, paths_all, k = None, [], [], 0

    def finish(p):
        job, paths = p
        streams = enc.finish(job)
        fs = [pool.submit(T.write_png, enc.L, path, addr, nb, H, W) for path, (addr, nb) in zip(paths, streams)]
        enc.release(job, fs)
        futures_all.extend(fs)

    for imgs in batches:
        paths = [os.path.join(out_dir, f'{k + i}.png') for i in range(imgs.shape[0])]
        k += imgs.shape[0]
        paths_all.extend(paths)
        job = enc.launch(imgs, bgr=True)
        if pending is not None:
            finish(pending)
        pending = (job, paths)
    finish(pending)
    return paths_all, sum(f.result() for f in futures_all)


def measure_variant(T, torch, dev, batch, a, tmp, name):
    from PIL import Image
    from oadg_amd import _lib
    L = _lib.lib()
    n, H, W, _ = batch.shape
    batches = [batch[i:i + T.BATCH] for i in range(0, n, T.BATCH)]
    out_dir = os.path.join(tmp, name)
    os.makedirs(out_dir, exist_ok=True)
    workers = T.writer_threads(a.workers)
    res = {}
    with ThreadPoolExecutor(workers) as pool:
        enc = T.PngEncoder(dev)
        device_pass(T, enc, pool, batches, out_dir, H, W)                      # untimed: code objects, pinned slots, threads
        torch.cuda.synchronize()
        enc.device_ms, enc.images = 0.0, 0
        t0 = time.perf_counter()
        for _ in range(a.rounds):
            paths, nbytes = device_pass(T, enc, pool, batches, out_dir, H, W)
        wall = time.perf_counter() - t0
        images = a.rounds * n
        device_ms = enc.device_ms / enc.images
        # the copy and the writes alone
        job = enc.launch(batches[0], bgr=True)
        streams = enc.finish(job)
        cap, nb = job['cap'], batches[0].shape[0]
        dstreams = torch.empty((nb * cap,), dtype=torch.uint8, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        job['slot']['host'][:nb * cap].copy_(dstreams, non_blocking=True)
        e1.record()
        e1.synchronize()
        copy_ms = e0.elapsed_time(e1) / nb
        job = enc.launch(batches[0], bgr=True)
        streams = enc.finish(job)
        t1 = time.perf_counter()
        list(pool.map(lambda x: T.write_png(L, os.path.join(out_dir, f'w{x[0]}.png'), x[1][0], x[1][1], H, W), enumerate(streams)))
        write_ms = (time.perf_counter() - t1) * 1e3 / nb
        enc.release(job, [])
    ok = True
    host = batch.cpu().numpy()
    got = np.empty((H, W, 3), np.uint8)
    for i, p in enumerate(paths):
        rc = L.oadg_png_decode_bgr(p.encode(), got.ctypes.data, H, W)
        ok = ok and rc == 0 and np.array_equal(got, host[i])
    res['device'] = dict(ms_per_image=round(device_ms, 4),
                         copy_ms_per_image=round(copy_ms, 4), write_ms_per_image=round(write_ms, 4), writer_threads=workers,
                         images_per_s=round(images / wall, 1), wall_s=round(wall, 3), images=images,
                         bytes_per_image=int(nbytes / n), total_bytes=int(nbytes) * a.rounds)
    # the reference: PIL's default save, one thread
    rgb = np.ascontiguousarray(host[:, :, :, ::-1])
    k = max(1, min(a.pil_images, n))
    t0 = time.perf_counter()
    for i in range(k):
        Image.fromarray(rgb[i]).save(os.path.join(out_dir, f'pil{i}.png'))
    pil_s = (time.perf_counter() - t0) / k
    pil_bytes = sum(os.path.getsize(os.path.join(out_dir, f'pil{i}.png')) for i in range(k)) / k
    dev_bytes_same = sum(os.path.getsize(paths[i]) for i in range(k)) / k
    res['pil'] = dict(images=k, threads=1, s_per_image=round(pil_s, 4), bytes_per_image=int(pil_bytes))
    # the fastest host path of the same format
    lines = np.zeros((n, H, 3 * W + 1), np.uint8)
    lines[:, :, 0] = 1
    lines[:, :, 1:4] = rgb[:, :, 0]
    lines[:, :, 4:] = (rgb[:, :, 1:].astype(np.int16) - rgb[:, :, :-1]).astype(np.uint8).reshape(n, H, -1)
    blobs = [lines[i].tobytes() for i in range(n)]

    def huff(b):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
        return len(c.compress(b)) + len(c.flush())
    with ThreadPoolExecutor(16) as pool:
        list(pool.map(huff, blobs[:16]))
        t0 = time.perf_counter()
        sizes = list(pool.map(huff, blobs))
        z_s = time.perf_counter() - t0
    res['zlib_huffman_only'] = dict(threads=16, images_per_s=round(n / z_s, 1), bytes_per_image=int(sum(sizes) / n))
    res['ratio'] = dict(bytes_vs_pil=round(dev_bytes_same / pil_bytes, 4),
                        images_per_s_vs_pil_1_thread=round(images / wall * pil_s, 1),
                        images_per_s_vs_zlib_16_threads=round(images / wall / (n / z_s), 2))
    res['round_trip'] = bool(ok)
    for p in os.listdir(out_dir):
        os.unlink(os.path.join(out_dir, p))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=16)
    p.add_argument('--rounds', type=int, default=64, help='timed passes over the batch (64 x 16 images: most of a second)')
    p.add_argument('--workers', type=int, default=16)
    p.add_argument('--pil-images', type=int, default=2)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=2048)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_png_encode.py measures the device path: it needs the GPU')
    from bench import ClockSampler
    from oadg_amd.pipelines import SyntheticCityscapes
    from oadg_amd.pipelines.corrupt import Corrupt
    T = load_tool()
    dev = torch.device('cuda', torch.cuda.current_device())
    ds = SyntheticCityscapes(img_shape=(a.height, a.width), num_boxes=20, device=dev)      # make_synthetic_coco.py's images
    clean = torch.stack([ds.image(i) for i in range(a.n)]).contiguous()
    np.random.seed(0)
    variants = dict(clean=clean)
    for name in ('gaussian_blur', 'brightness'):
        variants[f'{name}_3'] = torch.cat([Corrupt(name, 3).batch(clean[i:i + T.BATCH]) for i in range(0, a.n, T.BATCH)])
    res = dict(n=a.n, height=a.height, width=a.width, rounds=a.rounds, raw_bytes_per_image=a.height * a.width * 3,
               segments_per_image=int(T.PngEncoder(dev).L.oadg_png_encode_segments(a.height, a.width)), variants={})
    sampler = ClockSampler().start()
    with tempfile.TemporaryDirectory() as tmp:
        for name, batch in variants.items():
            res['variants'][name] = measure_variant(T, torch, dev, batch, a, tmp, name)
    res['clocks'] = sampler.stop()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
