"""Throughput of tools/dataset_converters/cityscapes.py against a numpy restatement of the reference's per-instance loop.
Prints one JSON line.  Needs the GPU (the converter has no host path).

usage: python tools/bench_cityscapes_convert.py [--n 64] [--instances 40] [--nproc 16] [--ref-files 8]

Writes --n synthetic 1024 x 2048 gtFine instance maps (stuff stripes, --instances ellipses with distinct instance ids, 16-bit
PNG as Cityscapes ships them) into a temporary tree, converts it once untimed (code objects, pinned buffers, the thread
pool) and once timed:
  tool.images_per_s          files -> json, wall clock (ends after the json is on disk)
  tool.split_s               decode (threads fill a pinned slot; the previous batch is on the device meanwhile), device_wait
                             (the host blocked on the device's counts and results after that decode), assemble (records and
                             change points -> annotation dicts and RLE strings), json (cvt_annotations + json.dump)
  tool.device_ms_per_image   HIP events around the two C-ABI calls of each batch (six launches), summed, per image
  tool.map_bytes_per_image / device_gbps: the map is read three times (statistics, change-point count, change-point write)
  reference_numpy            one thread over the first --ref-files files: PIL decode, np.unique, and per instance
                             `inst == id` in Fortran order -> np.diff run lengths, area, box (what the reference's loop with
                             pycocotools computes; pycocotools' C run-length encoder is faster than np.diff, its per-instance
                             full-map comparison is the same)
  same_annotations           the two agree on every box, area and run-length string of the files both converted
  clocks                     sclk / power sampled during the timed pass (bench.ClockSampler)
"""
import argparse
import importlib.util
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_tool():
    spec = importlib.util.spec_from_file_location('cityscapes_converter_tool',
                                                  os.path.join(ROOT, 'tools', 'dataset_converters', 'cityscapes.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_map(seed, H, W, instances):
    rs = np.random.RandomState(seed)
    m = np.empty((H, W), dtype=np.uint16)
    for k, b in enumerate((23, 21, 11, 11, 8, 7, 7, 7)):              # sky, vegetation, building, sidewalk, road
        m[k * H // 8:(k + 1) * H // 8] = b
    labels = rs.choice([24, 25, 26, 26, 26, 27, 28, 32, 33], instances)
    for i, l in enumerate(labels):
        h, w = rs.randint(20, 260), rs.randint(20, 320)
        y0, x0 = rs.randint(H // 4, H - h), rs.randint(0, W - w)
        yy, xx = np.mgrid[0:h, 0:w]
        inside = ((yy - (h - 1) / 2) / (h / 2)) ** 2 + ((xx - (w - 1) / 2) / (w / 2)) ** 2 <= 1.0
        m[y0:y0 + h, x0:x0 + w][inside] = int(l) * 1000 + i
    return m


def make_tree(root, n, H, W, instances):
    from PIL import Image
    for i in range(n):
        city = ('aachen', 'bochum', 'bremen', 'cologne')[i % 4]
        stem = f'{city}_{i:06d}_000019'
        for d in ('leftImg8bit', 'gtFine'):
            os.makedirs(os.path.join(root, d, 'train', city), exist_ok=True)
        # (the converter lists the images but never opens them)
        Image.fromarray(np.zeros((2, 2, 3), np.uint8)).save(os.path.join(root, 'leftImg8bit', 'train', city, f'{stem}_leftImg8bit.png'))
        Image.fromarray(synthetic_map(i, H, W, instances)).save(
            os.path.join(root, 'gtFine', 'train', city, f'{stem}_gtFine_instanceIds.png'))


def reference_numpy(T, files):
    """the reference's load_img_info restated with numpy, one thread"""
    from PIL import Image
    infos = []
    for f in files:
        with Image.open(f[1]) as im:
            inst = np.asarray(im).astype(np.uint16)
        H, W = inst.shape
        annos = []
        for k in np.unique(inst[inst >= 24]).tolist():
            label = T.label_of(k, f[1])
            if label not in T.KEPT:
                continue
            mask = np.asarray(inst == k, dtype=np.uint8, order='F')
            flat = mask.reshape(-1, order='F')
            change = np.nonzero(np.diff(flat))[0] + 1
            counts = np.diff(np.concatenate([[0], change, [H * W]]))
            if flat[0]:
                counts = np.concatenate([[0], counts])
            ys, xs = np.nonzero(mask)
            annos.append(dict(iscrowd=int(k < 1000), category_id=label,
                              bbox=[float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1),
                                    float(ys.max() - ys.min() + 1)], area=int(len(ys)),
                              segmentation=dict(size=[H, W], counts=T.rle_to_string(counts))))
        infos.append(T.image_info(f, H, W, annos))
    return infos


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--n', type=int, default=64)
    p.add_argument('--instances', type=int, default=40)
    p.add_argument('--nproc', type=int, default=16)
    p.add_argument('--ref-files', type=int, default=8)
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=2048)
    a = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_cityscapes_convert.py measures the device path: it needs the GPU')
    from bench import ClockSampler
    T = load_tool()
    H, W = a.height, a.width
    with tempfile.TemporaryDirectory() as tmp:
        make_tree(tmp, a.n, H, W, a.instances)
        files = T.collect_files(os.path.join(tmp, 'leftImg8bit', 'train'), os.path.join(tmp, 'gtFine', 'train'))
        out = os.path.join(tmp, 'train.json')
        T.cvt_annotations(T.collect_annotations(files, nproc=a.nproc), out)          # untimed warm-up pass
        torch.cuda.synchronize()
        sampler = ClockSampler().start()
        timers = {}
        t0 = time.perf_counter()
        infos = T.collect_annotations(files, nproc=a.nproc, timers=timers)
        t1 = time.perf_counter()
        T.cvt_annotations(infos, out)
        t2 = time.perf_counter()
        clocks = sampler.stop()
        nref = min(a.ref_files, len(files))
        t3 = time.perf_counter()
        ref = reference_numpy(T, files[:nref])
        t4 = time.perf_counter()
        same = all(r['anno_info'] == i['anno_info'] for r, i in zip(ref, infos))
        ninst = sum(len(i['anno_info']) for i in infos) / len(infos)
        png_mb = sum(os.path.getsize(f[1]) for f in files) / len(files) / 1e6
    map_bytes = 3 * H * W * 2
    dev_ms = timers['device_ms'] / a.n
    res = dict(n=a.n, height=H, width=W, instances_per_image=round(ninst, 1), png_mb_per_file=round(png_mb, 3),
               decode_threads=min(a.nproc, T.MAX_THREADS),
               tool=dict(images_per_s=round(a.n / (t2 - t0), 2), wall_s=round(t2 - t0, 3),
                         split_s=dict(decode=round(timers['decode_s'], 3), device_wait=round(timers['device_wait_s'], 3),
                                      assemble=round(timers['assemble_s'], 3), json=round(t2 - t1, 3)),
                         device_ms_per_image=round(dev_ms, 4), map_bytes_per_image=map_bytes,
                         device_gbps=round(map_bytes / (dev_ms * 1e-3) / 1e9, 1) if dev_ms > 0 else None),
               reference_numpy=dict(files=nref, threads=1, images_per_s=round(nref / (t4 - t3), 3),
                                    s_per_image=round((t4 - t3) / nref, 3)),
               same_annotations=bool(same), clocks=clocks)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
