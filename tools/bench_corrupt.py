"""The robustness benchmark's on-the-fly corruptions (test_robustness.py --load-dataset original): the host path
(``corrupt()``: numpy / scipy / Pillow, one image at a time on one thread) against the device path of ``Corrupt.batch``
(pipelines/corrupt_device.py, csrc/corrupt.hip; for pixelate and jpeg_compression oadg_recompress.py, csrc/recompress.hip).
Prints one JSON line.

usage: python tools/bench_corrupt.py [--batch 4] [--reps 3] [--severities 3 5] [--names ...]

Per benchmark name and severity, on synthetic 1024x2048 images (lowpass noise):
  host_s_per_image: corrupt() on one image, one thread
  device: for the names of DEVICE_CORRUPTIONS and DEVICE_CODEC_CORRUPTIONS, a resident batch of --batch images through
      Corrupt.batch after one warm-up, between synchronisations, median of --reps: ms_per_image (wall), split into
      host_ms_per_image (draws, tables, glass_blur's shuffle: corrupt_device.STATS; the codec names' small tables are not
      timed apart and count as device time) and device_ms_per_image (the rest: launches, uploads, kernels, the read of the
      codec route's flags); byte_equal: image 0 of the batch equals the host result under the same seed; host_fallbacks
      (codec names): images of the timed batches the device handed back to Pillow
  projected_hours: the full benchmark (15 names x 5 severities x 500 images), each name at the mean of its measured
      severities, host only and with the device routing; frost (photographs not in the repository) is left out of both
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

BENCHMARK = ('gaussian_noise', 'shot_noise', 'impulse_noise', 'defocus_blur', 'glass_blur', 'motion_blur', 'zoom_blur',
             'snow', 'frost', 'fog', 'brightness', 'contrast', 'elastic_transform', 'pixelate', 'jpeg_compression')
H, W, IMAGES, SEVERITIES = 1024, 2048, 500, 5


def images(n):
    from inputs import lowpass_image
    out = []
    for i in range(n):
        rs = np.random.RandomState(i)
        a = lowpass_image(rs, H, W, 8).astype(np.int32) + rs.randint(-8, 9, (H, W, 3))
        out.append(np.clip(a, 0, 255).astype(np.uint8))
    return np.stack(out)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=4)
    p.add_argument('--reps', type=int, default=3)
    p.add_argument('--severities', type=int, nargs='+', default=[3, 5])
    p.add_argument('--names', nargs='+', default=list(BENCHMARK) + ['gaussian_blur', 'saturate'])
    a = p.parse_args()
    import torch
    from oadg_amd.pipelines import corrupt_device
    from oadg_amd.pipelines.corrupt import DEVICE_CODEC_CORRUPTIONS, DEVICE_CORRUPTIONS, NEEDS_ASSETS, Corrupt, corrupt
    imgs = images(a.batch)
    gpu = torch.cuda.is_available()
    x = torch.from_numpy(imgs).cuda() if gpu else None
    res = dict(size=[H, W], batch=a.batch, severities=a.severities, names={})
    for name in a.names:
        if name in NEEDS_ASSETS and not os.environ.get('OADG_FROST_DIR'):
            res['names'][name] = None
            continue
        per = {}
        for s in a.severities:
            np.random.seed(0)
            t = time.perf_counter()
            ref = corrupt(imgs[0], name, s)
            r = dict(host_s_per_image=round(time.perf_counter() - t, 4))
            if gpu and (name in DEVICE_CORRUPTIONS or name in DEVICE_CODEC_CORRUPTIONS):
                c = Corrupt(name, s)
                np.random.seed(0)
                out = c.batch(x)
                r['byte_equal'] = bool(np.array_equal(out[0].cpu().numpy(), ref))
                walls, hosts, fell_back = [], [], Corrupt.runs['host']
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    h0 = corrupt_device.STATS['host_s']
                    t = time.perf_counter()
                    c.batch(x)
                    torch.cuda.synchronize()
                    walls.append(time.perf_counter() - t)
                    hosts.append(corrupt_device.STATS['host_s'] - h0)
                k = int(np.argsort(walls)[len(walls) // 2])
                wall, host = walls[k] / a.batch * 1e3, hosts[k] / a.batch * 1e3
                r['device'] = dict(ms_per_image=round(wall, 3), host_ms_per_image=round(host, 3),
                                   device_ms_per_image=round(wall - host, 3))
                if name in DEVICE_CODEC_CORRUPTIONS:
                    r['device']['host_fallbacks'] = Corrupt.runs['host'] - fell_back
            per[s] = r
        res['names'][name] = per

    def hours(device):
        total = 0.0
        for name, per in res['names'].items():
            if per is None or name not in BENCHMARK:
                continue
            secs = [r['device']['ms_per_image'] / 1e3 if device and 'device' in r else r['host_s_per_image']
                    for r in per.values()]
            total += float(np.mean(secs)) * SEVERITIES * IMAGES
        return round(total / 3600.0, 3)
    res['projected_hours'] = dict(host=hours(False), device_routing=hours(True) if gpu else None,
                                  names=[n for n in a.names if res['names'][n] is not None and n in BENCHMARK])
    print(json.dumps(res))


if __name__ == '__main__':
    main()
