#!/usr/bin/env python
"""Time drawing detections on one image, on the device and with Pillow on the host; prints one JSON line
(kept as profiles/draw_bench.json):

    python tools/bench_draw.py [--height 1024] [--width 2048] [--detections 100] [--repeats 30] [--warmup 5]

Medians over ``--repeats`` runs, milliseconds per image:
  draw_device_ms        csrc/draw.hip alone (HIP events around the launch; the display list is already resident)
  draw_call_ms          ``oadg_draw.draw_items``: checks, upload of the list, launch, until the stream is idle (wall clock)
  show_device_ms        copy + draw + PNG encode + stream to the host + the file written: what --show-dir adds per image
                        when nothing overlaps it (wall clock)
  pillow_draw_ms        the same rectangles, plates and labels with one ``ImageDraw`` on the host
  pillow_draw_save_ms   ... and ``Image.save`` as PNG (Pillow's default compression level)
Records, not gates.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CLASSES = ('person', 'rider', 'car', 'truck', 'bus', 'train', 'motorcycle', 'bicycle')


def detections(n, H, W, seed=0):
    rs = np.random.RandomState(seed)
    bw, bh = rs.uniform(24, 400, n), rs.uniform(24, 400, n)
    x0, y0 = rs.uniform(0, W - bw), rs.uniform(0, H - bh)
    boxes = np.stack([x0, y0, x0 + bw, y0 + bh, rs.uniform(0.3, 1.0, n)], 1).astype(np.float32)
    labels = rs.randint(0, len(CLASSES), n)
    return [boxes[labels == c] for c in range(len(CLASSES))]


def pillow_draw(rgb, items, text, path=None):
    from PIL import Image, ImageDraw, ImageFont
    font = ImageFont.load_default_imagefont()
    im = Image.fromarray(rgb)
    d = ImageDraw.Draw(im)
    for kind, a, b, c, e, w, colour, _ in items.tolist():
        col = ((colour >> 16) & 255, (colour >> 8) & 255, colour & 255)           # B, G, R rows on an R, G, B image
        if kind == 0:
            d.rectangle([a, b, c, e], outline=col, width=w)
        elif kind == 1:
            d.rectangle([a, b, c, e], fill=col)
        else:
            d.text((a, b), text[c:c + e].decode('latin-1'), font=font, fill=col)
    if path is not None:
        im.save(path)
    return im


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times)


def main(argv=None):
    p = argparse.ArgumentParser(description='time drawing detections on the device and on the host')
    p.add_argument('--height', type=int, default=1024)
    p.add_argument('--width', type=int, default=2048)
    p.add_argument('--detections', type=int, default=100)
    p.add_argument('--repeats', type=int, default=30)
    p.add_argument('--warmup', type=int, default=5)
    a = p.parse_args(argv)
    import torch
    import oadg_draw
    from oadg_amd import _lib, staging
    from oadg_amd import visualization as V
    if not torch.cuda.is_available():
        raise RuntimeError('tools/bench_draw.py times the MI355X path; there is no CPU fallback')
    dev = torch.device('cuda', torch.cuda.current_device())
    H, W = a.height, a.width
    from oadg_amd.pipelines import SyntheticCityscapes
    src = SyntheticCityscapes(img_shape=(H, W), device=dev).image(0)[None]      # (low-pass noise: the project's stand-in image)
    bgr = src[0].cpu().numpy()
    result = detections(a.detections, H, W)
    items, text = V.det_items(result, CLASSES, score_thr=0.3)
    joined = V.join_lists([(items, text)])
    work = src.clone()
    L = _lib.lib()

    d_items, d_off, d_text = staging.upload([joined[0].reshape(-1), joined[1], joined[2]], dev)
    device_ms = []
    for k in range(a.warmup + a.repeats):
        work.copy_(src)
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _lib.check(L.oadg_draw_items_u8(_lib.ptr(work), 1, H, W, _lib.ptr(d_items), _lib.ptr(d_off), len(items), _lib.ptr(d_text),
                                        len(text), _lib.stream_ptr()), 'oadg_draw_items_u8')
        t1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            device_ms.append(t0.elapsed_time(t1))

    def draw_call():
        oadg_draw.draw_items(work, *joined)
        torch.cuda.synchronize()

    with tempfile.TemporaryDirectory() as tmp:
        enc = oadg_draw.PngEncoder(dev, slots=1)
        path = os.path.join(tmp, 'device.png')

        def show_device():
            drawn = V.draw_detections(src, [result], CLASSES, 0.3)
            job = enc.launch(drawn, bgr=True)
            (address, nbytes), = enc.finish(job)
            oadg_draw.write_png(enc.L, path, address, nbytes, H, W)

        rgb = np.ascontiguousarray(bgr[:, :, ::-1])
        host_path = os.path.join(tmp, 'host.png')
        out = dict(
            image=[H, W], detections=int(len(items) // 3), rows=int(len(items)), repeats=a.repeats,
            draw_device_ms=round(statistics.median(device_ms), 4),
            draw_call_ms=round(median_ms(draw_call, a.repeats, a.warmup), 4),
            show_device_ms=round(median_ms(show_device, a.repeats, a.warmup), 3),
            device_png_bytes=os.path.getsize(path),
            pillow_draw_ms=round(median_ms(lambda: pillow_draw(rgb, items, text), a.repeats, a.warmup), 3),
            pillow_draw_save_ms=round(median_ms(lambda: pillow_draw(rgb, items, text, host_path), max(3, a.repeats // 5), 1), 3),
            pillow_png_bytes=os.path.getsize(host_path))
    print(json.dumps(out))
    return 0


if __name__ == '__main__':
    sys.exit(main())
