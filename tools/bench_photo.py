#!/usr/bin/env python
"""Time PhotoMetricDistortion + CutOut + Normalize + Pad for a batch on the device; prints one JSON line
(kept as profiles/photo_bench.json):

    python tools/bench_photo.py [--batch 8] [--height 1024] [--width 2048] [--repeats 50] [--inner 20] [--warmup 10]

bf16 output, every photometric sub-step switched on, three holes per image.  Medians over ``--repeats`` HIP-event
windows of ``--inner`` back-to-back runs each, milliseconds per batch; the tables are uploaded before the timed window (they
are a few hundred bytes):
  fused_ms       ONE launch of csrc/photo.hip for the batch (``oadg_photo_normalize_batch``)
  normalize_ms   ``--batch`` plain ``oadg_oamix_normalize`` launches on the same images: they move the same bytes (3 B in,
                 6 B out per pixel) and do none of the arithmetic - the floor
  torch_ms       the same chain written with torch ops on the device, which materialises the float32 image and every
                 intermediate in HBM: what one would write without a kernel
  *_gbps         (3 + 6) bytes per pixel over the time
Records, not gates.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def torch_chain(x_u8, p, hole, fill, mean, stdinv):
    """the per-pixel chain of include/oadg_hip.h (CutOut first, every sub-step on) with torch ops: uint8 [N, H, W, 3] -> bf16"""
    import torch
    eps = torch.finfo(torch.float32).eps
    x = x_u8.float()
    x = torch.where(hole[..., None], fill, x)
    x = (x + p['delta']) * p['alpha_pre']
    b, g, r = x.unbind(-1)
    v, vmin = x.amax(-1), x.amin(-1)
    diff = v - vmin
    s = diff / (v.abs() + eps)
    d = 60.0 / (diff + eps)
    h = torch.where(v == r, (g - b) * d, torch.where(v == g, (b - r) * d + 120.0, (r - g) * d + 240.0))
    h = torch.where(h < 0, h + 360.0, h)
    s = s * p['sat']
    h = h + p['hue']
    h = torch.where(h > 360, h - 360.0, h)
    h = torch.where(h < 0, h + 360.0, h)
    h6 = h * (6.0 / 360.0)
    h6 = torch.where(h6 < 0, h6 + 6.0, torch.where(h6 >= 6, h6 - 6.0, h6))
    fl = h6.floor()
    f = h6 - fl
    sector = fl.long().clamp_(0, 5)
    tab = torch.stack([v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))], -1)
    idx = torch.tensor([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]], device=x.device)[sector]
    x = torch.where((s == 0)[..., None], v[..., None], tab.gather(-1, idx))
    x = x * p['alpha_post']
    x = x[..., list(p['perm'])]
    return ((x.flip(-1) - mean) * stdinv).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--height', type=int, default=1024)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    a = ap.parse_args()
    import torch
    import oadg_amd  # noqa: F401
    import oadg_photo
    from oadg_amd import _lib, staging
    from oadg_amd.pipelines import Normalize
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_photo.py measures on the GPU; there is none')
    dev = torch.device('cuda:0')
    N, H, W = a.batch, a.height, a.width
    Hp, Wp = -(-H // 32) * 32, -(-W // 32) * 32
    na = Normalize(MEAN, STD).as_args()
    imgs = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(0))
    f32 = np.float32
    p = dict(flags=_lib.PHOTO_PRESENT | _lib.PHOTO_DELTA | _lib.PHOTO_ALPHA_PRE | _lib.PHOTO_SAT | _lib.PHOTO_HUE |
             _lib.PHOTO_ALPHA_POST | _lib.PHOTO_PERM, mode=0, delta=f32(-11.5), alpha_pre=f32(1.2), sat=f32(0.8), hue=f32(12.25),
             alpha_post=f32(0.9), perm=(2, 0, 1))
    rects = np.array([[W // 8, H // 8, W // 4, H // 3], [W // 2, H // 2, W // 2 + W // 5, H // 2 + H // 10],
                      [W - 40, H - 30, W, H]], np.int32)
    table, all_rects = oadg_photo.build_table([imgs[i] for i in range(N)], [oadg_photo.sample(p, rects, (0, 0, 0))] * N, Hp, Wp)
    d_table, d_rects = staging.upload([table, all_rects], dev)
    mean, stdinv = (ctypes.c_float * 3)(*na['mean']), (ctypes.c_float * 3)(*na['stdinv'])
    out = torch.empty((N, Hp, Wp, 3), dtype=torch.bfloat16, device=dev)
    L = _lib.lib()

    def fused():
        _lib.check(L.oadg_photo_normalize_batch(_lib.ptr(d_table), N, _lib.ptr(d_rects), mean, stdinv, 1, _lib.ptr(out), 1, Hp,
                                                Wp, Hp * Wp * 3, _lib.stream_ptr()), 'oadg_photo_normalize_batch')

    def plain():
        for i in range(N):
            _lib.check(L.oadg_oamix_normalize(_lib.ptr(imgs[i]), H, W, mean, stdinv, 1, _lib.ptr(out[i]), 1, Hp, Wp,
                                              _lib.stream_ptr()), 'oadg_oamix_normalize')

    hole = torch.zeros((N, H, W), dtype=torch.bool, device=dev)
    for x1, y1, x2, y2 in rects.tolist():
        hole[:, y1:y2, x1:x2] = True
    t_mean, t_stdinv = torch.tensor(na['mean'], device=dev), torch.tensor(na['stdinv'], device=dev)
    t_fill = torch.zeros(3, device=dev)

    def eager():
        return torch_chain(imgs, p, hole, t_fill, t_mean, t_stdinv)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.inner)
        return statistics.median(ms), min(ms), max(ms)

    # the fused launch and the torch restatement agree (bf16 of nearly the same floats: torch's division and its order of
    # operations are its own) before anything is timed
    fused()
    ref = eager()
    diff = (out[:, :H, :W].float() - ref.float()).abs()
    close = float((diff <= 0.02 * ref.float().abs().clamp_min(1.0)).float().mean())
    del ref, diff
    res = dict(tool='bench_photo', batch=N, height=H, width=W, dtype='bf16', repeats=a.repeats, inner=a.inner, warmup=a.warmup,
               agree_with_torch_fraction=round(close, 6), device=torch.cuda.get_device_name(0))
    nbytes = N * (H * W * 3 + Hp * Wp * 6)
    for key, fn in (('fused', fused), ('normalize', plain), ('torch', eager), ('fused_again', fused)):
        med, lo, hi = timed(fn)
        res[key + '_ms'] = round(med, 4)
        res[key + '_min_max_ms'] = [round(lo, 4), round(hi, 4)]
        res[key + '_gbps'] = round(nbytes / med / 1e6, 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
