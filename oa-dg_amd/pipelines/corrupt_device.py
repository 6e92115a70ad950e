"""The device path of ``Corrupt.batch`` (pipelines/corrupt.py) for the names of ``DEVICE_CORRUPTIONS``: a resident uint8
[N, H, W, 3] batch is corrupted by csrc/corrupt.hip, byte for byte as ``corrupt()`` corrupts each image on the host.

Only the deterministic filtering and resampling moves.  Every random draw is made here on the host, with the numpy calls,
shapes and order of ``corrupt()``, image by image in batch order, so numpy's global stream ends where the host loop leaves
it.  The filter weights and the uint8 -> float tables are computed by the same numpy expressions as the host path, then
uploaded with the draws through one pinned slot per batch (staging.upload).  glass_blur's sequential shuffle stays the host
loop (csrc/corrupt_host.hip) between its two device blurs.  Channel order is left as the batch holds it.
"""
import time

import numpy as np
import torch

from .. import _lib, hip_ops, staging
from . import corrupt as C

# seconds spent on the host side of the device path (draws, weights, tap tables, glass_blur's shuffle): tools/bench_corrupt.py
STATS = dict(host_s=0.0)

_LUT64 = np.arange(256) / 255.                                   # np.array(x) / 255.
_LUT32_ZOOM = (np.arange(256) / 255.).astype(np.float32)          # zoom_blur: (np.array(x) / 255.).astype(np.float32)
_LUT32 = np.arange(256, dtype=np.float32) / 255.                  # snow, elastic: np.array(x, dtype=np.float32) / 255.


def _upload(device, *arrays):
    return staging.upload(arrays, device)


def gaussian_weights(sigma, truncate):
    """scipy.ndimage.gaussian_filter1d's weights (_gaussian_kernel1d(sigma, 0, int(truncate * sd + 0.5))[::-1])"""
    radius = int(truncate * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    phi = phi / phi.sum()
    w = np.ascontiguousarray(phi[::-1])
    assert np.array_equal(w, w[::-1]), 'the device correlation assumes a symmetric kernel'
    return w


def zoom_geometry(h, w, z):
    """_clipped_zoom's centre crop and scipy.ndimage.zoom's order-1 grid for it: (top, left, ch, cw), (Ho, Wo), (ry, rx)"""
    ch, cw = int(np.ceil(h / float(z))), int(np.ceil(w / float(z)))
    top, left = (h - ch) // 2, (w - cw) // 2
    Ho, Wo = int(round(ch * z)), int(round(cw * z))
    ry = (ch - 1) / (Ho - 1) if Ho != 1 else 1.0
    rx = (cw - 1) / (Wo - 1) if Wo != 1 else 1.0
    return (top, left, ch, cw), (Ho, Wo), (ry, rx)


def _motion_tables(shapes_angles, radius, sigma):
    """kernel, taps int32 [N, T, 2] and counts int32 [N] of C._motion_taps for each (shape, angle)"""
    kernel = C._motion_kernel(radius, sigma)
    T = kernel.shape[0]
    taps = np.zeros((len(shapes_angles), T, 2), np.int32)
    counts = np.zeros(len(shapes_angles), np.int32)
    for i, (shape, angle) in enumerate(shapes_angles):
        t = C._motion_taps(shape, T, angle)
        counts[i] = len(t)
        if t:
            taps[i, :len(t)] = t
    return kernel, taps, counts


def _separable(src, weights, mode, lut=None):
    """gaussian_filter over axes 0 and 1 of [N, H, W, C] (float64 between and after the passes)"""
    w, = _upload(src.device, weights)
    tmp = torch.empty(src.shape, dtype=torch.float64, device=src.device)
    out = torch.empty_like(tmp)
    hip_ops.corrupt_correlate1d(src, tmp, 0, w, mode, lut)
    hip_ops.corrupt_correlate1d(tmp, out, 1, w, mode)
    return out


def _separable_2(src, w0, w1, mode):
    """the same with separate weights per axis (elastic_transform's sigma = (h, w) * 0.01)"""
    d0, d1 = _upload(src.device, w0, w1)
    tmp = torch.empty(src.shape, dtype=torch.float64, device=src.device)
    out = torch.empty_like(tmp)
    hip_ops.corrupt_correlate1d(src, tmp, 0, d0, mode)
    hip_ops.corrupt_correlate1d(tmp, out, 1, d1, mode)
    return out


def _gaussian_blur(x, severity):
    c = [1, 2, 3, 4, 6][severity - 1]
    lut, = _upload(x.device, _LUT64)
    blurred = _separable(x, gaussian_weights(c, 4.0), 'nearest', lut)
    out = torch.empty_like(x)
    hip_ops.corrupt_epilogue(blurred, out, _lib.CORRUPT_TO_U8_CLIP)
    return out


def _glass_blur(x, severity):
    sigma, delta, iters = [(0.7, 1, 2), (0.9, 2, 1), (1, 2, 3), (1.1, 3, 2), (1.5, 4, 2)][severity - 1]
    N, h, w, _ = x.shape
    t0 = time.perf_counter()
    wts = gaussian_weights(np.float64(sigma), 4.0)
    lut, = _upload(x.device, _LUT64)
    STATS['host_s'] += time.perf_counter() - t0
    mid = torch.empty_like(x)
    hip_ops.corrupt_epilogue(_separable(x, wts, 'nearest', lut), mid, _lib.CORRUPT_TO_U8)
    host = mid.cpu().numpy()
    t0 = time.perf_counter()
    if h > 2 * delta and w > 2 * delta:
        L = _lib.lib()
        for img in host:                                   # (contiguous [h, w, 3] views of the downloaded batch)
            d = np.ascontiguousarray(np.random.randint(-delta, delta, size=(iters, h - 2 * delta, w - 2 * delta, 2)),
                                     np.int32)
            _lib.check(L.oadg_glass_shuffle_u8(img.ctypes.data, h, w, 3, delta, iters, d.ctypes.data),
                       'oadg_glass_shuffle_u8')
    shuffled, lut = _upload(x.device, host, _LUT64)
    STATS['host_s'] += time.perf_counter() - t0
    out = torch.empty_like(x)
    hip_ops.corrupt_epilogue(_separable(shuffled, wts, 'nearest', lut), out, _lib.CORRUPT_TO_U8_CLIP)
    return out


def _defocus_blur(x, severity):
    radius, alias = [(3, 0.1), (4, 0.5), (6, 0.5), (8, 0.5), (10, 0.5)][severity - 1]
    kernel = C._disk(radius=radius, alias_blur=alias).astype(np.float64)
    K = kernel.shape[0]
    ii, jj = np.nonzero(np.abs(kernel) > np.finfo(np.float64).eps)        # row-major, as scipy keeps its footprint
    dydx = np.stack([ii - K // 2, jj - K // 2], -1).astype(np.int32)
    taps, wts, lut = _upload(x.device, dydx, kernel[ii, jj], _LUT64)
    out = torch.empty_like(x)
    hip_ops.corrupt_defocus(x, out, taps, wts, lut)
    return out


def _zoom_blur(x, severity):
    c = [np.arange(1, 1.11, 0.01), np.arange(1, 1.16, 0.01), np.arange(1, 1.21, 0.02), np.arange(1, 1.26, 0.02),
         np.arange(1, 1.33, 0.03)][severity - 1]
    N, h, w, _ = x.shape
    ratios, geo = np.zeros((len(c), 2)), np.zeros((len(c), 4), np.int32)
    for k, z in enumerate(c):
        crop, (Ho, Wo), ratios[k] = zoom_geometry(h, w, z)
        assert Ho >= h and Wo >= w, 'the zoomed layer covers the image'
        geo[k] = crop
    r, g, lut = _upload(x.device, ratios, geo, _LUT32_ZOOM)
    out = torch.empty_like(x)
    hip_ops.corrupt_zoom_blur(x, out, r, g, lut)
    return out


def _motion_blur(x, severity):
    radius, sigma = [(10, 3), (15, 5), (15, 8), (15, 12), (20, 15)][severity - 1]
    N, h, w, _ = x.shape
    t0 = time.perf_counter()
    angles = [np.random.uniform(-45, 45) for _ in range(N)]
    kernel, taps, counts = _motion_tables([((h, w), a) for a in angles], radius, sigma)
    k, t, n = _upload(x.device, kernel, taps, counts)
    STATS['host_s'] += time.perf_counter() - t0
    out = torch.empty_like(x)
    hip_ops.corrupt_motion_blur(x, out, t, n, k)
    return out


def _snow(x, severity):
    c = [(0.1, 0.3, 3, 0.5, 10, 4, 0.8), (0.2, 0.3, 2, 0.5, 12, 4, 0.7), (0.55, 0.3, 4, 0.9, 12, 8, 0.7),
         (0.55, 0.3, 4.5, 0.85, 12, 8, 0.65), (0.55, 0.3, 2.5, 0.85, 12, 12, 0.55)][severity - 1]
    N, h, w, _ = x.shape
    crop, (Ho, Wo), ratios = zoom_geometry(h, w, c[2])
    t0 = time.perf_counter()
    layers, angles = np.empty((N, h, w)), []
    for i in range(N):                                     # per image: the layer, then the angle
        layers[i] = np.random.normal(size=(h, w), loc=c[0], scale=c[1])
        angles.append(np.random.uniform(-135, -45))
    kernel, taps, counts = _motion_tables([((Ho, Wo), a) for a in angles], c[4], c[5])
    lay, k, t, n, lut32, lut64 = _upload(x.device, layers, kernel, taps, counts, _LUT32, _LUT64)
    STATS['host_s'] += time.perf_counter() - t0
    zoomed = torch.empty((N, Ho, Wo), dtype=torch.float64, device=x.device)
    hip_ops.corrupt_snow_layer(lay, zoomed, crop, ratios, c[3])
    q = torch.empty((N, Ho, Wo), dtype=torch.uint8, device=x.device)
    hip_ops.corrupt_motion_blur(zoomed, q, t, n, k)
    out = torch.empty_like(x)
    hip_ops.corrupt_snow_blend(x, q, out, np.float32(c[6]), np.float32(1 - c[6]), lut32, lut64)
    return out


def _elastic_transform(x, severity):
    N, h, w, _ = x.shape
    sigma = np.array((h, w)) * 0.01
    alpha = [250 * 0.05, 250 * 0.065, 250 * 0.085, 250 * 0.1, 250 * 0.12][severity - 1]
    max_d = h * 0.005
    t0 = time.perf_counter()
    draws = np.empty((2, N, h, w, 1))
    for i in range(N):                                     # per image: dx's field, then dy's
        draws[0, i, ..., 0] = np.random.uniform(-max_d, max_d, size=(h, w))
        draws[1, i, ..., 0] = np.random.uniform(-max_d, max_d, size=(h, w))
    w0, w1 = gaussian_weights(sigma[0], 3), gaussian_weights(sigma[1], 3)
    dev, lut = _upload(x.device, draws, _LUT32)
    STATS['host_s'] += time.perf_counter() - t0
    fields = []
    for k in range(2):
        f = torch.empty((N, h, w), dtype=torch.float32, device=x.device)
        hip_ops.corrupt_epilogue(_separable_2(dev[k], w0, w1, 'reflect'), f, _lib.CORRUPT_TO_F32, alpha)
        fields.append(f)
    out = torch.empty_like(x)
    hip_ops.corrupt_elastic(x, fields[0], fields[1], out, lut)
    return out


def _brightness(x, severity):
    c = [.1, .2, .3, .4, .5][severity - 1]
    lut, = _upload(x.device, _LUT64)
    out = torch.empty_like(x)
    hip_ops.corrupt_hsv(x, out, _lib.CORRUPT_BRIGHTNESS, c, 0.0, lut)
    return out


def _saturate(x, severity):
    c = [(0.3, 0), (0.1, 0), (2, 0), (5, 0.1), (20, 0.2)][severity - 1]
    lut, = _upload(x.device, _LUT64)
    out = torch.empty_like(x)
    hip_ops.corrupt_hsv(x, out, _lib.CORRUPT_SATURATE, c[0], c[1], lut)
    return out


_DEVICE_FUNCS = dict(gaussian_blur=_gaussian_blur, glass_blur=_glass_blur, defocus_blur=_defocus_blur,
                     motion_blur=_motion_blur, zoom_blur=_zoom_blur, snow=_snow, brightness=_brightness,
                     saturate=_saturate, elastic_transform=_elastic_transform)
assert tuple(_DEVICE_FUNCS) == C.DEVICE_CORRUPTIONS


def corrupt_batch(imgs_u8, corruption_name, severity):
    """uint8 [N, H, W, 3] on the device -> a new uint8 batch, each image equal to corrupt(image, name, severity), on
    torch's current stream of the batch's device"""
    if corruption_name not in _DEVICE_FUNCS:
        raise ValueError(f'{corruption_name!r} has no device path')
    if not 1 <= severity <= 5:
        raise ValueError('severity must be 1 ... 5 on the device path')
    if imgs_u8.dtype != torch.uint8 or imgs_u8.dim() != 4 or imgs_u8.shape[3] != 3:
        raise TypeError('corrupt expects a uint8 HxWx3 image')
    with torch.cuda.device(imgs_u8.device):
        return _DEVICE_FUNCS[corruption_name](imgs_u8.contiguous(), severity)
