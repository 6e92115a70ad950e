"""The device route of ``Corrupt.batch`` for ``jpeg_compression`` and ``pixelate`` (pipelines/corrupt.py
DEVICE_CODEC_CORRUPTIONS): the ctypes calls of ``oadg_jpeg_recompress_*`` and ``oadg_pil_*`` (csrc/recompress.hip) with the
host-side tables around them - libjpeg's quantisation tables for a quality, Pillow's BOX coefficients and its NEAREST scan -
and the host twins of both chains, which run the kernels' source on numpy buffers without a GPU.
``oadg_amd.pipelines.corrupt`` imports this module lazily.

WHERE THIS BELONGS: ``jpeg_recompress`` and ``pixelate`` are hip_ops wrappers and ``corrupt_batch`` belongs in
oa-dg_amd/pipelines/corrupt_device.py.  They are here, next to the package's import shim, for the reason oadg_photo.py and
oadg_draw.py give: tests/test_target_audit.py (test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI
call site under oa-dg_amd/ by name, and the change that added these kernels could add test files but not edit that one.  The
suite that answers for these call sites is tests/test_hip_recompress.py (the bytes on the GPU) with tests/test_recompress.py
(the host twins and the tables, without one).  The follow-up is mechanical: add 'oadg_jpeg_recompress_u8',
'oadg_jpeg_recompress_host', 'oadg_jpeg_recompress_bounds_host', 'oadg_pil_box_resize_u8', 'oadg_pil_nearest_u8' and
'oadg_pil_pixelate_host' to that test's OWN_SUITES and 'oadg_jpeg_recompress_workspace_bytes' to its LAUNCHES_NOTHING, move the
functions below into hip_ops.py / corrupt_device.py, and delete this file.
"""
import functools

import numpy as np
import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import check, ptr, require_cuda, stream_ptr

NAMES = ('pixelate', 'jpeg_compression')
JPEG_QUALITY = (25, 18, 15, 10, 7)              # jpeg_compression's severities
PIXELATE_SCALE = (0.6, 0.5, 0.4, 0.3, 0.25)     # pixelate's severities
PRECISION_BITS = 22                             # Pillow's 8-bit resampling: 32 - 8 - 2
BOUND_COEF, BOUND_COLUMN, BOUND_SAMPLE = 1, 2, 4    # bits of oadg_jpeg_recompress_bounds_host

# ITU-T T.81 Annex K, tables K.1 and K.2, in natural (row-major) order: libjpeg's std_luminance / std_chrominance_quant_tbl
_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
       80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
       95, 98, 112, 100, 103, 99)
_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
       99, 99) + (99,) * 32


def quant_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline): uint16 [2, 64], luminance then chrominance, natural order"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError('quality must be 1 ... 100')
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_K1, _K2], np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=64)
def box_tables(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BOX filter resampling n_in -> n_out samples:
    (bounds int32 [n_out, 2] = first tap and tap count, coeffs int32 [n_out, ksize]).  Python floats are C doubles.  The
    loops run once per pair of sizes (a test split has one or two): the read-only arrays are kept."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError('height and width must be > 0')           # (Pillow's message)
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 0.5 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, coeffs = np.zeros((n_out, 2), np.int32), np.zeros((n_out, ksize), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [1.0 if -0.5 < (t + lo - center + 0.5) * ss <= 0.5 else 0.0 for t in range(hi - lo)]
        ww = sum(w)
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[i] = lo, hi - lo
        coeffs[i, :hi - lo] = [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]
    return _frozen(bounds, coeffs)


@functools.lru_cache(maxsize=64)
def nearest_table(n_in, n_out):
    """the source index of every output sample of Image.resize(NEAREST), n_in -> n_out: ImagingScaleAffine's scan, which
    ACCUMULATES its step in double (-1: the scan left the source; Pillow leaves that pixel 0)"""
    a = n_in / n_out
    xo, out = 0.5 * a, np.empty(n_out, np.int32)
    for i in range(n_out):
        xin = -1 if xo < 0.0 else int(xo)
        out[i] = xin if xin < n_in else -1
        xo += a
    return _frozen(out)


def pixelate_size(H, W, severity):
    """(oh, ow) of pixelate's small image"""
    c = PIXELATE_SCALE[severity - 1]
    return int(H * c), int(W * c)


def pixelate_tables(H, W, oh, ow):
    """xbounds, xcoeffs, ybounds, ycoeffs, ymap, xmap for H x W -> BOX -> oh x ow -> NEAREST -> H x W"""
    xb, xk = box_tables(W, ow)
    yb, yk = box_tables(H, oh)
    return xb, xk, yb, yk, nearest_table(oh, H), nearest_table(ow, W)


def _host_batch(imgs):
    imgs = np.ascontiguousarray(imgs)
    if imgs.dtype != np.uint8 or imgs.ndim != 4 or imgs.shape[3] != 3 or imgs.size == 0:
        raise TypeError('expects a non-empty uint8 [N, H, W, 3] batch')
    return imgs


def jpeg_recompress_host(imgs, quality):
    """the host twin of ``jpeg_recompress`` on a numpy uint8 [N, H, W, 3] batch -> (out, flags int32 [N]); no GPU"""
    imgs = _host_batch(imgs)
    N, H, W, _ = imgs.shape
    qt = quant_tables(quality)
    out, flags = np.empty_like(imgs), np.zeros(N, np.int32)
    check(_lib.lib().oadg_jpeg_recompress_host(imgs.ctypes.data, N, H, W, qt.ctypes.data, out.ctypes.data, flags.ctypes.data),
          'oadg_jpeg_recompress_host')
    return out, flags


def idct_bounds_host(dequantized):
    """which bounds of the saturation rule a block of 64 dequantized coefficients (column-major: element u * 8 + v =
    horizontal frequency u, vertical v) breaks: 0, or BOUND_COEF | BOUND_COLUMN | BOUND_SAMPLE bits"""
    d = np.ascontiguousarray(dequantized, np.int32)
    if d.shape != (64,):
        raise ValueError('a block holds 64 coefficients')
    return int(_lib.lib().oadg_jpeg_recompress_bounds_host(d.ctypes.data))


def pixelate_host(imgs, oh, ow):
    """the host twin of ``pixelate`` on a numpy uint8 [N, H, W, 3] batch; no GPU"""
    imgs = _host_batch(imgs)
    N, H, W, _ = imgs.shape
    xb, xk, yb, yk, ymap, xmap = pixelate_tables(H, W, oh, ow)
    out = np.empty_like(imgs)
    check(_lib.lib().oadg_pil_pixelate_host(imgs.ctypes.data, N, H, W, oh, ow, xb.ctypes.data, xk.ctypes.data, xk.shape[1],
                                            yb.ctypes.data, yk.ctypes.data, yk.shape[1], ymap.ctypes.data, xmap.ctypes.data,
                                            out.ctypes.data), 'oadg_pil_pixelate_host')
    return out


def _device_batch(x):
    require_cuda(x)
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3 or x.numel() == 0:
        raise TypeError('corrupt expects a uint8 HxWx3 image')
    return x.contiguous()


def jpeg_recompress(x, quality):
    """csrc/recompress.hip on torch's current stream: uint8 [N, H, W, 3] on the device -> (out, flags): each image as
    Image.open(Image.save(image, 'JPEG', quality=quality)) decodes it, flags int32 [N] on the device, 1 where the image has
    to be recomputed with Pillow (a block outside the saturation bounds).  Two launches; nothing is read back here."""
    x = _device_batch(x)
    N, H, W, _ = (int(v) for v in x.shape)
    L = _lib.lib()
    qt = staging.upload(quant_tables(quality), x.device)
    planes = torch.empty(max(int(L.oadg_jpeg_recompress_workspace_bytes(N, H, W)), 8), dtype=torch.uint8, device=x.device)
    out, flags = torch.empty_like(x), torch.empty(N, dtype=torch.int32, device=x.device)
    check(L.oadg_jpeg_recompress_u8(ptr(x), N, H, W, ptr(qt), ptr(planes), planes.numel(), ptr(out), ptr(flags), stream_ptr()),
          'oadg_jpeg_recompress_u8')
    return out, flags


def pixelate(x, oh, ow):
    """csrc/recompress.hip on torch's current stream: uint8 [N, H, W, 3] on the device -> each image as
    image.resize((ow, oh), BOX).resize((W, H), NEAREST).  Three launches, one upload of the tables."""
    x = _device_batch(x)
    N, H, W, _ = (int(v) for v in x.shape)
    L = _lib.lib()
    tables = pixelate_tables(H, W, oh, ow)
    xb, xk, yb, yk, ymap, xmap = staging.upload(list(tables), x.device)
    wide = torch.empty((N, H, ow, 3), dtype=torch.uint8, device=x.device)
    small = torch.empty((N, oh, ow, 3), dtype=torch.uint8, device=x.device)
    out = torch.empty_like(x)
    check(L.oadg_pil_box_resize_u8(ptr(x), ptr(wide), N, H, W, 1, ow, ptr(xb), ptr(xk), tables[1].shape[1], stream_ptr()),
          'oadg_pil_box_resize_u8')
    check(L.oadg_pil_box_resize_u8(ptr(wide), ptr(small), N, H, ow, 0, oh, ptr(yb), ptr(yk), tables[3].shape[1], stream_ptr()),
          'oadg_pil_box_resize_u8')
    check(L.oadg_pil_nearest_u8(ptr(small), ptr(out), N, oh, ow, H, W, ptr(ymap), ptr(xmap), stream_ptr()),
          'oadg_pil_nearest_u8')
    return out


def read_flags(flags):
    """the saturation flags of a batch on the host: the device route's only read"""
    return flags.cpu().numpy()


def corrupt_batch(imgs_u8, corruption_name, severity):
    """uint8 [N, H, W, 3] on the device -> (a new uint8 batch, the indices of the images the caller has to recompute on the
    host), on torch's current stream of the batch's device; None when the device declines the batch (pixelate of an image
    so small that Pillow raises: the host path raises its error).  No random number is drawn."""
    if corruption_name not in NAMES:
        raise ValueError(f'{corruption_name!r} has no device codec path')
    if not 1 <= severity <= 5:
        raise ValueError('severity must be 1 ... 5 on the device path')
    if corruption_name == 'pixelate':
        oh, ow = pixelate_size(int(imgs_u8.shape[1]), int(imgs_u8.shape[2]), severity)
        if oh < 1 or ow < 1:
            return None
    with torch.cuda.device(imgs_u8.device):
        if corruption_name == 'pixelate':
            return pixelate(imgs_u8, oh, ow), []
        out, flags = jpeg_recompress(imgs_u8, JPEG_QUALITY[severity - 1])
        return out, [int(i) for i in np.flatnonzero(read_flags(flags))]
