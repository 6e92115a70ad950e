"""The device half of the COCO error analysis: the ctypes call of ``oadg_coco_error_match`` (csrc/coco_error.hip) and the upload /
launch / download around it.  ``oadg_amd.evaluation.coco_error_flags_device`` imports this module and calls ``flags_device``, so
``coco_error_analysis(device=...)`` and tools/analysis_tools/coco_error_analysis.py need nothing but the package, the library and
a GPU.

WHERE THIS BELONGS: ``coco_error_match`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py.  It is here, next to the
package's import shim, as oadg_coco_match.py is: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and this one
is not on its lists.  The suite that answers for this call site is tests/test_hip_coco_error.py.  The follow-up is mechanical: add 'oadg_coco_error_match' to that test's OWN_SUITES and
'oadg_coco_error_workspace_bytes' to its LAUNCHES_NOTHING, move the two functions below into hip_ops.py / evaluation.py, and
delete this file.
"""
import ctypes
import time

import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import check, ptr, require_cuda, stream_ptr

# the kernel's capacities (include/oadg_hip.h): matchings ((thresholds + 2) x area ranges) of one call; boxes of an IMAGE that
# are staged once - a larger image walks its boxes in chunks of that size and keeps its "taken" words in the workspace -; the
# detections that pass through LDS at a time
MAX_LANES, LDS_GTS, LDS_DETS = _lib.COCO_MAX_LANES, _lib.COCO_ERROR_LDS_GTS, _lib.COCO_ERROR_LDS_DETS
KEYS = ('dets', 'det_off', 'gts', 'gt_area', 'gt_crowd', 'gt_cat', 'img_off', 'cat_super')
DTYPES = (torch.float64, torch.int32, torch.float64, torch.float64, torch.uint8, torch.int32, torch.int32, torch.int32)


def coco_error_match(dets, det_off, gts, gt_area, gt_crowd, gt_cat, img_off, cat_super, thrs, sim_thr, area_rng, out=None,
                     workspace=None):
    """csrc/coco_error.hip on torch's current stream: for every (image, category) segment of a split the plain COCO matchings at
    ``thrs`` and the two "ignore confusion" matchings at ``sim_thr`` (thresholds already min(t, 1 - 1e-10)), for all of
    ``area_rng`` ([lo, hi] pairs), in one launch; (len(thrs) + 2) * len(area_rng) <= MAX_LANES.

    dets fp64 [D, 4] = x, y, w, h (per segment by descending score, cut to maxDets), det_off int32 [n_img * K + 1], gts fp64
    [G, 4] (every box of an image once, annotation order), gt_area fp64 [G], gt_crowd uint8 [G], gt_cat int32 [G], img_off
    int32 [n_img + 1], cat_super int32 [K].  Returns flags uint8 [n_area, len(thrs) + 2, D]: 0 false positive, 1 true
    positive, 2 ignored.  ``out``: the tensor to write into; ``workspace``: a uint8 tensor to use instead of a fresh one."""
    tensors = (dets, det_off, gts, gt_area, gt_crowd, gt_cat, img_off, cat_super)
    require_cuda(*tensors)
    for t, dtype, what in zip(tensors, DTYPES, KEYS):
        if t.dtype != dtype or not t.is_contiguous():
            raise ValueError(f'{what} must be a contiguous {dtype} tensor')
    if dets.dim() != 2 or dets.shape[1] != 4 or gts.dim() != 2 or gts.shape[1] != 4:
        raise ValueError('dets must be [D, 4] and gts [G, 4]')
    D, G, N, K = dets.shape[0], gts.shape[0], img_off.numel() - 1, cat_super.numel()
    if N < 0 or K < 1 or det_off.numel() != N * K + 1 or gt_area.numel() != G or gt_crowd.numel() != G or gt_cat.numel() != G:
        raise ValueError('det_off holds n_img * K + 1 entries, img_off n_img + 1, gt_area, gt_crowd and gt_cat one per box')
    thrs = [float(t) for t in thrs]
    area_rng = [tuple(r) for r in area_rng]
    if any(len(r) != 2 for r in area_rng):
        raise ValueError('area_rng holds [lo, hi] pairs')
    rng = [float(v) for r in area_rng for v in r]
    T, A = len(thrs), len(area_rng)
    if out is None:
        out = torch.empty((A, T + 2, D), dtype=torch.uint8, device=dets.device)
    require_cuda(out)
    if out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != (A, T + 2, D):
        raise ValueError('flags must be a contiguous uint8 tensor [n_area, n_thr + 2, D]')
    L = _lib.lib()
    if workspace is None:
        workspace = torch.empty(max(int(L.oadg_coco_error_workspace_bytes(N, K, D, G, T, A)), 8), dtype=torch.uint8,
                                device=dets.device)
    require_cuda(workspace)
    check(L.oadg_coco_error_match(ptr(dets), ptr(det_off), ptr(gts), ptr(gt_area), ptr(gt_crowd), ptr(gt_cat), ptr(img_off),
                                  ptr(cat_super), N, K, D, G, (ctypes.c_double * max(T, 1))(*thrs), T, float(sim_thr),
                                  (ctypes.c_double * max(2 * A, 1))(*rng), A, ptr(out), ptr(workspace), workspace.numel(),
                                  stream_ptr()), 'oadg_coco_error_match')
    return out


def flags_device(pack, thrs, sim_thr, area_rng, device, timings=None):
    """the flags of ``evaluation.coco_error_flags_host`` from the device: one upload of the pack (``evaluation.pack_coco_error``)
    through the staging path, ONE launch for the split, all rows and all area ranges, one download -> uint8 [n_area, n_thr + 2,
    D].  The thresholds are capped at 1 - 1e-10 here, as the host caps them.  ``timings``: a dict that receives upload / kernel /
    download seconds (each step synchronised: for tools/bench_coco_error.py only)."""
    dev = torch.device(device)
    capped = [min(float(t), 1 - 1e-10) for t in thrs]
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        up = staging.upload([pack[k] for k in KEYS], dev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
        flags = coco_error_match(*up, capped, min(float(sim_thr), 1 - 1e-10), area_rng)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
        out = staging.readback(flags).wait().numpy()
    if timings is not None:
        timings.update(upload=t1 - t0, kernel=t2 - t1, download=time.perf_counter() - t2)
    return out
