"""The device half of the VOC evaluation: the ctypes call of ``oadg_voc_tpfp`` (csrc/voc_eval.hip) and the upload /
launch / download around it.  ``oadg_amd.evaluation.voc_flags_device`` imports this module and calls ``flags_device``, so
``eval_map_voc(device=...)`` and ``SdgodDataset.evaluate`` need nothing but the package, the library and a GPU.

WHERE THIS BELONGS: ``voc_tpfp`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py.  It is here, next to the
package's import shim, for one reason: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and the
change that added this kernel could add test files but not edit that one.  The suite that answers for this call site is
tests/test_hip_voc_eval.py.  The follow-up is mechanical: add 'oadg_voc_tpfp' to that test's OWN_SUITES and
'oadg_voc_tpfp_workspace_bytes' to its LAUNCHES_NOTHING, move the two functions below into hip_ops.py / evaluation.py, and
delete this file.
"""
import ctypes
import time

import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import check, ptr, require_cuda, stream_ptr


def _dense(t, dtype, what):
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f'{what} must be a contiguous {dtype} tensor')


def voc_tpfp(dets, det_off, gts, gt_off, gt_reg, iou_thrs, legacy, out=None, workspace=None):
    """csrc/voc_eval.hip on torch's current stream: the VOC-protocol matching of every (image, class) segment of a split,
    for all of ``iou_thrs`` (at most _lib.VOC_MAX_THRS floats), in one launch.

    dets fp32 [D, 5], det_off int32 [S + 1], gts fp32 [G, 4] (per segment: regular boxes, then ignored ones), gt_off int32
    [S + 1], gt_reg int32 [S].  Returns (iou_max fp32 [D], iou_arg int32 [D], flags uint8 [n_thr, D]: 0 ignored, 1 tp, 2 fp);
    ``out``: those three tensors to write into; ``workspace``: a uint8 tensor to use instead of a fresh one."""
    require_cuda(dets, det_off, gts, gt_off, gt_reg)
    _dense(dets, torch.float32, 'dets')
    _dense(gts, torch.float32, 'gts')
    for t in (det_off, gt_off, gt_reg):
        _dense(t, torch.int32, 'det_off / gt_off / gt_reg')
    D, G, S = dets.shape[0], gts.shape[0], gt_reg.numel()
    if dets.dim() != 2 or dets.shape[1] != 5 or gts.dim() != 2 or gts.shape[1] != 4:
        raise ValueError('dets must be [D, 5] and gts [G, 4]')
    if det_off.numel() != S + 1 or gt_off.numel() != S + 1:
        raise ValueError('det_off and gt_off hold one entry more than gt_reg')
    thrs = [float(t) for t in iou_thrs]
    if not 1 <= len(thrs) <= _lib.VOC_MAX_THRS:
        raise ValueError(f'1 to {_lib.VOC_MAX_THRS} thresholds per call')
    if out is None:
        out = (torch.empty(D, dtype=torch.float32, device=dets.device), torch.empty(D, dtype=torch.int32, device=dets.device),
               torch.empty((len(thrs), D), dtype=torch.uint8, device=dets.device))
    iou_max, iou_arg, flags = out
    require_cuda(iou_max, iou_arg, flags)
    _dense(iou_max, torch.float32, 'iou_max')
    _dense(iou_arg, torch.int32, 'iou_arg')
    _dense(flags, torch.uint8, 'flags')
    if iou_max.numel() != D or iou_arg.numel() != D or tuple(flags.shape) != (len(thrs), D):
        raise ValueError('iou_max, iou_arg must hold D elements and flags [n_thr, D]')
    L = _lib.lib()
    if workspace is None:
        workspace = torch.empty(max(int(L.oadg_voc_tpfp_workspace_bytes(S, D, G, len(thrs))), 8), dtype=torch.uint8,
                                device=dets.device)
    check(L.oadg_voc_tpfp(ptr(dets), ptr(det_off), ptr(gts), ptr(gt_off), ptr(gt_reg), S, D, G,
                          (ctypes.c_float * len(thrs))(*thrs), len(thrs), int(bool(legacy)), ptr(iou_max), ptr(iou_arg),
                          ptr(flags), ptr(workspace), workspace.numel(), stream_ptr()), 'oadg_voc_tpfp')
    return iou_max, iou_arg, flags


def flags_device(pack, iou_thrs, use_legacy_coordinate, device, timings=None):
    """the flags of ``evaluation.voc_flags_host`` from the device: one upload of the pack through the staging path, ONE
    launch for the split and all thresholds, one download -> uint8 [n_thr, D].  ``timings``: a dict that receives upload /
    kernel / download seconds (each step synchronised: for tools/bench_voc_eval.py only)."""
    dev = torch.device(device)
    keys = ('dets', 'det_off', 'gts', 'gt_off', 'gt_reg')
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        up = staging.upload([pack[k] for k in keys], dev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
        _, _, flags = voc_tpfp(*up, iou_thrs, use_legacy_coordinate)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
        out = staging.readback(flags).wait().numpy()
    if timings is not None:
        timings.update(upload=t1 - t0, kernel=t2 - t1, download=time.perf_counter() - t2)
    return out

