"""The device half of the COCO bbox evaluation: the ctypes call of ``oadg_coco_match`` (csrc/coco_eval.hip) and the upload /
launch / download around it.  ``oadg_amd.evaluation.coco_flags_device`` imports this module and calls ``flags_device``, so
``coco_eval_bbox(device=...)``, ``CocoDataset.evaluate`` and ``EvalHook`` need nothing but the package, the library and a GPU.

WHERE THIS BELONGS: ``coco_match`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py.  It is here, next to the
package's import shim, for the reason oadg_voc_tpfp.py and oadg_draw.py give: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and the
change that added this kernel could add test files but not edit that one.  The suite that answers for this call site is
tests/test_hip_coco_eval.py.  The follow-up is mechanical: add 'oadg_coco_match' to that test's OWN_SUITES and
'oadg_coco_match_workspace_bytes' to its LAUNCHES_NOTHING, move the two functions below into hip_ops.py / evaluation.py, and
delete this file.
"""
import ctypes
import time

import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import check, ptr, require_cuda, stream_ptr

# the kernel's capacities (include/oadg_hip.h): matchings (thresholds x area ranges) of one call; boxes of a segment that are
# staged once - a larger segment walks its boxes in chunks of that size and keeps its "taken" words in the workspace -; the
# detections that pass through LDS at a time
MAX_LANES, LDS_GTS, LDS_DETS = _lib.COCO_MAX_LANES, _lib.COCO_LDS_GTS, _lib.COCO_LDS_DETS
KEYS = ('dets', 'det_off', 'gts', 'gt_area', 'gt_crowd', 'gt_off')


def _dense(t, dtype, what):
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f'{what} must be a contiguous {dtype} tensor')


def coco_match(dets, det_off, gts, gt_area, gt_crowd, gt_off, thrs, area_rng, out=None, want_match=False, workspace=None):
    """csrc/coco_eval.hip on torch's current stream: the COCO-protocol greedy matching of every (image, category) segment of
    a split, for all of ``thrs`` (already min(t, 1 - 1e-10)) and all of ``area_rng`` ([lo, hi] pairs), in one launch;
    len(thrs) * len(area_rng) <= MAX_LANES.

    dets fp64 [D, 4] = x, y, w, h (per segment by descending score, cut to the largest maxDets), det_off int32 [S + 1], gts
    fp64 [G, 4] (annotation order), gt_area fp64 [G], gt_crowd uint8 [G], gt_off int32 [S + 1].  Returns (flags uint8
    [n_area, n_thr, D]: 0 false positive, 1 true positive, 2 ignored; match int32 [n_area, n_thr, D], the matched box within
    the segment or -1 - None unless ``want_match``).  ``out``: (flags, match or None) to write into; ``workspace``: a uint8
    tensor to use instead of a fresh one."""
    require_cuda(dets, det_off, gts, gt_area, gt_crowd, gt_off)
    _dense(dets, torch.float64, 'dets')
    _dense(gts, torch.float64, 'gts')
    _dense(gt_area, torch.float64, 'gt_area')
    _dense(gt_crowd, torch.uint8, 'gt_crowd')
    for t in (det_off, gt_off):
        _dense(t, torch.int32, 'det_off / gt_off')
    if dets.dim() != 2 or dets.shape[1] != 4 or gts.dim() != 2 or gts.shape[1] != 4:
        raise ValueError('dets must be [D, 4] and gts [G, 4]')
    D, G, S = dets.shape[0], gts.shape[0], det_off.numel() - 1
    if S < 0 or gt_off.numel() != S + 1 or gt_area.numel() != G or gt_crowd.numel() != G:
        raise ValueError('det_off and gt_off hold S + 1 entries, gt_area and gt_crowd one per box')
    thrs = [float(t) for t in thrs]
    area_rng = [tuple(r) for r in area_rng]
    if any(len(r) != 2 for r in area_rng):
        raise ValueError('area_rng holds [lo, hi] pairs')
    rng = [float(v) for r in area_rng for v in r]
    T, A = len(thrs), len(area_rng)
    if T < 1 or A < 1 or T * A > MAX_LANES:
        raise ValueError(f'thresholds x area ranges: 1 to {MAX_LANES} matchings per call (got {T} x {A})')
    if out is None:
        out = (torch.empty((A, T, D), dtype=torch.uint8, device=dets.device),
               torch.empty((A, T, D), dtype=torch.int32, device=dets.device) if want_match else None)
    flags, match = out
    require_cuda(flags, match)
    _dense(flags, torch.uint8, 'flags')
    if match is not None:
        _dense(match, torch.int32, 'match')
    if tuple(flags.shape) != (A, T, D) or (match is not None and tuple(match.shape) != (A, T, D)):
        raise ValueError('flags and match must be [n_area, n_thr, D]')
    L = _lib.lib()
    if workspace is None:
        workspace = torch.empty(max(int(L.oadg_coco_match_workspace_bytes(S, D, G, T, A)), 8), dtype=torch.uint8,
                                device=dets.device)
    require_cuda(workspace)
    check(L.oadg_coco_match(ptr(dets), ptr(det_off), ptr(gts), ptr(gt_area), ptr(gt_crowd), ptr(gt_off), S, D, G,
                            (ctypes.c_double * T)(*thrs), T, (ctypes.c_double * (2 * A))(*rng), A, ptr(flags), ptr(match),
                            ptr(workspace), workspace.numel(), stream_ptr()), 'oadg_coco_match')
    return flags, match


def flags_device(pack, thrs, area_rng, device, timings=None, want_match=False):
    """the flags of ``evaluation.coco_flags_host`` from the device: one upload of the pack through the staging path, ONE
    launch for the split, all thresholds and all area ranges, one download -> uint8 [n_area, n_thr, D] (with ``want_match``:
    the pair (flags, match)).  ``thrs``: the protocol's thresholds; they are capped at 1 - 1e-10 here, as the host caps them.
    ``timings``: a dict that receives upload / kernel / download seconds (each step synchronised: for
    tools/bench_coco_eval.py only)."""
    dev = torch.device(device)
    capped = [min(float(t), 1 - 1e-10) for t in thrs]
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        up = staging.upload([pack[k] for k in KEYS], dev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
        flags, match = coco_match(*up, capped, area_rng, want_match=want_match)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
        back = [staging.readback(t) for t in ((flags, match) if want_match else (flags,))]
        out = [b.wait().numpy() for b in back]
    if timings is not None:
        timings.update(upload=t1 - t0, kernel=t2 - t1, download=time.perf_counter() - t2)
    return tuple(out) if want_match else out[0]
