"""The COCO bbox evaluation of one test split on the host (evaluation.coco_eval_bbox(device=None): ``_evaluate_img`` per image,
category and area range, a Python triple loop each) against the device path (csrc/coco_eval.hip: one pack, one upload, one
launch, one download, a numpy accumulate), end to end and step by step.  Prints one JSON line.  Needs the GPU.

usage: python tools/bench_coco_eval.py [--images 500] [--classes 8] [--max-dets 100] [--boxes 18] [--crowd 0.05] [--seed 0]
                                       [--mmdet] [--skip-host]

The input is a seeded synthetic split of Cityscapes-val size (--images 5000 --classes 80: a COCO-sized one): per image of
1024 x 2048 about --boxes ground-truth boxes (Poisson) of 8 .. 400 pixels a side, a fraction --crowd of them crowds, mask-like
``area`` fields, and 0 .. --max-dets detections - jittered copies of the boxes (two per box while they last, so detections
contest boxes) and random boxes - with random classes and scores.
  segments                     images x classes: one workgroup each on the device
  host.seconds                 coco_eval_bbox(device=None), wall clock
  device.seconds               coco_eval_bbox(device=cuda), wall clock, as Dataset.evaluate runs it (no extra synchronisation)
  device.pack / upload / kernel / download / accumulate   a second pass with a synchronisation after every step
  equal                        the flags of every (area range, threshold, detection) and all twelve numbers are the same on
                               both paths (the flags through evaluation.coco_flags_host)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_split(n_img, n_cls, max_dets, boxes_mean, crowd, seed, W=2048, H=1024):
    """(gt_anns, results) in the formats of evaluation.dataset_gt_anns and single_gpu_test"""
    rs = np.random.RandomState(seed)
    gt_anns, results = [], []
    empty = np.zeros((0, 5), np.float32)
    for _ in range(n_img):
        n = rs.poisson(boxes_mean)
        xy = rs.uniform(0, [W - 60, H - 60], (n, 2))
        wh = np.exp(rs.uniform(np.log(8), np.log(400), (n, 2)))
        lab = rs.randint(0, n_cls, n)
        is_crowd = rs.uniform(size=n) < crowd
        area = wh[:, 0] * wh[:, 1] * rs.uniform(0.4, 1.0, n)
        gt_anns.append([dict(bbox=[float(v) for v in (*xy[j], *wh[j])], category=int(lab[j]), area=float(area[j]),
                             iscrowd=int(is_crowd[j])) for j in range(n)])
        nd = rs.randint(0, max_dets + 1)
        src = np.concatenate([np.arange(n), np.arange(n)])[:nd]
        hit = np.concatenate([xy[src], xy[src] + wh[src]], 1) + rs.uniform(-8, 8, (len(src), 4))
        p = rs.uniform(0, [W - 60, H - 60], (nd - len(src), 2))
        miss = np.concatenate([p, p + np.exp(rs.uniform(np.log(8), np.log(400), (len(p), 2)))], 1)
        d = np.concatenate([np.concatenate([hit, miss]), rs.uniform(0.05, 1, (nd, 1))], 1).astype(np.float32)
        dl = np.concatenate([lab[src], rs.randint(0, n_cls, nd - len(src))])
        order = np.argsort(dl, kind='stable')
        d, cuts = d[order], np.searchsorted(dl[order], np.arange(1, n_cls))
        results.append([q if len(q) else empty for q in np.split(d, cuts)])
    return gt_anns, results


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=500)
    p.add_argument('--classes', type=int, default=8)
    p.add_argument('--max-dets', type=int, default=100)
    p.add_argument('--boxes', type=float, default=18.0)
    p.add_argument('--crowd', type=float, default=0.05)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--mmdet', action='store_true', help='maxDets (100, 300, 1000) as CocoDataset.evaluate, not (1, 10, 100)')
    p.add_argument('--skip-host', action='store_true', help='time the device path only (no equality check)')
    a = p.parse_args()
    import torch
    import oadg_coco_match
    from oadg_amd import evaluation as E
    dev = torch.device('cuda', 0)
    gt_anns, results = synthetic_split(a.images, a.classes, a.max_dets, a.boxes, a.crowd, a.seed)
    K = a.classes
    max_dets = list(E.MMDET_MAX_DETS) if a.mmdet else [1, 10, 100]
    E.coco_eval_bbox(gt_anns[:8], results[:8], K, max_dets=max_dets, device=dev)           # (library load, first launch)
    torch.cuda.synchronize()
    out = dict(metric='coco_bbox_eval_seconds', images=a.images, classes=K, max_dets=max_dets,
               detections=int(sum(len(c) for r in results for c in r)), boxes=int(sum(len(g) for g in gt_anns)),
               segments=a.images * K, segments_with_detections=int(sum(len(c) > 0 for r in results for c in r)),
               matchings_per_segment=len(E.IOU_THRS) * len(E.AREA_RNG))
    # ---- device, end to end
    t0 = time.perf_counter()
    dev_res = E.coco_eval_bbox(gt_anns, results, K, max_dets=max_dets, device=dev)
    dev_s = time.perf_counter() - t0
    # ---- device, step by step
    steps = {}
    t0 = time.perf_counter()
    pack = E.pack_coco_segments(gt_anns, results, K, max_dets[-1])
    steps['pack'] = time.perf_counter() - t0
    flags_dev = oadg_coco_match.flags_device(pack, E.IOU_THRS, E.AREA_RNG, dev, timings=steps)
    t0 = time.perf_counter()
    acc = E.coco_summarize(*E.coco_accumulate(pack, flags_dev, max_dets))
    steps['accumulate'] = time.perf_counter() - t0
    out['device'] = dict(seconds=round(dev_s, 4), **{k: round(v, 5) for k, v in steps.items()})
    out['stats'] = dev_res
    assert acc == dev_res
    # ---- host
    if not a.skip_host:
        t0 = time.perf_counter()
        host_res = E.coco_eval_bbox(gt_anns, results, K, max_dets=max_dets)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        flags_host = E.coco_flags_host(pack)
        out['host'] = dict(seconds=round(host_s, 4), flags=round(time.perf_counter() - t0, 4))
        assert np.array_equal(flags_host, flags_dev), 'device flags differ from the host flags'
        assert host_res == dev_res, (host_res, dev_res)
        out['equal'] = True
        out['speedup_end_to_end'] = round(host_s / dev_s, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
