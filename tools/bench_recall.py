"""The proposal recall of one test split on the host (evaluation.eval_recalls(device=None): per image and budget G rounds of
an argmax over a G x P IoU matrix, the reference's ``_recalls`` restated) against the device path (csrc/recall.hip: one pack,
one upload, one launch for all images and budgets, one download, a numpy sort and count), end to end and step by step.
Prints one JSON line.  Needs the GPU.

usage: python tools/bench_recall.py [--images 500] [--proposals 1000] [--boxes 18] [--seed 0] [--legacy] [--skip-host]

The input is a seeded synthetic split of Cityscapes-val size: per image of 1024 x 2048 about --boxes ground-truth boxes
(Poisson) of 8 .. 400 pixels a side and --proposals scored proposals - jittered copies of the boxes (four per box, from
tight to loose) among random boxes; the coordinates of every other image are rounded, so equal IoUs occur.  Budgets
(100, 300, 1000), thresholds .5 ... .95: what ``CocoDataset.evaluate(metric='proposal_fast')`` asks for.
  host.seconds                 eval_recalls(device=None), wall clock
  device.seconds               eval_recalls(device=cuda), wall clock, as proposal_evaluate runs it (no extra synchronisation)
  device.pack / upload / kernel / download / accumulate   a second pass with a synchronisation after every step
  equal                        the matched IoU of every (budget, image, round) and all recalls are the same on both paths
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NUMS = (100, 300, 1000)


def synthetic_split(n_img, n_prop, boxes_mean, seed, W=2048, H=1024):
    """(gts, proposals): per image fp32 [g, 4] and fp32 [n_prop, 5]"""
    rs = np.random.RandomState(seed)
    gts, props = [], []
    for i in range(n_img):
        n = rs.poisson(boxes_mean)
        xy = rs.uniform(0, [W - 60, H - 60], (n, 2))
        wh = np.exp(rs.uniform(np.log(8), np.log(400), (n, 2)))
        g = np.concatenate([xy, xy + wh], 1)
        near = [g + rs.uniform(-s, s, g.shape) for s in (2, 6, 15, 40)]
        p = rs.uniform(0, [W - 60, H - 60], (n_prop, 2))
        far = np.concatenate([p, p + np.exp(rs.uniform(np.log(8), np.log(400), (n_prop, 2)))], 1)
        d = np.concatenate(near + [far])
        d = d[rs.permutation(len(d))[:n_prop]]
        if i % 2 == 0:
            g, d = np.round(g), np.round(d)
        gts.append(g.astype(np.float32))
        props.append(np.concatenate([d, rs.uniform(0.05, 1, (len(d), 1))], 1).astype(np.float32))
    return gts, props


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=500)
    p.add_argument('--proposals', type=int, default=1000)
    p.add_argument('--boxes', type=float, default=18.0)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--legacy', action='store_true', help='the "+ 1" extents of the VOC-style datasets')
    p.add_argument('--skip-host', action='store_true', help='time the device path only (no equality check)')
    a = p.parse_args()
    import torch
    from oadg_amd import evaluation as E
    dev = torch.device('cuda', 0)
    gts, props = synthetic_split(a.images, a.proposals, a.boxes, a.seed)
    thrs = E.IOU_THRS
    E.eval_recalls(gts[:8], props[:8], NUMS, thrs, logger='silent', use_legacy_coordinate=a.legacy, device=dev)
    torch.cuda.synchronize()                                                           # (library load, first launch)
    out = dict(metric='proposal_recall_seconds', images=a.images, proposals=int(sum(len(q) for q in props)),
               boxes=int(sum(len(g) for g in gts)), nums=list(NUMS), thresholds=len(thrs), legacy=bool(a.legacy),
               workgroups=a.images * len(NUMS))
    # ---- device, end to end
    t0 = time.perf_counter()
    dev_res = E.eval_recalls(gts, props, NUMS, thrs, logger='silent', use_legacy_coordinate=a.legacy, device=dev)
    dev_s = time.perf_counter() - t0
    # ---- device, step by step
    steps = {}
    t0 = time.perf_counter()
    pack = E.pack_recall(gts, props, NUMS)
    steps['pack'] = time.perf_counter() - t0
    ious_dev = E.recall_ious_device(pack, a.legacy, dev, timings=steps)
    t0 = time.perf_counter()
    acc = E.recalls_from_ious(ious_dev, thrs)
    steps['accumulate'] = time.perf_counter() - t0
    out['device'] = dict(seconds=round(dev_s, 4), **{k: round(v, 5) for k, v in steps.items()})
    out['AR'] = {f'AR@{n}': float(v) for n, v in zip(NUMS, dev_res.mean(axis=1))}
    assert np.array_equal(acc, dev_res)
    # ---- host
    if not a.skip_host:
        t0 = time.perf_counter()
        host_res = E.eval_recalls(gts, props, NUMS, thrs, logger='silent', use_legacy_coordinate=a.legacy)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        ious_host = E.recall_ious_host(pack, a.legacy)
        out['host'] = dict(seconds=round(host_s, 4), ious=round(time.perf_counter() - t0, 4))
        assert np.array_equal(ious_host, ious_dev), 'device IoUs differ from the host IoUs'
        assert np.array_equal(host_res, dev_res), (host_res, dev_res)
        out['equal'] = True
        out['speedup_end_to_end'] = round(host_s / dev_s, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
