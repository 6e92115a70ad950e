"""The VOC07 evaluation of one Diverse-Weather split on the host (evaluation.eval_map_voc(device=None): the reference's
per-(image, class) numpy problems, one after the other) against the device path (csrc/voc_eval.hip: one pack, one upload,
one launch, one download), end to end and step by step.  Prints one JSON line.  Needs the GPU.

usage: python tools/bench_voc_eval.py [--images 26158] [--classes 7] [--max-dets 100] [--boxes 12] [--difficult 0.1]
                                      [--thrs 0.5] [--seed 0] [--skip-host]

The input is a seeded synthetic split of night-sunny size: per image about --boxes ground-truth boxes (Poisson), a fraction
--difficult of them ignored, and 0 .. --max-dets detections - jittered copies of the boxes (two per box while they last, so
detections contest boxes) and random boxes - with random classes and scores.
  segments                     images x classes: one workgroup each on the device; segments_with_detections: the numpy
                               problems the host path solves (a segment without detections costs it nothing)
  host.seconds                 eval_map_voc(device=None), wall clock
  host.pack / flags / accumulate   a second host pass, each step measured on its own
  device.seconds               eval_map_voc(device=cuda), wall clock, as SdgodDataset.evaluate runs it (no extra synchronisation)
  device.pack / upload / kernel / download / accumulate   a second pass with a synchronisation after every step
  equal                        the flags of every detection, every per-class AP and the mean are the same on both paths
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_split(n_img, n_cls, max_dets, boxes_mean, difficult, seed, W=1280, H=720):
    """(results, annotations) in the formats of single_gpu_test and get_ann_info"""
    rs = np.random.RandomState(seed)
    anns, results = [], []
    empty = np.zeros((0, 5), np.float32)
    for _ in range(n_img):
        n = rs.poisson(boxes_mean)
        x1, y1 = rs.uniform(0, W - 60, n), rs.uniform(0, H - 60, n)
        b = np.round(np.stack([x1, y1, x1 + rs.uniform(10, 300, n), y1 + rs.uniform(10, 200, n)], 1)).astype(np.float32)
        lab = rs.randint(0, n_cls, n)
        hard = rs.uniform(size=n) < difficult
        anns.append(dict(bboxes=b[~hard], labels=lab[~hard].astype(np.int64), bboxes_ignore=b[hard],
                         labels_ignore=lab[hard].astype(np.int64)))
        nd = rs.randint(0, max_dets + 1)
        src = np.concatenate([np.arange(n), np.arange(n)])[:nd]
        d = np.concatenate([b[src] + rs.uniform(-8, 8, (len(src), 4)),
                            np.abs(rs.uniform(0, 1, (nd - len(src), 4)) * [W, H, W, H])]).astype(np.float32)
        d[len(src):, 2:] = d[len(src):, :2] + np.abs(rs.uniform(10, 200, (nd - len(src), 2))).astype(np.float32)
        dl = np.concatenate([lab[src], rs.randint(0, n_cls, nd - len(src))])
        d = np.concatenate([d, rs.uniform(0.05, 1, (nd, 1)).astype(np.float32)], 1)
        order = np.argsort(dl, kind='stable')
        d, cuts = d[order], np.searchsorted(dl[order], np.arange(1, n_cls))
        results.append([p if len(p) else empty for p in np.split(d, cuts)])
    return results, anns


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--images', type=int, default=26158)
    p.add_argument('--classes', type=int, default=7)
    p.add_argument('--max-dets', type=int, default=100)
    p.add_argument('--boxes', type=float, default=12.0)
    p.add_argument('--difficult', type=float, default=0.1)
    p.add_argument('--thrs', type=float, nargs='+', default=[0.5])
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--skip-host', action='store_true', help='time the device path only (no equality check)')
    a = p.parse_args()
    import torch
    import oadg_voc_tpfp
    from oadg_amd import evaluation as E
    dev = torch.device('cuda', 0)
    results, anns = synthetic_split(a.images, a.classes, a.max_dets, a.boxes, a.difficult, a.seed)
    C, thrs = a.classes, [float(t) for t in a.thrs]
    E.eval_map_voc_thrs(results[:8], anns[:8], C, thrs, 'voc07', True, dev)          # (library load, first launch)
    torch.cuda.synchronize()
    out = dict(metric='voc07_eval_seconds', images=a.images, classes=C, thresholds=thrs,
               detections=int(sum(len(c) for r in results for c in r)),
               boxes=int(sum(len(x['bboxes']) + len(x['bboxes_ignore']) for x in anns)),
               segments=a.images * C, segments_with_detections=int(sum(len(c) > 0 for r in results for c in r)))
    # ---- device, end to end
    t0 = time.perf_counter()
    dev_res = E.eval_map_voc_thrs(results, anns, C, thrs, 'voc07', True, dev)
    dev_s = time.perf_counter() - t0
    # ---- device, step by step
    steps = {}
    t0 = time.perf_counter()
    pack = E.pack_voc_segments(results, anns, C)
    steps['pack'] = time.perf_counter() - t0
    flags_dev = oadg_voc_tpfp.flags_device(pack, thrs, True, dev, timings=steps)
    t0 = time.perf_counter()
    acc = [E.voc_accumulate(pack, flags_dev[t], 'voc07') for t in range(len(thrs))]
    steps['accumulate'] = time.perf_counter() - t0
    out['device'] = dict(seconds=round(dev_s, 4), **{k: round(v, 5) for k, v in steps.items()})
    out['mean_ap'] = [m for m, _ in dev_res]
    assert [m for m, _ in acc] == out['mean_ap']
    # ---- host
    if not a.skip_host:
        t0 = time.perf_counter()
        host_res = E.eval_map_voc_thrs(results, anns, C, thrs, 'voc07', True, None)
        host_s = time.perf_counter() - t0
        host = {}                                            # (a second pass, step by step, every step measured here)
        t0 = time.perf_counter()
        pack_h = E.pack_voc_segments(results, anns, C)
        host['pack'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        flags_host = E.voc_flags_host(pack_h, thrs, True)
        host['flags'] = time.perf_counter() - t0
        t0 = time.perf_counter()
        [E.voc_accumulate(pack_h, flags_host[t], 'voc07') for t in range(len(thrs))]
        host['accumulate'] = time.perf_counter() - t0
        out['host'] = dict(seconds=round(host_s, 4), **{k: round(v, 5) for k, v in host.items()})
        assert np.array_equal(flags_host, flags_dev), 'device flags differ from the host flags'
        for (mh, ph), (md, pd) in zip(host_res, dev_res):
            assert mh == md and [r['ap'] for r in ph] == [r['ap'] for r in pd], (mh, md)
        out['equal'] = True
        out['speedup_end_to_end'] = round(host_s / dev_s, 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
