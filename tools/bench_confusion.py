"""The two result analyses of one test split - the confusion matrix (tools/analysis_tools/confusion_matrix.py) and the
per-image mAP (tools/analysis_tools/analyze_results.py) - on the host path against the device path, end to end and step by
step.  Prints one JSON line.  Needs the GPU.

usage: python tools/bench_confusion.py [--split cityscapes_val night_sunny] [--score-thr 0.3] [--tp-iou-thr 0.5] [--seed 0]
                                       [--skip-host] [--reference-loop]

The input is the seeded synthetic split of tools/bench_voc_eval.py at two sizes: ``cityscapes_val`` (500 images of
1024 x 2048, 8 classes, about 18 boxes and 0 .. 100 detections per image) and ``night_sunny`` (26,158 images of 720 x 1280, 7
classes, about 12 boxes): jittered copies of the boxes (two per box while they last) and random boxes, random classes and
scores.  Per split:
  confusion.host.seconds       pack_confusion_segments + confusion_counts_host (one numpy IoU matrix per image), wall clock
  confusion.device.seconds     pack + confusion_counts_device (csrc/confusion.hip), wall clock, no extra synchronisation
  confusion.device.pack / upload / kernel / download    a second pass with a synchronisation after every step
  confusion.reference_loop     (--reference-loop) confusion_per_image, the reference's Python triple loop, image by image
  per_image_map.host / device  per_image_map(device=None) / (device=cuda): ten thresholds, one pack; .flags: the matching
                               alone (voc_flags_host / voc_flags_device over the ten thresholds)
  equal                        the counts and every per-image mAP are the same on both paths
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_voc_eval import synthetic_split  # noqa: E402

SPLITS = dict(cityscapes_val=dict(n_img=500, n_cls=8, max_dets=100, boxes_mean=18.0, W=2048, H=1024),
              night_sunny=dict(n_img=26158, n_cls=7, max_dets=100, boxes_mean=12.0, W=1280, H=720))


def bench_split(name, a, dev):
    import oadg_confusion
    from oadg_amd import _lib
    from oadg_amd import evaluation as E
    s = SPLITS[name]
    results, anns = synthetic_split(s['n_img'], s['n_cls'], s['max_dets'], s['boxes_mean'], 0.1, a.seed, s['W'], s['H'])
    C = s['n_cls']
    out = dict(images=s['n_img'], classes=C, detections=int(sum(len(c) for r in results for c in r)),
               boxes=int(sum(len(x['bboxes']) for x in anns)))
    # ---- confusion: device end to end, then step by step
    t0 = time.perf_counter()
    dev_cm = E.confusion_counts_device(E.pack_confusion_segments(results, anns, C, a.score_thr), a.tp_iou_thr, dev)
    conf = dict(device=dict(seconds=round(time.perf_counter() - t0, 5)))
    steps = {}
    t0 = time.perf_counter()
    pack = E.pack_confusion_segments(results, anns, C, a.score_thr)
    steps['pack'] = time.perf_counter() - t0
    assert np.array_equal(oadg_confusion.counts_device(pack, a.tp_iou_thr, dev, timings=steps), dev_cm)
    conf['device'].update({k: round(v, 5) for k, v in steps.items()})
    out['detections_over_score_thr'] = int(len(pack['dets']))
    out['counts'] = int(dev_cm.sum())
    # ---- per-image mAP: device
    t0 = time.perf_counter()
    dev_map = E.per_image_map(results, anns, C, device=dev)
    pim = dict(device=dict(seconds=round(time.perf_counter() - t0, 4)))
    vpack = E.pack_voc_segments(results, anns, C)
    thrs = [E._f32_at_least(t) for t in E.IOU_THRS]
    t0 = time.perf_counter()
    for k in range(0, len(thrs), _lib.VOC_MAX_THRS):
        E.voc_flags_device(vpack, thrs[k:k + _lib.VOC_MAX_THRS], False, dev)
    pim['device']['flags'] = round(time.perf_counter() - t0, 4)
    out['per_image_map_mean'] = float(dev_map.mean())
    if not a.skip_host:
        t0 = time.perf_counter()
        host_cm = E.confusion_counts_host(E.pack_confusion_segments(results, anns, C, a.score_thr), a.tp_iou_thr)
        conf['host'] = dict(seconds=round(time.perf_counter() - t0, 4))
        assert np.array_equal(host_cm, dev_cm), 'device counts differ from the host counts'
        if a.reference_loop:
            cm = np.zeros((C + 1, C + 1))
            t0 = time.perf_counter()
            for x, r in zip(anns, results):
                E.confusion_per_image(cm, x['bboxes'], x['labels'], r, a.score_thr, a.tp_iou_thr)
            conf['reference_loop'] = dict(seconds=round(time.perf_counter() - t0, 3))
            assert np.array_equal(cm, dev_cm)
        t0 = time.perf_counter()
        host_map = E.per_image_map(results, anns, C, device=None)
        pim['host'] = dict(seconds=round(time.perf_counter() - t0, 4))
        t0 = time.perf_counter()
        for k in range(0, len(thrs), _lib.VOC_MAX_THRS):
            E.voc_flags_host(vpack, thrs[k:k + _lib.VOC_MAX_THRS], False)
        pim['host']['flags'] = round(time.perf_counter() - t0, 4)
        assert np.array_equal(host_map, dev_map), 'per-image mAP differs between the paths'
        out['equal'] = True
        conf['speedup_end_to_end'] = round(conf['host']['seconds'] / conf['device']['seconds'], 2)
        pim['speedup_end_to_end'] = round(pim['host']['seconds'] / pim['device']['seconds'], 2)
    out['confusion'], out['per_image_map'] = conf, pim
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--split', nargs='+', default=list(SPLITS), choices=list(SPLITS))
    p.add_argument('--score-thr', type=float, default=0.3)
    p.add_argument('--tp-iou-thr', type=float, default=0.5)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--skip-host', action='store_true', help='time the device path only (no equality check)')
    p.add_argument('--reference-loop', action='store_true', help="also time confusion_per_image, the reference's loop")
    a = p.parse_args()
    import torch
    from oadg_amd import evaluation as E
    dev = torch.device('cuda', 0)
    results, anns = synthetic_split(8, 8, 20, 5.0, 0.1, 1)                               # (library load, first launches)
    E.confusion_counts_device(E.pack_confusion_segments(results, anns, 8, 0.3), 0.5, dev)
    E.per_image_map(results, anns, 8, device=dev)
    torch.cuda.synchronize()
    out = dict(metric='result_analysis_seconds', score_thr=a.score_thr, tp_iou_thr=a.tp_iou_thr)
    out.update({name: bench_split(name, a, dev) for name in a.split})
    print(json.dumps(out))


if __name__ == '__main__':
    main()
