"""The matching of the COCO error analysis (tools/analysis_tools/coco_error_analysis.py: the plain rows at IoU 0.75 / 0.5 / 0.1
and the two "ignore confusion" rows at 0.1, four area ranges) of one test split, three ways.  Prints one JSON line.  Needs
the GPU.

usage: python tools/bench_coco_error.py [--splits cityscapes coco] [--max-dets 100] [--boxes 18] [--crowd 0.05] [--seed 0]
                                        [--host-images 500] [--repeats 5]

The input is a seeded synthetic split per entry of --splits: 'cityscapes' = 500 images, 8 classes in 2 supercategories
(Cityscapes-val size), 'coco' = 5000 images, 80 classes in 12 supercategories (COCO-val size), or IMAGESxCLASSESxSUPERS.  Per
image of 1024 x 2048 about --boxes ground-truth boxes (Poisson) of 8 .. 400 pixels a side, a fraction --crowd of them crowds,
and 0 .. --max-dets detections - jittered copies of the boxes, 70 % with the box's class and 30 % with another (the
confusion), and random boxes.  Per split:
  host        (a) evaluation.coco_error_flags_host, the literal restatement (per segment the relabelled box lists through
              ``_evaluate_img``), on the first --host-images images: pack + flags seconds
  three_launches  (b) three launches of csrc/coco_eval.hip (oadg_coco_match) on three packs, the two variant packs with every box
              of an image replicated into each of its K category segments (the detections are packed once and shared):
              pack (all three) / device (upload, kernel, download of the three) seconds, and the boxes the packs hold
  one_launch  (c) csrc/coco_error.hip: pack / upload / kernel / download seconds, and the boxes its pack holds
  equal       (a), (b) and (c) gave the same flags - checked before anything is timed; nothing is printed otherwise
The two device columns are timed --repeats times in turn; every figure is the median.
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPLITS = dict(cityscapes=(500, 8, 2), coco=(5000, 80, 12))


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
        confused = rs.uniform(size=len(src)) < 0.3
        dl = np.concatenate([np.where(confused, rs.randint(0, n_cls, len(src)), lab[src]), rs.randint(0, n_cls, nd - len(src))])
        order = np.argsort(dl, kind='stable')
        d, cuts = d[order], np.searchsorted(dl[order], np.arange(1, n_cls))
        results.append([q if len(q) else empty for q in np.split(d, cuts)])
    return gt_anns, results


def replicated_packs(pack, plain):
    """the two variant packs of column (b) in the layout of oadg_coco_match: per (image, category k) segment the boxes of the
    image that the variant shows it, in annotation order, the foreign ones as crowds (-> [sim, oth]).  ``pack``: the boxes of
    ``evaluation.pack_error_boxes``; ``plain``: the plain pack, whose detections all three launches share"""
    K, off, cat, sup = pack['num_classes'], pack['img_off'].astype(np.int64), pack['gt_cat'].astype(np.int64), pack['cat_super']
    n = len(off) - 1
    idx = np.concatenate([np.tile(np.arange(off[i], off[i + 1]), K) for i in range(n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    k = np.concatenate([np.repeat(np.arange(K), off[i + 1] - off[i]) for i in range(n)] + [np.zeros(0, np.int64)]).astype(np.int64)
    seg = np.repeat(np.arange(n), np.diff(off) * K) * K + k
    out = []
    for keep in (sup[cat[idx]] == sup[k], np.ones(len(idx), bool)):
        i, kk, s = idx[keep], k[keep], seg[keep]
        q = dict(plain)
        q.update(gts=np.ascontiguousarray(pack['gts'][i]), gt_area=np.ascontiguousarray(pack['gt_area'][i]),
                 gt_crowd=np.ascontiguousarray(((pack['gt_crowd'][i] != 0) | (cat[i] != kk)).astype(np.uint8)),
                 gt_off=np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n * K))]).astype(np.int32))
        out.append(q)
    return out


def three_launches(gt_anns, results, K, sup, thrs, sim, area_rng, dev, flags_device):
    from oadg_amd import evaluation as E
    t0 = time.perf_counter()
    plain = E.pack_coco_segments(gt_anns, results, K, E.ERROR_MAX_DET)
    packs = [plain] + replicated_packs(E.pack_error_boxes(gt_anns, K, sup), plain)       # (the detections are packed once)
    t1 = time.perf_counter()
    parts = [flags_device(q, t, area_rng, dev) for q, t in zip(packs, (thrs, [sim], [sim]))]
    flags = np.concatenate(parts, axis=1)
    t2 = time.perf_counter()
    return flags, dict(pack=t1 - t0, device=t2 - t1, seconds=t2 - t0, boxes=int(sum(len(q['gts']) for q in packs)))


def one_launch(gt_anns, results, K, sup, thrs, sim, area_rng, dev):
    from oadg_amd import evaluation as E
    steps = {}
    t0 = time.perf_counter()
    pack = E.pack_coco_error(gt_anns, results, K, sup)
    steps['pack'] = time.perf_counter() - t0
    flags = E.coco_error_flags_device(pack, thrs, sim, area_rng, dev, timings=steps)
    steps['seconds'] = time.perf_counter() - t0
    return flags, dict(steps, boxes=int(len(pack['gts'])))


def bench_split(name, a, dev):
    import torch
    import oadg_coco_match
    from oadg_amd import evaluation as E
    n_img, K, n_sup = SPLITS[name] if name in SPLITS else tuple(int(v) for v in name.split('x'))
    sup = [k * n_sup // K for k in range(K)]
    thrs, sim, area_rng = list(E.ERROR_THRS), E.ERROR_SIM_THR, E.error_area_rng((1024, 9216, 10 ** 10))
    gt_anns, results = synthetic_split(n_img, K, a.max_dets, a.boxes, a.crowd, a.seed)
    out = dict(split=name, images=n_img, classes=K, supercategories=n_sup,
               detections=int(sum(len(c) for r in results for c in r)), boxes=int(sum(len(g) for g in gt_anns)),
               segments=n_img * K, segments_with_detections=int(sum(len(c) > 0 for r in results for c in r)),
               matchings_per_segment=(len(thrs) + 2) * len(area_rng))
    # ---- all three agree, before anything is timed (this pass also loads the library and warms the launches up)
    b, _ = three_launches(gt_anns, results, K, sup, thrs, sim, area_rng, dev, oadg_coco_match.flags_device)
    c, _ = one_launch(gt_anns, results, K, sup, thrs, sim, area_rng, dev)
    assert np.array_equal(b, c), 'three launches of oadg_coco_match and the one launch of oadg_coco_error_match differ'
    h = min(n_img, a.host_images)
    t0 = time.perf_counter()
    host_pack = E.pack_coco_error(gt_anns[:h], results[:h], K, sup)
    t1 = time.perf_counter()
    host_flags = E.coco_error_flags_host(host_pack, thrs, sim, area_rng)
    t2 = time.perf_counter()
    assert np.array_equal(host_flags, c[:, :, :host_flags.shape[2]]), 'the device flags differ from the host flags'
    out['equal'] = True
    out['host'] = dict(images=h, pack=round(t1 - t0, 4), flags=round(t2 - t1, 4), seconds=round(t2 - t0, 4))
    # ---- timed: the two device columns in turn, --repeats times, the median of every figure
    runs_b, runs_c = [], []
    for _ in range(a.repeats):
        for runs, fn, extra in ((runs_b, three_launches, (oadg_coco_match.flags_device,)), (runs_c, one_launch, ())):
            gc.collect()
            torch.cuda.synchronize()
            runs.append(fn(gt_anns, results, K, sup, thrs, sim, area_rng, dev, *extra)[1])
    median = lambda runs: {k: (float(np.median([r[k] for r in runs])) if isinstance(runs[0][k], float) else runs[0][k])   # noqa: E731
                           for k in runs[0]}
    tb, tc = median(runs_b), median(runs_c)
    rnd = lambda d: {k: (round(v, 5) if isinstance(v, float) else v) for k, v in d.items()}          # noqa: E731
    out['repeats'] = a.repeats
    out['three_launches'], out['one_launch'] = rnd(tb), rnd(tc)
    out['speedup_one_launch_vs_three_launches'] = round(tb['seconds'] / tc['seconds'], 2)
    out['host_over_one_launch_per_image'] = round((t2 - t0) / h / (tc['seconds'] / n_img), 1)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--splits', nargs='+', default=['cityscapes', 'coco'], help="cityscapes | coco | IMAGESxCLASSESxSUPERS")
    p.add_argument('--max-dets', type=int, default=100)
    p.add_argument('--boxes', type=float, default=18.0)
    p.add_argument('--crowd', type=float, default=0.05)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--host-images', type=int, default=500, help='the literal host path runs on the first so many images')
    p.add_argument('--repeats', type=int, default=5, help='timed passes of the two device columns; the medians are printed')
    a = p.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    print(json.dumps(dict(metric='coco_error_analysis_matching_seconds', splits=[bench_split(s, a, dev) for s in a.splits])))


if __name__ == '__main__':
    main()
