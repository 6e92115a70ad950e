"""Inputs of the COCO evaluation suites (tests/test_coco_eval_pack.py on the CPU, tests/test_hip_coco_eval.py on the GPU): a
seeded split in the formats of ``coco_eval_bbox``, and packs built segment by segment."""
import numpy as np

from oadg_amd import evaluation as E


def seeded_split(seed=0, n_img=30, n_cls=5, W=640, H=384):
    """(gt_anns, results): per image about 12 boxes of 6 .. 260 pixels a side (every area range occurs), about 15 % crowds,
    ``area`` fields that are NOT w * h, one image without ground truth and one without detections; per (image, class) 0 .. 30
    detections - jittered copies of the boxes, two per box while they last, and random boxes - with one-decimal scores (ties)"""
    rs = np.random.RandomState(seed)
    gt_anns, results = [], []
    for i in range(n_img):
        n = 0 if i == 3 else rs.poisson(12)
        xy = rs.uniform(0, [W - 40, H - 40], (n, 2))
        wh = np.exp(rs.uniform(np.log(6), np.log(260), (n, 2)))
        cat = rs.randint(0, n_cls, n)
        crowd = rs.uniform(size=n) < 0.15
        area = wh[:, 0] * wh[:, 1] * rs.uniform(0.4, 1.0, n)                  # (a mask's area: less than the box's)
        gt_anns.append([dict(bbox=[float(v) for v in np.concatenate([xy[j], wh[j]])], category=int(cat[j]),
                             area=float(area[j]), iscrowd=int(crowd[j])) for j in range(n)])
        per_class = []
        for c in range(n_cls):
            own = np.flatnonzero(cat == c)
            m = 0 if i == 5 else rs.randint(0, 31)
            src = np.concatenate([own, own])[:m]
            hit = np.concatenate([xy[src], xy[src] + wh[src]], 1) + rs.uniform(-6, 6, (len(src), 4))
            p = rs.uniform(0, [W - 40, H - 40], (m - len(src), 2))
            miss = np.concatenate([p, p + np.exp(rs.uniform(np.log(6), np.log(260), (len(p), 2)))], 1)
            boxes = np.concatenate([hit, miss])
            per_class.append(np.concatenate([boxes, np.round(rs.uniform(0.05, 1, (m, 1)), 1)], 1).astype(np.float32))
        results.append(per_class)
    return gt_anns, results


def pack_segments(segs):
    """segs: list of (dets [m, 5] = x, y, w, h, score; boxes [k, 4] = x, y, w, h; area [k] or None = w * h; crowd [k] or None)
    -> the pack of ``pack_coco_segments`` with one class and one image per entry (detections put in descending score order)"""
    d, g, ar, cr = [], [], [], []
    for dets, boxes, area, crowd in segs:
        dets = np.asarray(dets, np.float64).reshape(-1, 5)
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        d.append(dets[np.argsort(-dets[:, 4], kind='mergesort')])
        g.append(boxes)
        ar.append(boxes[:, 2] * boxes[:, 3] if area is None else np.asarray(area, np.float64).reshape(-1))
        cr.append(np.zeros(len(boxes), np.uint8) if crowd is None else np.asarray(crowd).astype(np.uint8).reshape(-1))
        assert len(ar[-1]) == len(boxes) == len(cr[-1])
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)      # noqa: E731
    cat = lambda xs, tail: np.ascontiguousarray(np.concatenate(xs + [tail]))                      # noqa: E731
    dd = cat(d, np.zeros((0, 5)))
    seg = np.repeat(np.arange(len(segs)), [len(x) for x in d])
    return dict(dets=np.ascontiguousarray(dd[:, :4]), det_off=off(d), gts=cat(g, np.zeros((0, 4))),
                gt_area=cat(ar, np.zeros(0)), gt_crowd=cat(cr, np.zeros(0, np.uint8)), gt_off=off(g),
                det_score=np.ascontiguousarray(dd[:, 4]), det_rank=np.arange(len(dd)) - off(d)[:-1][seg].astype(np.int64),
                det_cat=np.zeros(len(dd), np.int64), gt_cat=np.zeros(sum(len(x) for x in g), np.int64), num_classes=1)


def summary(pack, flags, max_dets, names=None):
    return E.coco_summarize(*E.coco_accumulate(pack, flags, max_dets), names)
