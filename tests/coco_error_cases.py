"""Inputs of the COCO error analysis suites (tests/test_coco_error.py on the CPU, tests/test_hip_coco_error.py on the GPU): the
hand cases with their flags written out, the seeded split, packs built image by image, and the reference tool's algorithm done
the long way (per class: deep copy, relabel, keep that class's detections, the unchanged evaluation path, column k)."""
import copy
import importlib.util
import json
import os
import sys

import numpy as np

from oadg_amd import evaluation as E

THRS, SIM = list(E.ERROR_THRS), E.ERROR_SIM_THR          # rows 0.75, 0.5, 0.1 | Sim (0.1) | Oth (0.1)
AREAS = (1024, 9216, 10 ** 10)
AREA_RNG = E.error_area_rng(AREAS)                        # all, small, medium, large
ALL, SMALL, MEDIUM, LARGE = range(4)
SUPERCATS = [0, 0, 0, 1, 1, 2]
FP, TP, IG = E.COCO_FP, E.COCO_TP, E.COCO_IGNORED


def pack_images(images, num_classes, supercats):
    """images: list of (boxes: list of (x, y, w, h, category[, area[, crowd]]); dets: {category: rows x, y, w, h, score})
    -> ``pack_coco_error`` of them (results in the x1, y1, x2, y2, score format it reads)"""
    gt_anns, results = [], []
    for boxes, dets in images:
        gt_anns.append([dict(bbox=[float(v) for v in b[:4]], category=int(b[4]),
                             area=float(b[5]) if len(b) > 5 and b[5] is not None else float(b[2]) * float(b[3]),
                             iscrowd=int(b[6]) if len(b) > 6 else 0) for b in boxes])
        per = []
        for k in range(num_classes):
            d = np.asarray(dets.get(k, []), np.float64).reshape(-1, 5)
            per.append(np.stack([d[:, 0], d[:, 1], d[:, 0] + d[:, 2], d[:, 1] + d[:, 3], d[:, 4]], 1))
        results.append(per)
    return E.pack_coco_error(gt_anns, results, num_classes, supercats)


# ------------------------------------------------------------------------------------------------------------ hand cases
# Each: (images, K, supercats, expected) with expected = {area range: [per detection in pack order, the 5 rows]}.  Boxes and
# detections are integers, so x, y, x + w, y + h are exact and every IoU below is the quotient written beside it.
def hand_cases():
    cases = {}
    # a class-0 detection exactly on a class-1 box.  Same supercategory: a false positive in the plain rows, ignored in both
    # variants; another supercategory: ignored only when every class's confusion is.  (100 x 100: 'large')
    on_foreign = [([(0, 0, 100, 100, 1)], {0: [[0, 0, 100, 100, 0.9]]})]
    cases['same supercategory'] = (on_foreign, 2, [0, 0], {ALL: [[FP, FP, FP, IG, IG]], LARGE: [[FP, FP, FP, IG, IG]],
                                                           SMALL: [[IG, IG, IG, IG, IG]]})
    cases['another supercategory'] = (on_foreign, 2, [0, 1], {ALL: [[FP, FP, FP, FP, IG]], LARGE: [[FP, FP, FP, FP, IG]],
                                                              MEDIUM: [[IG, IG, IG, IG, IG]]})
    # own box [0, 100) x [0, 100), detection [0, 100) x [0, 30): IoU 3000 / 10000 = 0.3; a class-1 box [0, 100) x [0, 27) holds
    # 0.9 of the detection (crowd style: 2700 / 3000).  A regular match above the threshold beats an ignored one: a true
    # positive at 0.1 in all three, a false positive at 0.75 and 0.5
    cases['a regular match beats an ignored one'] = (
        [([(0, 0, 100, 27, 1), (0, 0, 100, 100, 0)], {0: [[0, 0, 100, 30, 0.9]]})], 2, [0, 0],
        {ALL: [[FP, FP, TP, TP, TP]]})
    # two detections inside one foreign box: a crowd takes any number of detections
    cases['two detections on one foreign box'] = (
        [([(0, 0, 200, 200, 1)], {0: [[10, 10, 50, 50, 0.9], [100, 100, 80, 40, 0.8]]})], 2, [0, 0],
        {ALL: [[FP, FP, FP, IG, IG]] * 2})
    # a 'large' foreign box is present and ignored in 'small' too: the 20 x 20 detection inside it is ignored there, not a
    # false positive; in 'medium' and 'large' the detection (400 pixels) is outside the range: ignored, matched or not
    cases['a foreign box outside the area range'] = (
        [([(0, 0, 200, 200, 1)], {0: [[10, 10, 20, 20, 0.9]]})], 2, [0, 0],
        {ALL: [[FP, FP, FP, IG, IG]], SMALL: [[FP, FP, FP, IG, IG]], MEDIUM: [[IG] * 5], LARGE: [[IG] * 5]})
    # an unmatched detection outside the range is ignored (100 pixels: inside all and small)
    cases['an unmatched detection outside the range'] = (
        [([(0, 0, 50, 50, 0), (300, 0, 50, 50, 1)], {0: [[400, 300, 10, 10, 0.9]]})], 2, [0, 0],
        {ALL: [[FP] * 5], SMALL: [[FP] * 5], MEDIUM: [[IG] * 5], LARGE: [[IG] * 5]})
    return cases


# ------------------------------------------------------------------------------------------------------------ seeded split
def seeded_split(seed=0, n_img=12, n_cls=6, W=640, H=384):
    """(gt_anns, results): per image poisson(10) boxes with sides exp(U(log 6, log 260)), 15 % crowds, area = w * h *
    U(0.4, 1); image 3 is empty, image 5 has no detections.  Per (image, class) randint(0, 16) detections that copy ANY box of
    the image, whatever its class - the confusion -, jittered by U(-1, 1) * one of {2, 12, 40} pixels, plus randint(0, 4)
    random boxes; scores with one decimal (ties)."""
    rs = np.random.RandomState(seed)
    gt_anns, results = [], []
    for i in range(n_img):
        n = 0 if i == 3 else rs.poisson(10)
        xy = rs.uniform(0, [W - 40, H - 40], (n, 2))
        wh = np.exp(rs.uniform(np.log(6), np.log(260), (n, 2)))
        cat = rs.randint(0, n_cls, n)
        crowd = rs.uniform(size=n) < 0.15
        area = wh[:, 0] * wh[:, 1] * rs.uniform(0.4, 1.0, n)
        gt_anns.append([dict(bbox=[float(v) for v in np.concatenate([xy[j], wh[j]])], category=int(cat[j]),
                             area=float(area[j]), iscrowd=int(crowd[j])) for j in range(n)])
        per_class = []
        for c in range(n_cls):
            m = rs.randint(0, 16) if n and i != 5 else 0
            src = rs.randint(0, max(n, 1), m)
            jitter = rs.uniform(-1, 1, (m, 4)) * np.array([2.0, 12.0, 40.0])[rs.randint(0, 3, m)][:, None]
            hit = (np.concatenate([xy[src], xy[src] + wh[src]], 1) + jitter) if m else np.zeros((0, 4))
            r = 0 if i == 5 else rs.randint(0, 4)
            p = rs.uniform(0, [W - 40, H - 40], (r, 2))
            miss = np.concatenate([p, p + np.exp(rs.uniform(np.log(6), np.log(260), (r, 2)))], 1)
            boxes = np.concatenate([hit, miss])
            boxes[:, 2:] = np.maximum(boxes[:, 2:], boxes[:, :2] + 1)
            per_class.append(np.concatenate([boxes, np.round(rs.uniform(0.05, 1, (len(boxes), 1)), 1)], 1).astype(np.float32))
        results.append(per_class)
    return gt_anns, results


# ------------------------------------------------------------------------------------------------------------ the long way
def _precision(gt_anns, results, K, thrs, area_rng):
    """the unchanged evaluation path: pack_coco_segments -> coco_flags_host -> coco_accumulate, maxDets = [100]"""
    pack = E.pack_coco_segments(gt_anns, results, K, 100)
    flags = E.coco_flags_host(pack, thrs, area_rng, iou_thrs=thrs)
    return E.coco_accumulate(pack, flags, [100], iou_thrs=thrs, area_rng=area_rng)[0]


def long_way(gt_anns, results, K, supercats, areas=AREAS):
    """analyze_results / analyze_individual_category of the reference's tool, step by step -> ps [7, R, K, 4, 1]"""
    area_rng = E.error_area_rng(areas)
    ps = _precision(gt_anns, results, K, [0.75, 0.5, 0.1], area_rng)
    ps = np.vstack([ps, np.zeros((4, *ps.shape[1:]))])
    for k in range(K):
        dt = [[r if c == k else np.zeros((0, 5), np.float32) for c, r in enumerate(per)] for per in copy.deepcopy(results)]
        for row, foreign in ((3, lambda c: supercats[c] == supercats[k]), (4, lambda c: True)):
            gt = copy.deepcopy(gt_anns)
            for per in gt:
                for ann in per:
                    if ann['category'] != k and foreign(ann['category']):
                        ann['ignore'] = 1
                        ann['iscrowd'] = 1
                        ann['category'] = k
            ps[row, :, k, :, :] = _precision(gt, dt, K, [0.1], area_rng)[0, :, k, :, :]
        ps[ps == -1] = 0
        ps[5, :, k, :, :] = ps[4, :, k, :, :] > 0
        ps[6, :, k, :, :] = 1.0
    return ps


# ------------------------------------------------------------------------------------------------------------ files
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('person', 'rider', 'car', 'truck', 'bus', 'train')


def load_tool(path):
    """a tool by its path below the repository root"""
    if os.path.join(ROOT, 'tools') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'tools'))                 # (tools/test.py imports tools/train.py's DictAction)
    spec = importlib.util.spec_from_file_location('oadg_tool_' + os.path.basename(path)[:-3], os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def write_ann(path, gt_anns, names, supercategory=None, W=640, H=384):
    """a COCO annotation file whose image ids (10, 13, 16, ...) and category ids (3, 5, 7, ...) are not 0 .. n"""
    images = [dict(id=10 + 3 * i, file_name=f'{i}.png', height=H, width=W) for i in range(len(gt_anns))]
    anns = [dict(id=100 + j, image_id=10 + 3 * i, category_id=3 + 2 * g['category'], iscrowd=g['iscrowd'], area=g['area'],
                 bbox=g['bbox']) for j, (i, g) in enumerate((i, g) for i, per in enumerate(gt_anns) for g in per)]
    cats = [dict(id=3 + 2 * k, name=n, **({} if supercategory is None else dict(supercategory=supercategory[k])))
            for k, n in enumerate(names)]
    with open(path, 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=cats), f)
    return str(path)


def coco_dataset(ann, names):
    from oadg_amd.datasets import CocoDataset
    return CocoDataset(ann, classes=tuple(names), img_prefix=os.path.dirname(ann), device='cpu', test_mode=True)
