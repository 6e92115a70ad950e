"""COCO-style bounding-box evaluation (AP@[.50:.95], AP50, AP75, APs/m/l, AR1/10/100, ARs/m/l) for the Cityscapes /
COCO-format test sets, and the corruption-benchmark aggregation (P, mPC, rPC).

The reference evaluates through ``CocoDataset.evaluate`` -> ``pycocotools.cocoeval.COCOeval`` (mmdet/datasets/coco.py:
362-...; mmdet/datasets/cityscapes.py:212-... delegates 'bbox' to it) and aggregates the robustness runs with
tools/analysis_tools/robustness_eval.py:37-118 and test_robustness.py:28-64.  pycocotools is not installed here, so
this file restates COCOeval's published algorithm for iouType 'bbox' (evaluateImg / accumulate / summarize): the greedy
score-ordered matching with crowd and area-range "ignore" regions, the 101-point interpolated precision envelope, and
the twelve summary numbers.  It is pinned by hand-computed cases (tests/test_evaluation.py), not by pycocotools.

The VOC protocol of the Diverse-Weather benchmark (``SdgodDataset.evaluate`` -> mmdet/core/evaluation/mean_ap.py ``eval_map``
with 'voc07' and the legacy coordinates) is ``eval_map_voc`` below: host functions pinned to the reference's own output
(tests/golden/voc_eval_reference.npz) and the same matching on the GPU (csrc/voc_eval.hip).

The recall of PROPOSALS (mmdet/core/evaluation/recall.py ``eval_recalls``; the 'proposal', 'proposal_fast' and 'recall' metrics
of the reference's datasets, for the results of an 'RPN' detector) is ``eval_recalls`` / ``proposal_evaluate`` below: host
functions pinned to the reference's own output (tests/golden/recall_reference.npz) and the same matching on the GPU
(csrc/recall.hip).
"""
import os

import numpy as np

from ._lib import VOC_MAX_THRS                # thresholds of one device call (oadg_voc_tpfp)

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
METRICS = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'AR1', 'AR10', 'AR100', 'ARs', 'ARm', 'ARl']
# CocoDataset.evaluate (mmdet/datasets/coco.py:362-575, CityscapesDataset delegates 'bbox' to it): proposal_nums =
# (100, 300, 1000) become cocoEval.params.maxDets, mAP is taken at maxDets[-1] = 1000 and the names are mmdet's
MMDET_MAX_DETS = (100, 300, 1000)
MMDET_METRICS = ['mAP', 'mAP_50', 'mAP_75', 'mAP_s', 'mAP_m', 'mAP_l', 'AR@100', 'AR@300', 'AR@1000', 'AR_s@1000',
                 'AR_m@1000', 'AR_l@1000']


def _iou_xywh(d, g, iscrowd):
    """maskUtils.iou for boxes [x, y, w, h]: intersection / union, or / det area for crowd ground truth"""
    if len(d) == 0 or len(g) == 0:
        return np.zeros((len(d), len(g)))
    d, g = np.asarray(d, np.float64), np.asarray(g, np.float64)
    iw = np.minimum(d[:, None, 0] + d[:, None, 2], g[None, :, 0] + g[None, :, 2]) - np.maximum(d[:, None, 0], g[None, :, 0])
    ih = np.minimum(d[:, None, 1] + d[:, None, 3], g[None, :, 1] + g[None, :, 3]) - np.maximum(d[:, None, 1], g[None, :, 1])
    inter = np.clip(iw, 0, None) * np.clip(ih, 0, None)
    da, ga = d[:, 2] * d[:, 3], g[:, 2] * g[:, 3]
    union = np.where(np.asarray(iscrowd, bool)[None, :], da[:, None], da[:, None] + ga[None, :] - inter)
    with np.errstate(divide='ignore', invalid='ignore'):
        out = inter / union
    return np.where(union > 0, out, 0.0)


def _evaluate_img(gts, dts, a_rng, max_det, iou_thrs=None):
    """COCOeval.evaluateImg for one (image, category).  gts: list of dict(bbox xywh, area, iscrowd); dts: list of
    dict(bbox xywh, area, score).  Returns None when both are empty.  ``iou_thrs``: params.iouThrs, IOU_THRS by default."""
    if not gts and not dts:
        return None
    iou_thrs = IOU_THRS if iou_thrs is None else iou_thrs
    g_ig = np.array([1 if (g['iscrowd'] or g['area'] < a_rng[0] or g['area'] > a_rng[1]) else 0 for g in gts], int)
    gtind = np.argsort(g_ig, kind='mergesort')
    gts = [gts[i] for i in gtind]
    g_ig = g_ig[gtind]
    dtind = np.argsort([-d['score'] for d in dts], kind='mergesort')[:max_det]
    dts = [dts[i] for i in dtind]
    iscrowd = [int(g['iscrowd']) for g in gts]
    ious = _iou_xywh([d['bbox'] for d in dts], [g['bbox'] for g in gts], iscrowd)
    T, G, D = len(iou_thrs), len(gts), len(dts)
    gtm, dtm, dt_ig = np.zeros((T, G)), np.zeros((T, D)), np.zeros((T, D))
    if G and D:
        for ti, t in enumerate(iou_thrs):
            for di in range(D):
                iou, m = min(t, 1 - 1e-10), -1
                for gi in range(G):
                    if gtm[ti, gi] > 0 and not iscrowd[gi]:
                        continue                      # already matched, and not a crowd
                    if m > -1 and g_ig[m] == 0 and g_ig[gi] == 1:
                        break                         # a regular match exists: do not trade it for an ignored gt
                    if ious[di, gi] < iou:
                        continue
                    iou, m = ious[di, gi], gi
                if m == -1:
                    continue
                dt_ig[ti, di] = g_ig[m]
                dtm[ti, di] = m + 1
                gtm[ti, m] = di + 1
    out_of_range = np.array([d['area'] < a_rng[0] or d['area'] > a_rng[1] for d in dts], bool).reshape(1, D)
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(out_of_range, T, 0)))
    return dict(dtm=dtm, dt_ig=dt_ig, g_ig=g_ig, scores=np.array([d['score'] for d in dts], np.float64))


def coco_eval_bbox(gt_anns, results, num_classes, max_dets=None, names=None, device=None):
    """gt_anns: per image, list of dict(bbox=[x, y, w, h], category=label index, area, iscrowd);
    results: per image, list over classes of arrays [k, 5] = x1, y1, x2, y2, score (``bbox2result`` format).
    Returns dict(metric name -> value) with the twelve COCO numbers (-1 where undefined).
    ``max_dets`` / ``names``: COCOeval's defaults (1, 10, 100) with its own names - what test_robustness.py's
    coco_eval_with_return reports - or MMDET_MAX_DETS / MMDET_METRICS for the numbers of ``CocoDataset.evaluate``
    (tools/test.py --eval bbox).
    ``device=None``: the host loops below; a torch device: one pack, csrc/coco_eval.hip for the matching of the whole split,
    a vectorised accumulate - the same flags, so the same twelve numbers (tests/test_hip_coco_eval.py compares with ==)."""
    MAX_DETS = list(max_dets) if max_dets is not None else [1, 10, 100]
    names = list(names) if names is not None else METRICS
    assert len(MAX_DETS) == 3 and len(names) == 12
    if device is not None:
        pack = pack_coco_segments(gt_anns, results, num_classes, MAX_DETS[-1])
        precision, recall = coco_accumulate(pack, coco_flags_device(pack, IOU_THRS, AREA_RNG, device), MAX_DETS)
        return coco_summarize(precision, recall, names)
    n_img = len(gt_anns)
    assert len(results) == n_img
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), num_classes, len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    eps = np.spacing(1)
    for k in range(K):
        per_img = []
        for i in range(n_img):
            gts = [g for g in gt_anns[i] if g['category'] == k]
            dets = np.asarray(results[i][k], np.float64).reshape(-1, 5)
            # CocoDataset._det2json / xyxy2xywh + COCO.loadRes (area = w * h)
            dts = [dict(bbox=[d[0], d[1], d[2] - d[0], d[3] - d[1]], area=(d[2] - d[0]) * (d[3] - d[1]), score=d[4])
                   for d in dets]
            dts = [dts[j] for j in np.argsort([-d['score'] for d in dts], kind='mergesort')[:MAX_DETS[-1]]]
            per_img.append((gts, dts))
        for a, a_rng in enumerate(AREA_RNG):
            evs = [_evaluate_img(g, d, a_rng, MAX_DETS[-1]) for g, d in per_img]
            evs = [e for e in evs if e is not None]
            if not evs:
                continue
            for m, max_det in enumerate(MAX_DETS):
                scores = np.concatenate([e['scores'][:max_det] for e in evs])
                inds = np.argsort(-scores, kind='mergesort')
                dtm = np.concatenate([e['dtm'][:, :max_det] for e in evs], axis=1)[:, inds]
                dt_ig = np.concatenate([e['dt_ig'][:, :max_det] for e in evs], axis=1)[:, inds]
                g_ig = np.concatenate([e['g_ig'] for e in evs])
                npig = np.count_nonzero(g_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
                for t in range(T):
                    tp, fp = tp_sum[t], fp_sum[t]
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + eps)
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros((R,))
                    for ri, pi in enumerate(np.searchsorted(rc, REC_THRS, side='left')):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, k, a, m] = q

    return coco_summarize(precision, recall, names)


def coco_summarize(precision, recall, names=None):
    """COCOeval.summarize: precision [T, R, K, A, M] and recall [T, K, A, M] (-1 where undefined) -> the twelve numbers"""
    def summarize(ap, iou=None, area=0, max_det=2):
        s = precision[:, :, :, area, max_det] if ap else recall[:, :, area, max_det]
        if iou is not None:
            s = s[np.where(np.isclose(IOU_THRS, iou))[0]]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    stats = [summarize(1), summarize(1, .5), summarize(1, .75), summarize(1, None, 1), summarize(1, None, 2),
             summarize(1, None, 3), summarize(0, None, 0, 0), summarize(0, None, 0, 1), summarize(0, None, 0, 2),
             summarize(0, None, 1), summarize(0, None, 2), summarize(0, None, 3)]
    return dict(zip(METRICS if names is None else names, stats))


# ------------------------------------------------------------------------------------------ COCO matching, one split at a time
# The same protocol as ``coco_eval_bbox`` above cut into the steps of the device path: pack the split into flat arrays (one
# segment per (image, category), as pack_voc_segments), match every segment for every (area range, threshold) - on the host
# through ``_evaluate_img`` (the yardstick) or in one launch of csrc/coco_eval.hip -, accumulate with numpy.  All that
# accumulate reads of the matching is one flag per (area range, threshold, detection).
COCO_FP, COCO_TP, COCO_IGNORED = 0, 1, 2


def pack_coco_segments(gt_anns, results, num_classes, max_det, xywh=False):
    """a split as the arrays of oadg_coco_match: one segment per (image, category), s = image * num_classes + category.
    dict(dets fp64 [D, 4] = x, y, w, h - per segment by descending score (stable) and cut to ``max_det`` -, det_off int32
    [S + 1], gts fp64 [G, 4] = x, y, w, h in annotation order, gt_area fp64 [G] (the annotation's field), gt_crowd uint8 [G],
    gt_off int32 [S + 1]; per kept detection det_score fp64, det_rank (its place within the segment) and det_cat; gt_cat).
    ``xywh``: the rows of ``results`` are x, y, w, h, score already (a COCO result file read back: nothing is subtracted)."""
    n, K = len(gt_anns), int(num_classes)
    assert len(results) == n
    S = n * K
    flat = [np.asarray(results[i][k], np.float64).reshape(-1, 5) for i in range(n) for k in range(K)]
    cnt = np.fromiter((len(a) for a in flat), dtype=np.int64, count=S)
    d = np.concatenate(flat) if S else np.zeros((0, 5), np.float64)
    seg = np.repeat(np.arange(S, dtype=np.int64), cnt)
    order = np.lexsort((-d[:, 4], seg))           # (stable: by segment, by descending score, by position among equal scores)
    d = d[order]
    first = np.concatenate([[0], np.cumsum(cnt)])
    rank = np.arange(len(d), dtype=np.int64) - first[:-1][seg]
    keep = rank < max_det
    d, seg, rank = d[keep], seg[keep], rank[keep]
    # CocoDataset._det2json / xyxy2xywh
    if xywh:
        dets = d[:, :4]
    else:
        dets = np.stack([d[:, 0], d[:, 1], d[:, 2] - d[:, 0], d[:, 3] - d[:, 1]], axis=1) if len(d) else np.zeros((0, 4))
    anns = [(i, g) for i, per_img in enumerate(gt_anns) for g in per_img]
    g_img = np.fromiter((i for i, _ in anns), dtype=np.int64, count=len(anns))
    g_cat = np.fromiter((g['category'] for _, g in anns), dtype=np.int64, count=len(anns))
    g_box = np.array([g['bbox'] for _, g in anns], np.float64).reshape(-1, 4)
    g_area = np.fromiter((g['area'] for _, g in anns), dtype=np.float64, count=len(anns))
    g_crowd = np.fromiter((bool(g['iscrowd']) for _, g in anns), dtype=np.uint8, count=len(anns))
    ok = (g_cat >= 0) & (g_cat < K)
    g_seg = (g_img * K + g_cat)[ok]
    g_order = np.argsort(g_seg, kind='stable')     # (annotation order within a segment)
    assert len(dets) < 2 ** 31 and len(g_order) < 2 ** 31
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int32)           # noqa: E731
    return dict(dets=np.ascontiguousarray(dets), det_off=off(np.bincount(seg, minlength=S)),
                gts=np.ascontiguousarray(g_box[ok][g_order]), gt_area=np.ascontiguousarray(g_area[ok][g_order]),
                gt_crowd=np.ascontiguousarray(g_crowd[ok][g_order]), gt_off=off(np.bincount(g_seg, minlength=S)),
                det_score=np.ascontiguousarray(d[:, 4]), det_rank=rank, det_cat=seg % K, gt_cat=g_cat[ok][g_order],
                num_classes=K)


def coco_flags_host(pack, thrs=None, area_rng=None, want_match=False, iou_thrs=None):
    """``_evaluate_img`` over every (segment, area range) of a pack -> flags uint8 [n_area, n_thr, D]: COCO_FP (unmatched,
    inside the range), COCO_TP (matched to a box that is not ignored), COCO_IGNORED (matched to an ignored box, or unmatched
    and outside the range); with ``want_match`` also int32 [n_area, n_thr, D], the matched box within its segment in
    annotation order, or -1.  ``thrs``: thresholds out of IOU_THRS (``_evaluate_img`` knows no others), all of them by default.
    ``iou_thrs``: another params.iouThrs for ``_evaluate_img`` to match at, in the place of IOU_THRS in the sentence before."""
    iou_thrs = IOU_THRS if iou_thrs is None else np.asarray(iou_thrs, np.float64)
    thrs = iou_thrs if thrs is None else thrs
    area_rng = AREA_RNG if area_rng is None else area_rng
    rows = [np.flatnonzero(iou_thrs == t) for t in thrs]
    if any(len(r) != 1 for r in rows):
        raise ValueError('the host evaluator matches at IOU_THRS only')
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    D = len(pack['dets'])
    flags = np.zeros((len(area_rng), len(rows), D), dtype=np.uint8)
    match = np.full((len(area_rng), len(rows), D), -1, dtype=np.int32)
    d_off, g_off = pack['det_off'], pack['gt_off']
    for s in np.flatnonzero(np.diff(d_off)):
        d0, d1, g0, g1 = d_off[s], d_off[s + 1], g_off[s], g_off[s + 1]
        gts = [dict(bbox=pack['gts'][g], area=pack['gt_area'][g], iscrowd=int(pack['gt_crowd'][g])) for g in range(g0, g1)]
        dts = [dict(bbox=pack['dets'][j], area=pack['dets'][j, 2] * pack['dets'][j, 3], score=pack['det_score'][j])
               for j in range(d0, d1)]
        for a, a_rng in enumerate(area_rng):
            e = _evaluate_img(gts, dts, a_rng, d1 - d0, iou_thrs)
            dtm, dt_ig = e['dtm'][rows], e['dt_ig'][rows]
            flags[a, :, d0:d1] = np.where(dt_ig, COCO_IGNORED, np.where(dtm > 0, COCO_TP, COCO_FP))
            if want_match and g1 > g0:
                # dtm counts in _evaluate_img's order of the boxes: its stable sort by the ignore flag, redone here
                g_ig = [1 if (g['iscrowd'] or g['area'] < a_rng[0] or g['area'] > a_rng[1]) else 0 for g in gts]
                gtind = np.argsort(np.array(g_ig, int), kind='mergesort')
                assert np.array_equal(np.array(g_ig, int)[gtind], e['g_ig'])
                match[a, :, d0:d1] = np.where(dtm > 0, gtind[np.maximum(dtm.astype(np.int64), 1) - 1], -1)
    return (flags, match) if want_match else flags


def coco_flags_device(pack, thrs, area_rng, device, timings=None, want_match=False):
    """the same flags from csrc/coco_eval.hip: one upload of the pack through the staging path, ONE launch for the split, all
    thresholds and all area ranges, one download (``oadg_coco_match.flags_device``, the module next to the package's import
    shim that holds the ctypes call of the kernel; see its docstring for why that call is not in hip_ops.py)."""
    import oadg_coco_match
    return oadg_coco_match.flags_device(pack, thrs, area_rng, device, timings=timings, want_match=want_match)


def coco_accumulate(pack, flags, max_dets, iou_thrs=None, area_rng=None):
    """COCOeval.accumulate over the flags of a pack (uint8 [A, T, D] for AREA_RNG and IOU_THRS, in pack order) -> (precision
    [T, R, K, A, M], recall [T, K, A, M]), exactly the arrays ``coco_eval_bbox`` fills: per (category, area range, maxDets)
    the detections of rank < maxDets by descending score (stable over the images in order), fp64 cumulative tp / fp,
    recall over the boxes that are not ignored, the precision envelope sampled at REC_THRS; -1 where no box counts.
    ``iou_thrs`` / ``area_rng``: the thresholds (only their number is read) and area ranges of ``flags`` when they are not
    IOU_THRS and AREA_RNG.  The boxes that count are those of ``gt_cat``'s own class (pack_coco_error: the relabelled boxes of
    the two variants are ignored, so they never count)."""
    iou_thrs = IOU_THRS if iou_thrs is None else iou_thrs
    area_rng = AREA_RNG if area_rng is None else area_rng
    T, R, K, A, M = len(iou_thrs), len(REC_THRS), pack['num_classes'], len(area_rng), len(max_dets)
    assert flags.shape == (A, T, len(pack['dets']))
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    eps = np.spacing(1)
    area, crowd = pack['gt_area'], pack['gt_crowd'] != 0
    # the boxes that count per (category, area range): not crowd, area inside [lo, hi]
    npig = np.stack([np.bincount(pack['gt_cat'][~(crowd | (area < lo) | (area > hi))], minlength=K) for lo, hi in area_rng], 1)
    score, rank, cat = pack['det_score'], pack['det_rank'], pack['det_cat']
    by_cat = np.argsort(cat, kind='stable')
    cuts = np.searchsorted(cat[by_cat], np.arange(K + 1))
    for k in range(K):
        if not npig[k].any():
            continue
        idx = by_cat[cuts[k]:cuts[k + 1]]                       # (pack order: image after image)
        for m, max_det in enumerate(max_dets):
            sel = idx[rank[idx] < max_det]
            sel = sel[np.argsort(-score[sel], kind='mergesort')]
            nd = len(sel)
            for a in range(A):
                if npig[k, a] == 0:
                    continue
                f = flags[a][:, sel]
                tp = np.cumsum(f == COCO_TP, axis=1).astype(np.float64)
                fp = np.cumsum(f == COCO_FP, axis=1).astype(np.float64)
                rc = tp / npig[k, a]
                pr = tp / (fp + tp + eps)
                recall[:, k, a, m] = rc[:, -1] if nd else 0
                pr = np.maximum.accumulate(pr[:, ::-1], axis=1)[:, ::-1]       # (the envelope: the backward loop's values)
                q = np.zeros((T, R))
                for t in range(T):
                    pi = np.searchsorted(rc[t], REC_THRS, side='left')
                    ok = pi < nd
                    q[t, ok] = pr[t, pi[ok]]
                precision[:, :, k, a, m] = q
    return precision, recall


# ------------------------------------------------------------------------------------------ COCO error analysis
# tools/analysis_tools/coco_error_analysis.py of the reference: the precision lost by each class split into C75 / C50 (AP at
# IoU 0.75 / 0.5), Loc (AP at 0.1), Sim (AP at 0.1 when confusion inside the supercategory is ignored), Oth (when confusion with
# every class is ignored), BG and FN.  The reference runs COCOeval once at [0.75, 0.5, 0.1] and per class twice more at [0.1]
# on a deep copy of the dataset whose foreign boxes are relabelled `ignore = 1, iscrowd = 1, category_id = catId`.  Here: one
# pack that holds every box of an image once, all 3 + 2 matchings x 4 area ranges of every (image, class) in one launch of
# csrc/coco_error.hip (or the literal host restatement below, the yardstick), one accumulate.
ERROR_THRS = (0.75, 0.5, 0.1)              # analyze_results: cocoEval.params.iouThrs
ERROR_SIM_THR = 0.1                        # analyze_individual_category: cocoEval.params.iouThrs of both variants
ERROR_TYPES = ('C75', 'C50', 'Loc', 'Sim', 'Oth', 'BG', 'FN')
ERROR_AREA_NAMES = ('allarea', 'small', 'medium', 'large')
ERROR_MAX_DET = 100


def error_area_rng(areas):
    """analyze_results: the three ``--areas`` bounds as params.areaRng (all, small, medium, large)"""
    areas = list(areas)
    assert len(areas) == 3, '3 integers should be specified as areas, representing 3 area regions'
    return [[0 ** 2, areas[2]], [0 ** 2, areas[0]], [areas[0], areas[1]], [areas[1], areas[2]]]


def pack_error_boxes(gt_anns, num_classes, supercats):
    """the box half of ``pack_coco_error``: every box of an image ONCE, whatever its class - gts fp64 [G, 4] = x, y, w, h in
    annotation order, gt_area, gt_crowd uint8, gt_cat int32, img_off int32 [n + 1] - and cat_super int32 [K] from ``supercats``
    (one hashable per class, equal values = one supercategory)"""
    n, K = len(gt_anns), int(num_classes)
    assert len(supercats) == K and n * K < 2 ** 31
    anns = [(i, g) for i, per_img in enumerate(gt_anns) for g in per_img if 0 <= g['category'] < K]
    G = len(anns)
    assert G < 2 ** 31
    g_img = np.fromiter((i for i, _ in anns), dtype=np.int64, count=G)
    ids = {}
    cat_super = np.array([ids.setdefault(v, len(ids)) for v in supercats], np.int32).reshape(K)
    return dict(gts=np.ascontiguousarray(np.array([g['bbox'] for _, g in anns], np.float64).reshape(-1, 4)),
                gt_area=np.fromiter((g['area'] for _, g in anns), dtype=np.float64, count=G),
                gt_crowd=np.fromiter((bool(g['iscrowd']) for _, g in anns), dtype=np.uint8, count=G),
                gt_cat=np.fromiter((g['category'] for _, g in anns), dtype=np.int32, count=G),
                img_off=np.concatenate([[0], np.cumsum(np.bincount(g_img, minlength=n))]).astype(np.int32),
                cat_super=cat_super, num_classes=K)


def pack_coco_error(gt_anns, results, num_classes, supercats, max_det=ERROR_MAX_DET, xywh=False):
    """a split as the arrays of oadg_coco_error_match.  The detections as ``pack_coco_segments`` packs them (dets, det_off,
    det_score, det_rank, det_cat: one segment per (image, category), s = image * num_classes + category, by descending score,
    cut to ``max_det``; ``xywh`` as there); the boxes as ``pack_error_boxes`` packs them, once per image."""
    seg = pack_coco_segments([[] for _ in range(len(gt_anns))], results, int(num_classes), max_det, xywh=xywh)
    return dict(pack_error_boxes(gt_anns, num_classes, supercats),
                **{k: seg[k] for k in ('dets', 'det_off', 'det_score', 'det_rank', 'det_cat')})


def coco_error_flags_host(pack, thrs, sim_thr, area_rng):
    """the yardstick of csrc/coco_error.hip -> flags uint8 [n_area, n_thr + 2, D].  Per (image, category k) segment with
    detections the reference's three box lists, built literally: the boxes of class k for the plain rows; for row n_thr the
    annotations of the image in order, those of another class of k's supercategory relabelled iscrowd = 1 (pycocotools derives
    ``ignore`` from it) and category k, the rest of the foreign ones left out; for row n_thr + 1 every foreign one relabelled.
    Each list goes through ``_evaluate_img`` at its own thresholds."""
    K, D = pack['num_classes'], len(pack['dets'])
    thrs = [float(t) for t in thrs]
    T = len(thrs)
    flags = np.zeros((len(area_rng), T + 2, D), dtype=np.uint8)
    d_off, i_off, sup = pack['det_off'], pack['img_off'], pack['cat_super']
    for s in np.flatnonzero(np.diff(d_off)):
        i, k = divmod(int(s), K)
        d0, d1 = d_off[s], d_off[s + 1]
        anns = [dict(bbox=pack['gts'][g], area=pack['gt_area'][g], iscrowd=int(pack['gt_crowd'][g]), category=int(pack['gt_cat'][g]))
                for g in range(i_off[i], i_off[i + 1])]
        dts = [dict(bbox=pack['dets'][j], area=pack['dets'][j, 2] * pack['dets'][j, 3], score=pack['det_score'][j])
               for j in range(d0, d1)]

        def relabelled(foreign):
            out = []
            for ann in anns:
                ann = dict(ann)                                      # (copy.deepcopy(cocoGt))
                if ann['category'] != k and foreign(ann['category']):
                    ann.update(ignore=1, iscrowd=1, category=k)
                if ann['category'] == k:                             # (useCats = 1: _gts[imgId, catId])
                    out.append(ann)
            return out
        lists = [(relabelled(lambda c: False), thrs, slice(0, T)),
                 (relabelled(lambda c: sup[c] == sup[k]), [float(sim_thr)], slice(T, T + 1)),
                 (relabelled(lambda c: True), [float(sim_thr)], slice(T + 1, T + 2))]
        for gts, iou_thrs, rows in lists:
            if not iou_thrs:
                continue
            for a, a_rng in enumerate(area_rng):
                e = _evaluate_img(gts, dts, a_rng, d1 - d0, iou_thrs)
                flags[a, rows, d0:d1] = np.where(e['dt_ig'], COCO_IGNORED, np.where(e['dtm'] > 0, COCO_TP, COCO_FP))
    return flags


def coco_error_flags_device(pack, thrs, sim_thr, area_rng, device, timings=None):
    """the same flags from csrc/coco_error.hip: one upload of the pack through the staging path, ONE launch for the split, all
    rows and all area ranges, one download (``oadg_coco_error.flags_device``, the module next to the package's import shim that
    holds the ctypes call of the kernel; see its docstring for why that call is not in hip_ops.py)."""
    import oadg_coco_error
    return oadg_coco_error.flags_device(pack, thrs, sim_thr, area_rng, device, timings=timings)


def coco_error_analysis(gt_anns, results, num_classes, supercats, areas=(1024, 9216, 10 ** 10), device=None, timings=None,
                        xywh=False):
    """analyze_results of the reference's coco_error_analysis.py for 'bbox' -> ps fp64 [7, R, K, 4, 1], the array it plots:
    the precision at the 101 recall thresholds per (ERROR_TYPES band, class, area range), maxDets = 100.  Bands 0 - 2 are the
    plain evaluation at ERROR_THRS, 3 and 4 the two variants at ERROR_SIM_THR, then ``ps[ps == -1] = 0``, BG = (Oth > 0),
    FN = 1.  gt_anns / results: as ``coco_eval_bbox`` (``xywh``: as ``pack_coco_segments``); supercats: one value per class.  ``device=None``: the host yardstick;
    a torch device: one launch of csrc/coco_error.hip - the same flags, so the same array."""
    area_rng = error_area_rng(areas)
    pack = pack_coco_error(gt_anns, results, num_classes, supercats, xywh=xywh)
    if device is None:
        flags = coco_error_flags_host(pack, ERROR_THRS, ERROR_SIM_THR, area_rng)
    else:
        flags = coco_error_flags_device(pack, ERROR_THRS, ERROR_SIM_THR, area_rng, device, timings=timings)
    rows = list(ERROR_THRS) + [ERROR_SIM_THR] * 2
    precision, _ = coco_accumulate(pack, flags, [ERROR_MAX_DET], iou_thrs=rows, area_rng=area_rng)
    ps = np.vstack([precision, np.zeros((2, *precision.shape[1:]))])
    ps[ps == -1] = 0
    ps[5] = ps[4] > 0
    ps[6] = 1.0
    return ps


def error_band_means(ps, names):
    """the numbers of the plots' legends, unrounded: per class (and 'allclass') and per area range the mean of each band"""
    out = {}
    for name, sub in list(zip(names, np.moveaxis(ps, 2, 0))) + [('allclass', ps)]:
        out[name] = {area: {t: float(sub[b][..., a, 0].mean()) for b, t in enumerate(ERROR_TYPES)}
                     for a, area in enumerate(ERROR_AREA_NAMES)}
    return out


def dataset_gt_anns(dataset, indices=None):
    """ground truth in the evaluator's format.  COCO-format datasets: the raw json annotations of every image (crowd
    regions included, as COCOeval sees them); synthetic datasets: their boxes (area = w * h, no crowds)."""
    idx = range(len(dataset)) if indices is None else indices
    out = []
    for i in idx:
        if hasattr(dataset, 'coco'):
            info = dataset.data_infos[i]
            anns = dataset.coco.load_anns(dataset.coco.get_ann_ids(img_ids=[info['id']]))
            out.append([dict(bbox=list(a['bbox']), category=dataset.cat2label[a['category_id']], area=a['area'],
                             iscrowd=int(a.get('iscrowd', 0))) for a in anns if a['category_id'] in dataset.cat_ids])
        else:
            b, l = dataset.boxes(i)
            out.append([dict(bbox=[float(x[0]), float(x[1]), float(x[2] - x[0]), float(x[3] - x[1])], category=int(c),
                             area=float((x[2] - x[0]) * (x[3] - x[1])), iscrowd=0) for x, c in zip(b, l)])
    return out


# ------------------------------------------------------------------------------------------ VOC-style mAP
def average_precision(recalls, precisions, mode='area'):
    """mean_ap.py:13-56 for one scale.  'area': the area under the precision envelope; '11points' (mean_ap.py:45-52, the
    VOC07 protocol): the mean of the best precision at recall >= 0, 0.1, ..., 1, accumulated in fp32 as the reference's
    ``ap`` array does."""
    if mode == '11points':
        recalls, precisions = np.asarray(recalls), np.asarray(precisions)
        ap = np.zeros(1, dtype=np.float32)
        for thr in np.arange(0, 1 + 1e-3, 0.1):
            precs = precisions[recalls >= thr]
            ap[0] += precs.max() if precs.size > 0 else 0
        ap /= 11
        return float(ap[0])
    if mode != 'area':
        raise ValueError('Unrecognized mode, only "area" and "11points" are supported')
    mrec = np.concatenate([[0.0], recalls, [1.0]])
    mpre = np.concatenate([[0.0], precisions, [0.0]])
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i])
    ind = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[ind + 1] - mrec[ind]) * mpre[ind + 1]))


def eval_map(results, annotations, num_classes, iou_thr=0.5):
    """mean_ap.py:298-440 (tpfp_default, no ignore / difficult flags): per-class AP and their mean."""
    from .core import bbox_overlaps_np
    aps = []
    for c in range(num_classes):
        scores, tp, n_gt = [], [], 0
        for res, (gtb, gtl) in zip(results, annotations):
            dets, gts = res[c], gtb[gtl == c]
            n_gt += len(gts)
            if len(dets) == 0:
                continue
            order = np.argsort(-dets[:, 4])
            flags = np.zeros(len(dets), dtype=np.float32)
            if len(gts):
                ious = bbox_overlaps_np(dets[:, :4], gts)
                best, arg = ious.max(axis=1), ious.argmax(axis=1)
                covered = np.zeros(len(gts), dtype=bool)
                for i in order:
                    if best[i] >= iou_thr and not covered[arg[i]]:
                        covered[arg[i]] = True
                        flags[i] = 1
            scores.append(dets[:, 4])
            tp.append(flags)
        if n_gt == 0:
            continue
        if not scores:
            aps.append(0.0)
            continue
        s, t = np.concatenate(scores), np.concatenate(tp)
        o = np.argsort(-s)
        ctp, cfp = np.cumsum(t[o]), np.cumsum(1 - t[o])
        aps.append(average_precision(ctp / max(n_gt, 1e-12), ctp / np.maximum(ctp + cfp, 1e-12)))
    return (float(np.mean(aps)) if aps else 0.0), aps


def dataset_box_anns(dataset, indices=None):
    """per image (boxes [n, 4], labels [n]): ``get_ann_info`` of a file dataset, ``boxes`` of the synthetic one"""
    idx = range(len(dataset)) if indices is None else indices
    anns = []
    for i in idx:
        if hasattr(dataset, 'get_ann_info'):
            a_ = dataset.get_ann_info(i)
            anns.append((a_['bboxes'], a_['labels']))
        else:
            anns.append(dataset.boxes(i))
    return anns


# ------------------------------------------------------------------------------------------ the reference's VOC protocol
# mean_ap.py:168-267, 297-440 and bbox_overlaps.py as SdgodDataset.evaluate drives them (sdgod.py:65-89): fp32 IoU with the
# legacy "+ 1" extents, difficult / min_size boxes as "ignore" regions, the 11-point AP for a VOC2007 prefix.  The host
# functions below are the yardstick (pinned to the reference's own output by tests/golden/voc_eval_reference.npz) and the
# path without a GPU; csrc/voc_eval.hip computes the same flags for a whole split in one launch.  Two rules are FIXED here
# where the reference leaves them to numpy: equal scores are ordered lowest index first (a stable
# sort, per image and in the per-class accumulation), and the threshold is rounded to fp32 and compared in fp32.
FLAG_IGNORED, FLAG_TP, FLAG_FP = 0, 1, 2


def bbox_overlaps_voc(b1, b2, use_legacy_coordinate=False):
    """bbox_overlaps.py:5-65, mode 'iou': fp32 [n, k], every operation in the reference's order (numpy fuses nothing)"""
    b1 = np.asarray(b1).astype(np.float32).reshape(-1, 4)
    b2 = np.asarray(b2).astype(np.float32).reshape(-1, 4)
    ex = np.float32(1.0 if use_legacy_coordinate else 0.0)
    if b1.shape[0] * b2.shape[0] == 0:
        return np.zeros((b1.shape[0], b2.shape[0]), dtype=np.float32)
    area1 = (b1[:, 2] - b1[:, 0] + ex) * (b1[:, 3] - b1[:, 1] + ex)
    area2 = (b2[:, 2] - b2[:, 0] + ex) * (b2[:, 3] - b2[:, 1] + ex)
    x_start = np.maximum(b1[:, None, 0], b2[None, :, 0])
    y_start = np.maximum(b1[:, None, 1], b2[None, :, 1])
    x_end = np.minimum(b1[:, None, 2], b2[None, :, 2])
    y_end = np.minimum(b1[:, None, 3], b2[None, :, 3])
    overlap = np.maximum(x_end - x_start + ex, np.float32(0)) * np.maximum(y_end - y_start + ex, np.float32(0))
    union = np.maximum(area1[:, None] + area2[None, :] - overlap, np.float32(1e-6))
    return overlap / union


def voc_match(dets, gts_all, use_legacy_coordinate=False):
    """per detection the largest IoU with the boxes of its (image, class) and the FIRST box that attains it
    (mean_ap.py:231-236): (iou_max fp32 [m], iou_arg int32 [m]); (0, -1) where there is no box"""
    m = len(dets)
    if len(gts_all) == 0 or m == 0:
        return np.zeros(m, dtype=np.float32), np.full(m, -1, dtype=np.int32)
    ious = bbox_overlaps_voc(np.asarray(dets)[:, :4], gts_all, use_legacy_coordinate)
    return ious.max(axis=1), ious.argmax(axis=1).astype(np.int32)


def voc_flags(dets, gts_all, n_regular, iou_thr, use_legacy_coordinate=False, match=None):
    """mean_ap.py:196-267 with area_ranges=None for one (image, class): ``gts_all`` = the regular boxes followed by the
    ignored ones, the first ``n_regular`` of them regular.  uint8 [m]: FLAG_TP, FLAG_FP, or FLAG_IGNORED for a detection
    whose best box is an ignored one.  ``match``: ``voc_match`` of the same boxes, when the caller has it (it does not
    depend on the threshold)."""
    dets = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    flags = np.full(len(dets), FLAG_FP, dtype=np.uint8)
    if len(gts_all) == 0 or len(dets) == 0:          # (mean_ap.py:220-229: only with no regular AND no ignored box)
        return flags
    iou_max, iou_arg = voc_match(dets, gts_all, use_legacy_coordinate) if match is None else match
    thr = np.float32(iou_thr)
    covered = np.zeros(len(gts_all), dtype=bool)
    for i in np.argsort(-dets[:, 4], kind='stable'):
        if iou_max[i] >= thr:
            g = iou_arg[i]
            if g >= n_regular:
                flags[i] = FLAG_IGNORED
            elif not covered[g]:
                covered[g] = True
                flags[i] = FLAG_TP
    return flags


def tpfp_default(dets, gts, gts_ignore=None, iou_thr=0.5, use_legacy_coordinate=False):
    """mean_ap.py:168-267 (area_ranges=None): (tp, fp) fp32 [m] of 0 / 1"""
    gts = np.asarray(gts, dtype=np.float32).reshape(-1, 4)
    ign = np.zeros((0, 4), np.float32) if gts_ignore is None else np.asarray(gts_ignore, dtype=np.float32).reshape(-1, 4)
    flags = voc_flags(dets, np.vstack((gts, ign)), len(gts), iou_thr, use_legacy_coordinate)
    return (flags == FLAG_TP).astype(np.float32), (flags == FLAG_FP).astype(np.float32)


def pack_voc_segments(results, annotations, num_classes):
    """a split as the arrays of oadg_voc_tpfp: one segment per (image, class), s = image * num_classes + class.
    dict(dets fp32 [D, 5], det_off int32 [S + 1], gts fp32 [G, 4] - per segment the regular boxes, then the ignored ones, each
    in annotation order (get_cls_results, mean_ap.py:270-294) -, gt_off int32 [S + 1], gt_reg int32 [S])"""
    n, C = len(results), int(num_classes)
    assert len(annotations) == n
    S = n * C
    flat = [np.reshape(r[c], (-1, 5)) for r in results for c in range(C)]
    cnt = np.fromiter((len(a) for a in flat), dtype=np.int64, count=S)
    dets = np.concatenate(flat).astype(np.float32, copy=False) if S else np.zeros((0, 5), np.float32)
    boxes, labels, imgs, ign = [], [], [], []
    for which, (bk, lk) in enumerate((('bboxes', 'labels'), ('bboxes_ignore', 'labels_ignore'))):
        anns = annotations if which == 0 else [a if a.get('labels_ignore', None) is not None else {} for a in annotations]
        b = [np.reshape(a.get(bk, ()), (-1, 4)) for a in anns]
        k = np.fromiter((len(x) for x in b), dtype=np.int64, count=n)
        boxes += b
        labels += [np.reshape(a.get(lk, ()), (-1,)) for a in anns]
        imgs.append(np.repeat(np.arange(n, dtype=np.int64), k))
        ign.append(np.full(int(k.sum()), which, dtype=np.int64))
    boxes = np.concatenate(boxes).astype(np.float32, copy=False) if n else np.zeros((0, 4), np.float32)
    labels = np.concatenate(labels).astype(np.int64) if n else np.zeros(0, np.int64)
    imgs, ign = np.concatenate(imgs), np.concatenate(ign)
    keep = (labels >= 0) & (labels < C)
    boxes, ign, seg = boxes[keep], ign[keep], (imgs * C + labels)[keep]
    order = np.lexsort((ign, seg))               # (stable: by segment, regular before ignored, annotation order within)
    assert dets.shape[0] < 2 ** 31 and boxes.shape[0] < 2 ** 31
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int32)           # noqa: E731
    return dict(dets=np.ascontiguousarray(dets), det_off=off(cnt), gts=np.ascontiguousarray(boxes[order]),
                gt_off=off(np.bincount(seg, minlength=S)), gt_reg=np.bincount(seg[ign == 0], minlength=S).astype(np.int32),
                num_classes=C)


def voc_flags_host(pack, iou_thrs, use_legacy_coordinate=False):
    """``voc_flags`` over every segment of a pack: uint8 [n_thr, D]"""
    dets, d_off, gts, g_off, g_reg = (pack[k] for k in ('dets', 'det_off', 'gts', 'gt_off', 'gt_reg'))
    out = np.empty((len(iou_thrs), len(dets)), dtype=np.uint8)
    for s in np.nonzero(np.diff(d_off))[0]:
        d, g = dets[d_off[s]:d_off[s + 1]], gts[g_off[s]:g_off[s + 1]]
        match = voc_match(d, g, use_legacy_coordinate)            # (once per segment, whatever the number of thresholds)
        for t, thr in enumerate(iou_thrs):
            out[t, d_off[s]:d_off[s + 1]] = voc_flags(d, g, g_reg[s], thr, use_legacy_coordinate, match)
    return out


def voc_flags_device(pack, iou_thrs, use_legacy_coordinate, device):
    """the same flags from csrc/voc_eval.hip: one upload of the pack through the staging path, ONE launch for the split and
    all thresholds, one download (``oadg_voc_tpfp.flags_device``, the module next to the package's import shim that holds the
    ctypes call of the kernel; see its docstring for why that call is not in hip_ops.py)."""
    import oadg_voc_tpfp
    return oadg_voc_tpfp.flags_device(pack, iou_thrs, use_legacy_coordinate, device)


def voc_accumulate(pack, flags, dataset=None):
    """mean_ap.py:381-436 for one threshold (``flags`` uint8 [D] in pack order) -> (mean_ap, per_class): per class the
    detections of all images by descending score (stable), fp32 cumulative tp / fp, recall over the REGULAR boxes, the AP
    of the mode (``dataset='voc07'``: 11 points), and the mean over the classes that have a regular box (0.0 without any)"""
    C, dets = pack['num_classes'], pack['dets']
    det_cls = np.repeat(np.arange(len(pack['det_off']) - 1, dtype=np.int64) % C, np.diff(pack['det_off']))
    reg_cls = np.bincount(np.arange(len(pack['gt_reg'])) % C, weights=pack['gt_reg'], minlength=C).astype(int)
    mode = 'area' if dataset != 'voc07' else '11points'
    eps = np.finfo(np.float32).eps
    per_class = []
    for c in range(C):
        idx = np.nonzero(det_cls == c)[0]
        num_gts = np.zeros(1, dtype=int)
        num_gts[0] = reg_cls[c]
        sort_inds = np.argsort(-dets[idx, 4], kind='stable')
        f = flags[idx][sort_inds]
        tp = np.cumsum((f == FLAG_TP).astype(np.float32)[None, :], axis=1)
        fp = np.cumsum((f == FLAG_FP).astype(np.float32)[None, :], axis=1)
        recalls = (tp / np.maximum(num_gts[:, np.newaxis], eps))[0, :]
        precisions = (tp / np.maximum((tp + fp), eps))[0, :]
        ap = np.float32(average_precision(recalls, precisions, mode))
        per_class.append(dict(num_gts=num_gts.item(), num_dets=len(idx), recall=recalls, precision=precisions, ap=ap))
    aps = [r['ap'] for r in per_class if r['num_gts'] > 0]
    return (np.array(aps).mean().item() if aps else 0.0), per_class


def eval_map_voc_thrs(results, annotations, num_classes, iou_thrs, dataset=None, use_legacy_coordinate=False, device=None):
    """``eval_map_voc`` for several thresholds from ONE pack (and, with a device, one launch): a list of (mean_ap, per_class)"""
    iou_thrs = [float(t) for t in iou_thrs]
    pack = pack_voc_segments(results, annotations, num_classes)
    out = []
    for k in range(0, len(iou_thrs), VOC_MAX_THRS):
        thrs = iou_thrs[k:k + VOC_MAX_THRS]
        if device is None:
            flags = voc_flags_host(pack, thrs, use_legacy_coordinate)
        else:
            flags = voc_flags_device(pack, thrs, use_legacy_coordinate, device)
        out += [voc_accumulate(pack, flags[t], dataset) for t in range(len(thrs))]
    return out


def eval_map_voc(results, annotations, num_classes, iou_thr=0.5, dataset=None, use_legacy_coordinate=False, device=None):
    """mean_ap.py:297-440 ``eval_map`` (scale_ranges=None, tpfp_default): (mean_ap, per_class) with per class
    dict(num_gts, num_dets, recall, precision, ap).  results: per image, per class, [k, 5]; annotations: per image the
    ``get_ann_info`` dict (bboxes, labels, and bboxes_ignore / labels_ignore when present).  ``dataset='voc07'``: 11-point AP.
    ``device=None``: the host ``tpfp_default``; a torch device: csrc/voc_eval.hip - the same flags, so the same numbers."""
    return eval_map_voc_thrs(results, annotations, num_classes, [iou_thr], dataset, use_legacy_coordinate, device)[0]


def voc_device():
    """the device ``SdgodDataset.evaluate`` matches on: the current GPU when the library and a GPU are present, else None
    (the host path)"""
    import torch
    from . import _lib
    if torch.cuda.is_available() and os.path.exists(_lib.LIB_PATH):
        return torch.device('cuda', torch.cuda.current_device())
    return None


def sdgod_evaluate(ds, results, metric='mAP', logger=None, device='auto', **eval_kwargs):
    """sdgod.py:29-89 for 'mAP': ``eval_map_voc`` with the legacy coordinates and, for a VOC2007 prefix, the 11-point AP,
    per threshold -> the flat ordered dict (``AP50``, ..., ``mAP``).  'recall' / scale_ranges are rejected by name."""
    metrics = list(metric) if isinstance(metric, (list, tuple)) else [metric]
    check_evaluate_args(type(ds), metrics, eval_kwargs)
    assert len(metrics) == 1, 'one metric (sdgod.py:56-58)'
    assert len(results) == len(ds), f'{len(results)} results for {len(ds)} images'
    thr = eval_kwargs.get('iou_thr', 0.5)
    thrs = [thr] if isinstance(thr, float) else list(thr)
    anns = [ds.get_ann_info(i) for i in range(len(ds))]
    dev = voc_device() if device == 'auto' else device
    per_thr = eval_map_voc_thrs(results, anns, _num_classes(ds), thrs, 'voc07' if ds.year == 2007 else None, True, dev)
    out = {}
    for t, (mean_ap, _) in zip(thrs, per_thr):
        out[f'AP{int(t * 100):02d}'] = round(mean_ap, 3)
    out['mAP'] = sum(m for m, _ in per_thr) / len(per_thr)
    return out


def evaluate(results, ds, metrics, num_classes, mmdet_style=False, device='auto'):
    """{'bbox': {AP, AP50, ...}} (COCO style) and / or {'mAP': ...} (VOC style AP@0.5).  ``mmdet_style``: the numbers and
    names of CocoDataset.evaluate (maxDets 100 / 300 / 1000, mAP at 1000 detections: mAP, mAP_50, ..., AR@100, ...) -
    what tools/test.py prints, comparable with the reference's logs; False: COCOeval's defaults (1 / 10 / 100), which is
    what the robustness benchmark aggregates (test_robustness.py coco_eval_with_return).  ``device``: where 'bbox' is matched -
    'auto': the current GPU when the library and a GPU are present (``voc_device``), else the host; None: the host."""
    out = {}
    idx = range(len(results))
    if 'bbox' in metrics:
        kw = dict(max_dets=MMDET_MAX_DETS, names=MMDET_METRICS) if mmdet_style else {}
        dev = voc_device() if device == 'auto' else device
        out['bbox'] = coco_eval_bbox(dataset_gt_anns(ds, idx), results, num_classes, device=dev, **kw)
    if 'mAP' in metrics:
        m, aps = eval_map(results, dataset_box_anns(ds, idx), num_classes)
        out['mAP'] = dict(mAP=m, per_class=aps)
    return out


# ------------------------------------------------------------------------------------------ per-image mAP
# tools/analysis_tools/analyze_results.py:14-46 ``bbox_map_eval``: the mean over ten thresholds of ``eval_map`` on ONE image
# (modern coordinates, area-mode AP, ignored boxes honoured), once per image of the split.  Here the whole split is packed once
# (pack_voc_segments), matched by the flags functions above - one launch per VOC_MAX_THRS thresholds on the device - and only
# the accumulation runs per image.
def voc_accumulate_per_image(pack, flags, dataset=None):
    """``voc_accumulate`` image by image: ``flags`` uint8 [D] (one threshold, pack order) -> float64 [n_images], or [T, D] ->
    [T, n_images]; for every image i exactly ``eval_map_voc([results[i]], [annotations[i]], ...)[0]``: per class of the image
    that has a regular box the AP of its own detections (stable descending score, fp32 cumulative tp / fp, recall over the
    regular boxes), their fp32 mean; 0.0 for an image without a regular box.  Classes without a regular box are skipped, as
    there.  A segment is sorted once for all thresholds, and the area under the envelope is ``average_precision``'s own
    arithmetic with the envelope taken by a running maximum instead of its loop (the same values: a maximum selects)."""
    C, dets, d_off, g_reg = pack['num_classes'], pack['dets'], pack['det_off'], pack['gt_reg']
    n = len(g_reg) // C
    flags = np.asarray(flags)
    many = flags.ndim == 2
    flags = flags if many else flags[None]
    T = len(flags)
    eps = np.finfo(np.float32).eps
    out = np.zeros((T, n), dtype=np.float64)
    aps = [[] for _ in range(n)]                                      # per image: a row [T] of fp32 APs per class with a box
    for s in np.flatnonzero(g_reg > 0):
        d0, d1 = d_off[s], d_off[s + 1]
        num_gts = np.zeros(1, dtype=int)
        num_gts[0] = g_reg[s]
        sort_inds = np.argsort(-dets[d0:d1, 4], kind='stable')
        f = flags[:, d0:d1][:, sort_inds]
        tp = np.cumsum((f == FLAG_TP).astype(np.float32), axis=1)
        fp = np.cumsum((f == FLAG_FP).astype(np.float32), axis=1)
        recalls = tp / np.maximum(num_gts[:, np.newaxis], eps)            # [T, m] float64, as voc_accumulate's
        precisions = tp / np.maximum((tp + fp), eps)                      # [T, m] float32
        if dataset == 'voc07':
            ap = [np.float32(average_precision(recalls[t], precisions[t], '11points')) for t in range(T)]
        else:
            zeros, ones = np.zeros((T, 1)), np.ones((T, 1))
            mrec = np.concatenate([zeros, recalls, ones], axis=1)
            mpre = np.concatenate([zeros, precisions, zeros], axis=1)
            mpre = np.maximum.accumulate(mpre[:, ::-1], axis=1)[:, ::-1]
            ap = []
            for t in range(T):
                ind = np.where(mrec[t, 1:] != mrec[t, :-1])[0]
                ap.append(np.float32(float(np.sum((mrec[t, ind + 1] - mrec[t, ind]) * mpre[t, ind + 1]))))
        aps[s // C].append(ap)
    for i, a in enumerate(aps):
        if a:
            out[:, i] = [np.array(col).mean().item() for col in zip(*a)]
    return out if many else out[0]


def per_image_map(results, annotations, num_classes, device=None):
    """``bbox_map_eval`` for every image of a split -> float64 [n_images]: the mean over np.linspace(.5, .95, 10) of the
    one-image ``eval_map`` (dataset=None, modern coordinates).  results: per image the per-class list (or the (bbox, segm)
    tuple: its bbox part); annotations: per image the ``get_ann_info`` dict.  ONE pack for the split and all thresholds;
    ``device=None``: ``voc_flags_host``; a torch device: csrc/voc_eval.hip - the same flags, so the same numbers."""
    results = [r[0] if isinstance(r, tuple) else r for r in results]
    thrs = [_f32_at_least(t) for t in IOU_THRS]
    pack = pack_voc_segments(results, annotations, num_classes)
    total = np.zeros(len(results), dtype=np.float64)
    for k in range(0, len(thrs), VOC_MAX_THRS):
        part = thrs[k:k + VOC_MAX_THRS]
        flags = voc_flags_host(pack, part, False) if device is None else voc_flags_device(pack, part, False, device)
        for per_thr in voc_accumulate_per_image(pack, flags):
            total = total + per_thr                                        # (sum(mean_aps): left to right, from 0)
    return total / len(thrs)


def _f32_at_least(t):
    """the smallest fp32 value >= ``t``.  ``bbox_map_eval`` hands eval_map np.float64 thresholds (np.linspace), so the
    reference compares its fp32 IoUs with them in float64 - under every numpy; for fp32 IoUs that is exactly the fp32
    comparison with this value, which the flags functions (and the kernel) take as it is: np.float32 of it changes nothing.
    (0.7 -> the fp32 above fp32(0.7): an IoU of exactly fp32(0.7) = 0.699999988 is below the float64 0.7.)"""
    f = np.float32(t)
    if float(f) < float(t):
        f = np.nextafter(f, np.float32(np.inf))
    return float(f)


def rank_images(maps, topk=20):
    """analyze_results.py:108-130: (good, bad) lists of (index, mAP) - a STABLE ascending sort (equal mAPs keep the order of
    the images), ``bad`` its first ``topk`` and ``good`` its last ``topk``; ``topk`` becomes len // 2 when 2 * topk > len"""
    assert topk > 0
    if topk * 2 > len(maps):
        topk = len(maps) // 2
    ranked = sorted(((i, float(m)) for i, m in enumerate(maps)), key=lambda kv: kv[1])
    return ranked[-topk:], ranked[:topk]       # (a split of one image: topk 0, and [-0:] is that image - as the reference)


# ------------------------------------------------------------------------------------------ confusion matrix
# tools/analysis_tools/confusion_matrix.py:59-142.  ``confusion_per_image`` is the reference's loop (the yardstick, pinned to
# the reference's own output by tests/golden/result_analysis_reference.npz); the product path packs the split once - one
# segment per IMAGE - and counts it on the host (vectorised per image) or in one launch of csrc/confusion.hip.  The same two
# rules are FIXED as in the VOC protocol: the thresholds are rounded to fp32 and compared in fp32.
def confusion_per_image(cm, gt_bboxes, gt_labels, result, score_thr=0, tp_iou_thr=0.5, nms_iou_thr=None):
    """confusion_matrix.py:95-142 ``analyze_per_img_dets``: adds one image to ``cm`` [(C + 1), (C + 1)] (row: label of the
    box, column: class of the detection, the last of each: background).  A detection of class c with score >= score_thr
    adds 1 to cm[gt_label[j], c] for EVERY box j with iou >= tp_iou_thr, whatever its label, or 1 to cm[C, c] without one; a
    box that no detection of its own label matched adds 1 to cm[gt_label, C].  Nothing is claimed, ``bboxes_ignore`` takes no
    part.  ``nms_iou_thr`` (truthy): mmcv's nms(..., score_threshold=score_thr) per class first."""
    C = cm.shape[0] - 1
    gt_bboxes = np.asarray(gt_bboxes, dtype=np.float32).reshape(-1, 4)
    gt_labels = _checked_labels(gt_labels, C)
    if len(result) != C or len(gt_labels) != len(gt_bboxes):
        raise ValueError(f'{len(result)} classes of detections for a {C}-class matrix, or labels that do not match the boxes')
    thr, s_thr = np.float32(tp_iou_thr), np.float32(score_thr)
    true_positives = np.zeros(len(gt_labels), dtype=np.int64)
    for det_label, det_bboxes in enumerate(result):
        det_bboxes = np.asarray(det_bboxes, dtype=np.float32).reshape(-1, 5)
        if nms_iou_thr:
            det_bboxes = nms_host(det_bboxes, nms_iou_thr, score_thr)
        ious = bbox_overlaps_voc(det_bboxes[:, :4], gt_bboxes)
        for i, det_bbox in enumerate(det_bboxes):
            det_match = 0
            if det_bbox[4] >= s_thr:
                for j, gt_label in enumerate(gt_labels):
                    if ious[i, j] >= thr:
                        det_match += 1
                        if gt_label == det_label:
                            true_positives[j] += 1
                        cm[gt_label, det_label] += 1
                if det_match == 0:
                    cm[C, det_label] += 1
    for num_tp, gt_label in zip(true_positives, gt_labels):
        if num_tp == 0:
            cm[gt_label, C] += 1


def _checked_labels(labels, num_classes):
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if len(labels) and (labels.min() < 0 or labels.max() >= num_classes):
        raise ValueError(f'box label outside [0, {num_classes}): {labels[(labels < 0) | (labels >= num_classes)][:4].tolist()} '
                         f'(the reference would wrap a negative index silently)')
    return labels


def nms_host(dets, iou_thr, score_thr=0):
    """mmcv.ops.nms(boxes, scores, iou_thr, score_threshold=score_thr) of one class: the rows [k, 5] with score > score_thr
    (strictly), by descending score (stable), greedily suppressed where the fp32 IoU = inter / (area_i + area_j - inter)
    (offset 0) is > iou_thr -> the kept rows, in that order"""
    d = np.asarray(dets, dtype=np.float32).reshape(-1, 5)
    d = d[d[:, 4] > np.float32(score_thr)]
    d = d[np.argsort(-d[:, 4], kind='stable')]
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    area = (x2 - x1) * (y2 - y1)
    thr = np.float32(iou_thr)
    removed = np.zeros(len(d), dtype=bool)
    keep = []
    for i in range(len(d)):
        if removed[i]:
            continue
        keep.append(i)
        w = np.maximum(np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]), np.float32(0))
        h = np.maximum(np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]), np.float32(0))
        inter = w * h
        with np.errstate(divide='ignore', invalid='ignore'):
            removed[i + 1:] |= inter / ((area[i] + area[i + 1:]) - inter) > thr
    return d[keep]


def _aligned16(a):
    """``a`` contiguous at an address that is a multiple of 16 (the kernels read boxes 16 bytes at a time)"""
    a = np.ascontiguousarray(a)
    if a.ctypes.data % 16 == 0:
        return a
    buf = np.empty(a.nbytes + 16, dtype=np.uint8)
    off = -buf.ctypes.data % 16
    out = buf[off:off + a.nbytes].view(a.dtype).reshape(a.shape)
    out[...] = a
    return out


def pack_confusion_segments(results, annotations, num_classes, score_thr=0):
    """a split as the arrays of oadg_confusion_count: one segment per IMAGE.  dict(dets fp32 [D, 4] - per image class after
    class, within a class in the result's order, only the rows with score >= score_thr (fp32) -, det_cls int32 [D], det_off
    int32 [n + 1], gts fp32 [G, 4] in annotation order, gt_lab int32 [G], gt_off int32 [n + 1], num_classes); the box arrays
    start at multiples of 16 bytes.  annotations: per image the ``get_ann_info`` dict (bboxes, labels; the ignored boxes take
    no part).  ValueError: a label outside [0, num_classes), a result that has not num_classes arrays, lengths that differ."""
    n, C = len(results), int(num_classes)
    if len(annotations) != n:
        raise ValueError(f'{n} results for {len(annotations)} annotations')
    s_thr = np.float32(score_thr)
    dets, cls, d_cnt, boxes, labels, g_cnt = [], [], np.zeros(n, np.int64), [], [], np.zeros(n, np.int64)
    for i, (res, ann) in enumerate(zip(results, annotations)):
        if isinstance(res, tuple):
            res = res[0]
        if len(res) != C:
            raise ValueError(f'image {i}: {len(res)} classes of detections, num_classes is {C}')
        for c, d in enumerate(res):
            d = np.asarray(d, dtype=np.float32).reshape(-1, 5)
            d = d[d[:, 4] >= s_thr]
            dets.append(d[:, :4])
            cls.append(np.full(len(d), c, dtype=np.int32))
            d_cnt[i] += len(d)
        b = np.asarray(ann['bboxes'], dtype=np.float32).reshape(-1, 4)
        l = _checked_labels(ann['labels'], C)
        if len(b) != len(l):
            raise ValueError(f'image {i}: {len(b)} boxes with {len(l)} labels')
        boxes.append(b)
        labels.append(l.astype(np.int32))
        g_cnt[i] = len(b)
    cat = lambda xs, shape, dt: np.concatenate(xs + [np.zeros(shape, dt)])          # noqa: E731
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.int32)           # noqa: E731
    assert d_cnt.sum() < 2 ** 31 and g_cnt.sum() < 2 ** 31
    return dict(dets=_aligned16(cat(dets, (0, 4), np.float32)), det_cls=np.ascontiguousarray(cat(cls, (0,), np.int32)),
                det_off=off(d_cnt), gts=_aligned16(cat(boxes, (0, 4), np.float32)),
                gt_lab=np.ascontiguousarray(cat(labels, (0,), np.int32)), gt_off=off(g_cnt), num_classes=C)


def confusion_counts_host(pack, tp_iou_thr=0.5):
    """the counts of a pack on the host -> int64 [(C + 1), (C + 1)]: ``confusion_per_image``'s rules, one IoU matrix per
    image (all classes of its detections together)"""
    C = pack['num_classes']
    cm = np.zeros((C + 1, C + 1), dtype=np.int64)
    thr = np.float32(tp_iou_thr)
    d_off, g_off = pack['det_off'], pack['gt_off']
    for i in range(len(d_off) - 1):
        d, c = pack['dets'][d_off[i]:d_off[i + 1]], pack['det_cls'][d_off[i]:d_off[i + 1]].astype(np.int64)
        g, l = pack['gts'][g_off[i]:g_off[i + 1]], pack['gt_lab'][g_off[i]:g_off[i + 1]].astype(np.int64)
        hit = bbox_overlaps_voc(d, g) >= thr                                       # [m, k]
        di, gj = np.nonzero(hit)
        np.add.at(cm, (l[gj], c[di]), 1)
        np.add.at(cm, (np.full(int((~hit.any(axis=1)).sum()), C), c[~hit.any(axis=1)]), 1)
        found = (hit & (c[:, None] == l[None, :])).any(axis=0)
        np.add.at(cm, (l[~found], np.full(int((~found).sum()), C)), 1)
    return cm


def confusion_counts_device(pack, tp_iou_thr, device):
    """the same counts from csrc/confusion.hip: one upload of the pack through the staging path, ONE launch for the split, one
    download (``oadg_confusion.counts_device``, the module next to the package's import shim that holds the ctypes call of
    the kernel; see its docstring for why that call is not in hip_ops.py)."""
    import oadg_confusion
    return oadg_confusion.counts_device(pack, tp_iou_thr, device)


def dataset_ann_infos(dataset, indices=None):
    """per image the ``get_ann_info`` dict of a file dataset; ``boxes`` of the synthetic one in that form"""
    idx = range(len(dataset)) if indices is None else indices
    if hasattr(dataset, 'get_ann_info'):
        return [dataset.get_ann_info(i) for i in idx]
    return [dict(zip(('bboxes', 'labels'), dataset.boxes(i))) for i in idx]


def calculate_confusion_matrix(dataset, results, score_thr=0, nms_iou_thr=None, tp_iou_thr=0.5, device='auto'):
    """confusion_matrix.py:59-92: the float64 [(C + 1), (C + 1)] matrix of a split (C = len(dataset.CLASSES)).  Results
    given as (bbox, segm) tuples use the bbox part.  A truthy ``nms_iou_thr`` reruns NMS per (image, class) first, with
    mmcv's nms(..., score_threshold=score_thr) semantics - on the batched NMS kernel when matching on a device.  ``device``:
    'auto' counts on the current GPU when the library and a GPU are present (``voc_device``), None on the host - the same
    numbers either way."""
    C = _num_classes(dataset)
    if len(dataset) != len(results):
        raise ValueError(f'{len(results)} results for {len(dataset)} images')
    results = [r[0] if isinstance(r, tuple) else r for r in results]
    dev = voc_device() if device == 'auto' else device
    if nms_iou_thr:
        if dev is None:
            results = [[nms_host(d, nms_iou_thr, score_thr) for d in res] for res in results]
        else:
            import oadg_confusion
            results = oadg_confusion.nms_results_device(results, nms_iou_thr, score_thr, dev)
    pack = pack_confusion_segments(results, dataset_ann_infos(dataset), C, score_thr)
    counts = confusion_counts_host(pack, tp_iou_thr) if dev is None else confusion_counts_device(pack, tp_iou_thr, dev)
    return counts.astype(np.float64)


# ------------------------------------------------------------------------------------------ proposal recall
# mmdet/core/evaluation/recall.py as CocoDataset.evaluate 'proposal_fast' (coco.py:312-334, 426-435) and the VOC-style
# datasets' 'recall' (sdgod.py:90-105, custom.py:359-369) drive it: per image and per proposal budget Hosang's greedy
# bipartite matching of boxes to proposals, then the fraction of boxes matched at each IoU threshold.  The host functions
# below are the yardstick (pinned to the reference's own output by tests/golden/recall_reference.npz) and the path without a
# GPU; csrc/recall.hip computes the same matched IoUs for a whole split and all budgets in one launch.  Two rules are FIXED
# here where the reference leaves them to numpy: equal scores are ordered lowest index first (a stable
# sort; the reference's ``argsort()[::-1]`` is whatever numpy's quicksort leaves), and an fp32 IoU is promoted to fp64 before
# it is compared with the fp64 threshold (numpy 2's rule; numpy 1 compared in fp32).
def pack_recall(gts, proposals, proposal_nums):
    """a split as the arrays of oadg_recall_match.  gts: per image [g, 4] boxes or None; proposals: per image [n, 5] (sorted
    here by descending score, equal scores lowest index first) or [n, 4] (kept in their order), cut to ``proposal_nums[-1]``
    (recall.py:94-109).  dict(props fp32 [P, 4], prop_off int32 [N + 1], gts fp32 [G, 4], gt_off int32 [N + 1], nums int32
    [K] = min(num, proposal_nums[-1]), the budget that ``ious[:, :num]`` really leaves); the box arrays start at multiples of
    16 bytes.  ValueError: a coordinate that is not finite in fp32, or a NaN score."""
    nums = [int(v) for v in np.asarray(proposal_nums).reshape(-1)]
    if not nums or min(nums) < 0:
        raise ValueError(f'proposal_nums must hold at least one budget, none negative (got {nums})')
    if len(gts) != len(proposals):
        raise ValueError(f'{len(gts)} images of boxes for {len(proposals)} images of proposals')
    last = nums[-1]
    props, boxes, p_cnt, g_cnt = [], [], [], []
    for i, (g, p) in enumerate(zip(gts, proposals)):
        p = np.asarray(p)
        if p.ndim == 2 and p.shape[1] == 5:
            if np.isnan(p[:, 4]).any():
                raise ValueError(f'image {i}: a proposal score is NaN (it has no place in the evaluation order)')
            p = p[np.argsort(-p[:, 4], kind='stable')]
        elif p.size == 0:
            p = np.zeros((0, 4), np.float32)
        elif p.ndim != 2 or p.shape[1] != 4:
            raise ValueError(f'image {i}: proposals of shape {p.shape}, expected [n, 5] or [n, 4]')
        p = p[:last, :4].astype(np.float32)
        g = np.zeros((0, 4), np.float32) if g is None else np.asarray(g).astype(np.float32).reshape(-1, 4)
        if not (np.isfinite(p).all() and np.isfinite(g).all()):
            raise ValueError(f'image {i}: a box or proposal coordinate is not finite')
        props.append(p)
        boxes.append(g)
        p_cnt.append(len(p))
        g_cnt.append(len(g))
    cat = lambda xs: np.concatenate(xs + [np.zeros((0, 4), np.float32)])            # noqa: E731
    off = lambda c: np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int32)           # noqa: E731
    assert sum(p_cnt) < 2 ** 31 and sum(g_cnt) < 2 ** 31
    return dict(props=_aligned16(cat(props)), prop_off=off(p_cnt), gts=_aligned16(cat(boxes)), gt_off=off(g_cnt),
                nums=np.array([min(v, last) for v in nums], dtype=np.int32))


def recall_ious_host(pack, use_legacy_coordinate=False):
    """recall.py:17-34, the inner loop of ``_recalls`` over ``bbox_overlaps_voc``, for every image and budget of a pack ->
    fp32 [K, G]: row k, slice gt_off[i] .. gt_off[i + 1] holds ``gt_ious`` of image i IN ROUND ORDER (round j: the largest
    entry of the matrix - numpy's argmax: the lowest column per box, then the lowest box -, whose row and column become -1;
    -1 itself once the columns have run out; 0 for every box of an image without a proposal)"""
    props, p_off, gts, g_off, nums = (pack[k] for k in ('props', 'prop_off', 'gts', 'gt_off', 'nums'))
    out = np.zeros((len(nums), len(gts)), dtype=np.float32)
    for i in range(len(g_off) - 1):
        g0, g1 = g_off[i], g_off[i + 1]
        if g1 == g0:
            continue
        all_ious = bbox_overlaps_voc(gts[g0:g1], props[p_off[i]:p_off[i + 1]], use_legacy_coordinate)
        for k, proposal_num in enumerate(nums):
            ious = all_ious[:, :proposal_num].copy()
            gt_ious = np.zeros((ious.shape[0]))
            if ious.size == 0:
                continue
            for j in range(ious.shape[0]):
                gt_max_overlaps = ious.argmax(axis=1)
                max_ious = ious[np.arange(0, ious.shape[0]), gt_max_overlaps]
                gt_idx = max_ious.argmax()
                gt_ious[j] = max_ious[gt_idx]
                box_idx = gt_max_overlaps[gt_idx]
                ious[gt_idx, :] = -1
                ious[:, box_idx] = -1
            out[k, g0:g1] = gt_ious
    return out


def recall_ious_device(pack, use_legacy_coordinate, device, timings=None):
    """the same IoUs from csrc/recall.hip: one upload of the pack through the staging path, ONE launch for the split and all
    budgets, one download (``oadg_recall.ious_device``, the module next to the package's import shim that holds the ctypes
    call of the kernel; see its docstring for why that call is not in hip_ops.py)."""
    import oadg_recall
    return oadg_recall.ious_device(pack, pack['nums'], use_legacy_coordinate, device, timings=timings)


def recalls_from_ious(ious, iou_thrs):
    """recall.py:36-41: ``ious`` fp32 [K, G] (any order within a row) -> float64 [K, n_thrs], the fraction of the G boxes whose
    matched IoU - promoted to fp64 - is >= the fp64 threshold; nan everywhere when there is no box at all (0 / 0.0)"""
    ious = np.asarray(ious, dtype=np.float32)
    thrs = np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    total_gt_num = ious.shape[1]
    _ious = np.fliplr(np.sort(ious, axis=1)).astype(np.float64)
    recalls = np.zeros((ious.shape[0], thrs.size))
    with np.errstate(divide='ignore', invalid='ignore'):
        for i, thr in enumerate(thrs):
            recalls[:, i] = (_ious >= np.float64(thr)).sum(axis=1) / np.float64(total_gt_num)
    return recalls


def _print_log(msg, logger=None):
    """mmcv.utils.print_log: None prints, 'silent' does not, a logging.Logger logs at INFO"""
    if logger is None:
        print(msg)
    elif logger != 'silent':
        logger.info(msg)


def print_recall_summary(recalls, proposal_nums, iou_thrs, row_idxs=None, col_idxs=None, logger=None):
    """recall.py:117-147 as a plain text table (one row per budget, one column per threshold, 3 decimals) -> the text"""
    proposal_nums = np.asarray(proposal_nums, dtype=np.int32).reshape(-1)
    iou_thrs = np.asarray(iou_thrs).reshape(-1)
    row_idxs = np.arange(proposal_nums.size) if row_idxs is None else np.asarray(row_idxs)
    col_idxs = np.arange(iou_thrs.size) if col_idxs is None else np.asarray(col_idxs)
    rows = [[''] + [str(t) for t in iou_thrs[col_idxs].tolist()]]
    for i, num in enumerate(proposal_nums[row_idxs]):
        rows.append([str(int(num))] + [f'{val:.3f}' for val in np.asarray(recalls)[row_idxs[i], col_idxs].tolist()])
    width = [max(len(r[c]) for r in rows) for c in range(len(rows[0]))]
    rule = '+' + '+'.join('-' * (w + 2) for w in width) + '+'
    lines = [rule]
    for k, r in enumerate(rows):
        lines.append('| ' + ' | '.join(v.ljust(w) for v, w in zip(r, width)) + ' |')
        if k == 0:
            lines.append(rule)
    lines.append(rule)
    text = '\n'.join(lines)
    _print_log('\n' + text, logger=logger)
    return text


def eval_recalls(gts, proposals, proposal_nums=None, iou_thrs=0.5, logger=None, use_legacy_coordinate=False, device=None):
    """recall.py:65-114 ``eval_recalls``: float64 [n_nums, n_thrs].  gts: per image [g, 4] or None; proposals: per image
    [n, 5] or [n, 4]; ``proposal_nums``: an int or a sequence of them (the last one also cuts the proposals, as there);
    ``iou_thrs``: None (0.5), a float or a sequence.  ``device=None``: the host loop (``recall_ious_host``); a torch device:
    csrc/recall.hip - the same matched IoUs, so the same numbers."""
    if proposal_nums is None:
        raise TypeError('eval_recalls needs proposal_nums (an int or a sequence of ints)')
    nums = [proposal_nums] if isinstance(proposal_nums, (int, np.integer)) else list(np.asarray(proposal_nums).reshape(-1))
    thrs = np.array([0.5]) if iou_thrs is None else np.asarray(iou_thrs, dtype=np.float64).reshape(-1)
    pack = pack_recall(gts, proposals, nums)
    if device is None:
        ious = recall_ious_host(pack, use_legacy_coordinate)
    else:
        ious = recall_ious_device(pack, use_legacy_coordinate, device)
    recalls = recalls_from_ious(ious, thrs)
    print_recall_summary(recalls, nums, thrs, logger=logger)
    return recalls


def coco_recall_boxes(ds):
    """coco.py:313-329: per image the boxes ``fast_eval_recall`` counts - every annotation of the image that is neither a
    crowd nor marked ``ignore``, whatever its category, x y w h -> x1 y1 x2 y2 in fp32; a synthetic dataset: its boxes"""
    out = []
    for i in range(len(ds)):
        if hasattr(ds, 'coco'):
            anns = ds.coco.load_anns(ds.coco.get_ann_ids(img_ids=[ds.data_infos[i]['id']]))
            b = [[a['bbox'][0], a['bbox'][1], a['bbox'][0] + a['bbox'][2], a['bbox'][1] + a['bbox'][3]] for a in anns
                 if not (a.get('ignore', False) or a.get('iscrowd', 0))]
            out.append(np.array(b, dtype=np.float32).reshape(-1, 4))
        else:
            out.append(np.asarray(ds.boxes(i)[0], dtype=np.float32).reshape(-1, 4))
    return out


def fast_eval_recall(ds, results, proposal_nums, iou_thrs, logger=None, device='auto'):
    """coco.py:312-334 ``CocoDataset.fast_eval_recall``: the mean over ``iou_thrs`` of ``eval_recalls`` (modern extents)
    against ``coco_recall_boxes`` -> float64 [n_nums]"""
    dev = voc_device() if device == 'auto' else device
    recalls = eval_recalls(coco_recall_boxes(ds), results, proposal_nums, iou_thrs, logger=logger, device=dev)
    return recalls.mean(axis=1)


PROPOSAL_METRICS = ('proposal', 'proposal_fast', 'recall')


def _proposal_arrays(results, metric):
    """results of an RPN run: one [n, 5] (or [n, 4]) array per image"""
    for i, r in enumerate(results):
        if isinstance(r, (list, tuple)):
            raise TypeError(f"metric '{metric}' takes one [n, 5] array of proposals per image (the results of an RPN "
                            f"detector); image {i} holds a per-class {type(r).__name__} of {len(r)} arrays - those are "
                            f"detections: use metric 'proposal' (COCO style, class-agnostic) for them")
    return [np.asarray(r) for r in results]


def proposal_evaluate(ds, results, metric, logger=None, device='auto', proposal_nums=(100, 300, 1000), iou_thrs=None,
                      iou_thr=0.5, metric_items=None):
    """The three metrics of the reference's ``dataset.evaluate`` that score PROPOSALS -> its flat ordered dict.

    'proposal_fast' (coco.py:426-435; COCO-format and synthetic datasets): ``AR@{num}`` per budget, unrounded floats, the mean
      over ``iou_thrs`` (default IOU_THRS) of ``eval_recalls``; results: one [n, 5] array per image.
    'recall' (sdgod.py:90-105 - legacy "+ 1" extents for SdgodDataset -, custom.py:359-369 - modern - for XMLDataset and the
      synthetic set): ``recall@{num}@{thr}`` per pair and, with more than one ``iou_thr``, ``AR@{num}``; boxes are
      ``get_ann_info(i)['bboxes']``; results: one array per image.
    'proposal' (coco.py:437-511: COCOeval with useCats = 0; COCO-format and synthetic datasets): per image all boxes are one
      category and all detections one list - a per-class result concatenated in class order, or an [n, 5] array -, ordered
      by ``pack_coco_segments``' stable sort and cut to the last budget; ``AR@100, AR@300, AR@1000, AR_s@1000, AR_m@1000,
      AR_l@1000`` (or ``metric_items``) as floats of 3 decimals - the names belong to POSITIONS of the summary, as in the
      reference: with other ``proposal_nums`` 'AR@100' is the recall at proposal_nums[0].
    ``device``: 'auto' matches on the current GPU when the library and a GPU are present (``voc_device``), None on the host -
    the same numbers either way."""
    if not isinstance(metric, str):
        assert len(metric) == 1, 'one metric'
        metric = metric[0]
    if metric not in PROPOSAL_METRICS:
        raise KeyError(f'metric {metric} is not a proposal metric {PROPOSAL_METRICS}')
    if len(results) != len(ds):
        raise ValueError(f'{len(results)} results for {len(ds)} images')
    voc_style = any(p is VOC_EVAL for p in getattr(type(ds), 'EVAL_PROTOCOLS', ()))
    coco_style = any(p is COCO_EVAL for p in getattr(type(ds), 'EVAL_PROTOCOLS', ()))
    if (metric == 'recall' and not voc_style) or (metric != 'recall' and not coco_style):
        raise KeyError(f'metric {metric} is not supported by {type(ds).__name__}')
    dev = voc_device() if device == 'auto' else device
    nums = [int(v) for v in proposal_nums]
    out = {}          # (insertion-ordered)
    if metric == 'proposal_fast':
        thrs = IOU_THRS if iou_thrs is None else iou_thrs
        ar = fast_eval_recall(ds, _proposal_arrays(results, metric), nums, thrs, logger='silent', device=dev)
        for i, num in enumerate(nums):
            out[f'AR@{num}'] = float(ar[i])
        _print_log(''.join(f'\nAR@{num}\t{ar[i]:.4f}' for i, num in enumerate(nums)), logger=logger)
    elif metric == 'recall':
        thrs = [iou_thr] if isinstance(iou_thr, float) else list(iou_thr)
        boxes = [a['bboxes'] for a in dataset_ann_infos(ds)]
        legacy = bool(getattr(type(ds), 'RECALL_LEGACY_COORDINATE', False))     # (SdgodDataset: sdgod.py:98; custom.py: modern)
        recalls = eval_recalls(boxes, _proposal_arrays(results, metric), nums, thrs, logger=logger,
                               use_legacy_coordinate=legacy, device=dev)
        for i, num in enumerate(nums):
            for j, t in enumerate(thrs):
                out[f'recall@{num}@{t}'] = float(recalls[i, j])
        if recalls.shape[1] > 1:
            ar = recalls.mean(axis=1)
            for i, num in enumerate(nums):
                out[f'AR@{num}'] = float(ar[i])
    else:
        if iou_thrs is not None and not np.array_equal(np.asarray(iou_thrs, dtype=np.float64), IOU_THRS):
            raise NotImplementedError("evaluation key 'iou_thrs' of metric 'proposal' is not built: the COCO accumulation "
                                      "here runs at IOU_THRS (.50:.05:.95)")
        if len(nums) != 3:
            raise ValueError(f"metric 'proposal' takes three proposal_nums (COCOeval's maxDets), got {nums}")
        items = MMDET_METRICS[6:] if metric_items is None else \
            ([metric_items] if isinstance(metric_items, str) else list(metric_items))
        for it in items:
            if it not in MMDET_METRICS:
                raise KeyError(f'metric item {it} is not supported')
        one_class = [[np.concatenate([np.asarray(c, np.float64).reshape(-1, 5) for c in r]) if isinstance(r, (list, tuple))
                      else np.asarray(r, np.float64).reshape(-1, 5)] for r in results]
        gt = [[dict(g, category=0) for g in per_img] for per_img in dataset_gt_anns(ds)]
        stats = coco_eval_bbox(gt, one_class, 1, max_dets=nums, names=MMDET_METRICS, device=dev)
        for it in items:
            out[it] = float(f'{stats[it]:.3f}')
    return out


# ------------------------------------------------------------------------------------------ dataset.evaluate
# What ``dataset.evaluate(results, metric=..., **eval_kwargs)`` of the reference takes per protocol, and what of it this
# build computes.  A metric or keyword of the reference that is not built is rejected BY NAME (NotImplementedError), one the
# reference does not know either is a KeyError / TypeError as there - nothing is dropped silently.
COCO_EVAL = dict(metrics=('bbox',), absent=('segm', 'proposal', 'proposal_fast'),
                 kwargs=('proposal_nums', 'metric_items'),
                 absent_kwargs=('jsonfile_prefix', 'outfile_prefix', 'classwise', 'iou_thrs', 'picked_label'))
VOC_EVAL = dict(metrics=('mAP',), absent=('recall',), kwargs=('proposal_nums', 'iou_thr'), absent_kwargs=('scale_ranges',))


def check_evaluate_args(cls, metrics, eval_kwargs):
    """the metrics and forwarded keywords of an ``evaluation`` config against what ``cls.evaluate`` computes: raises with
    the offending name (and the dataset class), so that a run stops before any training work instead of after an epoch"""
    protos = getattr(cls, 'EVAL_PROTOCOLS', None)
    if not protos:
        raise NotImplementedError(f'{cls.__name__} has no evaluate()')
    for m in metrics:
        if not any(m in p['metrics'] for p in protos):
            if any(m in p['absent'] for p in protos):
                where = f"; evaluation.proposal_evaluate(dataset, results, '{m}') and tools/test.py --eval {m} compute it" \
                    if m in PROPOSAL_METRICS else ''
                raise NotImplementedError(f"metric '{m}' of {cls.__name__}.evaluate is not built "
                                          f"(built: {[x for p in protos for x in p['metrics']]}){where}")
            raise KeyError(f'metric {m} is not supported by {cls.__name__}')
    used = [p for p in protos if any(m in p['metrics'] for m in metrics)]
    for k in eval_kwargs:
        if not any(k in p['kwargs'] for p in used):
            if any(k in p['absent_kwargs'] for p in used):
                raise NotImplementedError(f"evaluation key '{k}' ({cls.__name__}.evaluate(..., {k}=...)) is not built "
                                          f"(built: {sorted({x for p in used for x in p['kwargs']})})")
            raise TypeError(f"{cls.__name__}.evaluate() got an unexpected keyword argument '{k}'")


def _num_classes(ds):
    return len(getattr(ds, 'CLASSES', None) or range(getattr(ds, 'num_classes', 8)))


def dataset_evaluate(ds, results, metric='bbox', logger=None, device='auto', **eval_kwargs):
    """``CocoDataset.evaluate`` (mmdet/datasets/coco.py:364-573, which CityscapesDataset delegates 'bbox' to) and
    ``VOCDataset.evaluate`` (voc.py:28-106) on this module's evaluators: the flat ordered dict the reference returns
    (``SdgodDataset.evaluate`` is ``sdgod_evaluate`` above).

    'bbox': ``bbox_mAP, bbox_mAP_50, bbox_mAP_75, bbox_mAP_s, bbox_mAP_m, bbox_mAP_l`` as floats of 3 decimals (or the
    ``metric_items`` asked for) and ``bbox_mAP_copypaste`` - the mmdet-style numbers: maxDets = ``proposal_nums`` =
    (100, 300, 1000), mAP at the last of them.  'mAP': ``AP50`` (``AP{100 * iou_thr}`` per threshold, 3 decimals) and ``mAP``
    (their mean) from ``eval_map``.  ``logger`` is the reference's parameter: nothing is printed here, the caller (EvalHook,
    tools/test.py) prints what it returns.  ``device`` ('bbox' only): 'auto' matches on the current GPU when the library and a
    GPU are present (``voc_device``, as ``sdgod_evaluate``), None on the host - the same numbers either way."""
    metrics = list(metric) if isinstance(metric, (list, tuple)) else [metric]
    check_evaluate_args(type(ds), metrics, eval_kwargs)
    assert len(results) == len(ds), f'{len(results)} results for {len(ds)} images'
    nc = _num_classes(ds)
    out = {}          # (insertion-ordered)
    for m in metrics:
        if m == 'bbox':
            nums = tuple(eval_kwargs.get('proposal_nums', MMDET_MAX_DETS))
            items = eval_kwargs.get('metric_items', None)
            items = ([items] if isinstance(items, str) else list(items)) if items is not None else MMDET_METRICS[:6]
            for it in items:
                if it not in MMDET_METRICS:
                    raise KeyError(f'metric item {it} is not supported')
            dev = voc_device() if device == 'auto' else device
            stats = coco_eval_bbox(dataset_gt_anns(ds), results, nc, max_dets=nums, names=MMDET_METRICS, device=dev)
            for it in items:
                out[f'bbox_{it}'] = float(f'{stats[it]:.3f}')
            out['bbox_mAP_copypaste'] = ' '.join(f'{stats[k]:.3f}' for k in MMDET_METRICS[:6])
        else:
            thr = eval_kwargs.get('iou_thr', 0.5)
            thrs = [thr] if isinstance(thr, float) else list(thr)
            anns = dataset_box_anns(ds)
            means = []
            for t in thrs:
                mean_ap, _ = eval_map(results, anns, nc, iou_thr=t)
                means.append(mean_ap)
                out[f'AP{int(t * 100):02d}'] = round(mean_ap, 3)
            out['mAP'] = sum(means) / len(means)
    return out


# ------------------------------------------------------------------------------------------ corruption benchmark
CORRUPTION_SETS = {   # tools/analysis_tools/test_robustness.py:225-256
    'all': ['gaussian_noise', 'shot_noise', 'impulse_noise', 'defocus_blur', 'glass_blur', 'motion_blur', 'zoom_blur',
            'snow', 'frost', 'fog', 'brightness', 'contrast', 'elastic_transform', 'pixelate', 'jpeg_compression',
            'speckle_noise', 'gaussian_blur', 'spatter', 'saturate'],
    'noise': ['gaussian_noise', 'shot_noise', 'impulse_noise'],
    'blur': ['defocus_blur', 'glass_blur', 'motion_blur', 'zoom_blur'],
    'weather': ['snow', 'frost', 'fog', 'brightness'],
    'digital': ['contrast', 'elastic_transform', 'pixelate', 'jpeg_compression'],
    'holdout': ['speckle_noise', 'gaussian_blur', 'spatter', 'saturate'],
}
CORRUPTION_SETS['benchmark'] = CORRUPTION_SETS['all'][:15]


def select_corruptions(names, severities):
    """the if-chain of test_robustness.py:225-256: first matching group wins; 'None' = clean data only"""
    for key in ('all', 'benchmark', 'noise', 'blur', 'weather', 'digital', 'holdout'):
        if key in names:
            return list(CORRUPTION_SETS[key]), list(severities)
    if 'None' in names:
        return ['None'], [0]
    return list(names), list(severities)


def corrupted_img_prefix(img_prefix, corruption, severity):
    """--load-dataset corrupted (test_robustness.py:283-299): the pre-generated ``cityscapes-c`` / ``coco-c`` trees"""
    if '/cityscapes/' in img_prefix:
        return f"{img_prefix.replace('cityscapes', 'cityscapes-c')}{corruption}/{severity}/"
    if '/cityscapes-c/' in img_prefix:
        return f'{img_prefix}{corruption}/{severity}/'
    if '/coco/' in img_prefix:
        return f"{img_prefix.replace('coco', 'coco-c')}{corruption}/{severity}/"
    if '/coco-c/' in img_prefix:
        return f'{img_prefix}{corruption}/{severity}/'
    raise NotImplementedError("set load_dataset as 'corrupted' but use original dataset.")


def aggregate_robustness(eval_output, task='bbox', metrics=None, aggregate='benchmark'):
    """robustness_eval.py:37-118 get_coco_style_results: eval_output[corruption][severity][task][metric] ->
    (P, mPC, rPC) arrays over ``metrics``: P = clean performance (first corruption, severity 0), mPC = mean over the
    corruptions (the first 15 for 'benchmark') and severities 1..5, rPC = mPC / P."""
    assert aggregate in ('benchmark', 'all')
    metrics = list(METRICS) if metrics is None else list(metrics)
    res = np.zeros((len(eval_output), 6, len(metrics)), dtype='float32')
    for ci, corruption in enumerate(eval_output):
        for severity in eval_output[corruption]:
            for mj, name in enumerate(metrics):
                res[ci, int(severity), mj] = eval_output[corruption][severity][task][name]
    P = res[0, 0, :]
    mPC = np.mean(res[:15, 1:, :], axis=(0, 1)) if aggregate == 'benchmark' else np.mean(res[:, 1:, :], axis=(0, 1))
    with np.errstate(divide='ignore', invalid='ignore'):
        rPC = mPC / P
    return dict(P=dict(zip(metrics, P.tolist())), mPC=dict(zip(metrics, mPC.tolist())),
                rPC=dict(zip(metrics, rPC.tolist())), table=res)
