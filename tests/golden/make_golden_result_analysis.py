"""Generate tests/golden/result_analysis_reference.npz from the reference's own result-analysis functions (run by path,
refload.py):
  * analyze_per_img_dets    tools/analysis_tools/confusion_matrix.py:95-142   (nms_iou_thr=None), summed over the images for
                            (score_thr, tp_iou_thr) in CASES
  * bbox_map_eval           tools/analysis_tools/analyze_results.py:14-46 - that file does not import here
                            (mmcv.runner.hooks), so mean_ap.eval_map is driven exactly as it drives it: per image, the ten
                            thresholds np.linspace(.5, .95, 10), iou_thr=thr, logger='silent', sum / len.
Seeded inputs: 10 images, 3 classes, 0-6 regular and 0-2 ignored boxes per image; per (image, class) jittered copies of the
boxes of that class, a second tighter copy (two detections on one box), jittered copies of boxes of OTHER labels (the
off-diagonal cells), one detection spanning two overlapping boxes, and random boxes; all scores distinct (the reference's
unstable sorts cannot matter), half of the coordinates fractional.
The shims of make_golden_voc_eval.py let mean_ap.py import; matplotlib.pyplot and numpy.ma are imported BEFORE np.bool is
set (numpy.ma does not import with it).
Run here only:  python tests/golden/make_golden_result_analysis.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import refload  # noqa: E402

N_IMG, N_CLS, W, H = 10, 3, 200, 120
CASES = ((0.0, 0.5), (0.3, 0.5), (0.3, 0.75))          # (score_thr, tp_iou_thr)
MAX_DETS = 14


def _boxes(rs, n, fractional):
    x1, y1 = rs.uniform(0, W - 40, n), rs.uniform(0, H - 30, n)
    b = np.stack([x1, y1, x1 + rs.uniform(8, 70, n), y1 + rs.uniform(8, 50, n)], axis=1)
    return (b if fractional else np.round(b)).astype(np.float32)


def make_inputs(seed=19):
    rs = np.random.RandomState(seed)
    anns, results = [], []
    scores = rs.permutation(N_IMG * N_CLS * MAX_DETS).astype(np.float32) / np.float32(N_IMG * N_CLS * MAX_DETS + 1)
    k = 0
    for i in range(N_IMG):
        frac = i % 2 == 1
        n_reg, n_ign = (0, 0) if i == 0 else (rs.randint(1, 7), rs.randint(0, 3))
        gt, ign = _boxes(rs, n_reg, frac), _boxes(rs, n_ign, frac)
        gl, il = rs.randint(0, N_CLS, n_reg).astype(np.int64), rs.randint(0, N_CLS, n_ign).astype(np.int64)
        if i == 1:
            # two heavily overlapping boxes of different labels: one detection matches both
            gt = np.concatenate([gt, np.array([[20, 20, 80, 70], [22, 21, 82, 72]], np.float32)])
            gl = np.concatenate([gl, np.array([0, 1])])
        if i == 2:
            gt, gl = gt[:1], gl[:1]                                  # a box nothing is aimed at below: a false negative
        anns.append(dict(bboxes=gt, labels=gl, bboxes_ignore=ign, labels_ignore=il))
        per_class = []
        for c in range(N_CLS):
            own = np.concatenate([gt[gl == c], ign[il == c]]) if i != 2 else np.zeros((0, 4), np.float32)
            other = gt[gl != c]
            parts = []
            if len(own):
                parts.append(own + rs.uniform(-4, 4, own.shape))
                parts.append(own + rs.uniform(-2, 2, own.shape))
            if len(other) and i != 2:
                parts.append(other[:2] + rs.uniform(-3, 3, other[:2].shape))
            if i == 1 and c == 0:
                parts.append(np.array([[21, 20, 81, 71]], np.float64))
            parts.append(_boxes(rs, rs.randint(0, 4), True))
            d = np.concatenate(parts)[:MAX_DETS]
            d = d if frac else np.round(d)
            d = d[rs.permutation(len(d))]
            per_class.append(np.concatenate([d, scores[k:k + len(d), None]], axis=1).astype(np.float32))
            k += len(d)
        results.append(per_class)
    return anns, results


def main():
    refload.install()
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot  # noqa: F401  (before np.bool: numpy.ma does not import with it)
    import numpy.ma  # noqa: F401
    np.bool = bool                                                   # (mean_ap.py:203 predates numpy 1.24)
    sys.modules['terminaltables'] = types.SimpleNamespace(AsciiTable=None)
    sys.modules['mmcv'].is_str = lambda x: isinstance(x, str)
    mean_ap = refload.ref('mmdet.core.evaluation.mean_ap')
    overlaps = refload.ref('mmdet.core.evaluation.bbox_overlaps', 'bbox_overlaps')
    spec = importlib.util.spec_from_file_location(
        'reference_confusion_matrix', os.path.join(refload.REF, 'tools', 'analysis_tools', 'confusion_matrix.py'))
    cmx = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cmx)
    anns, results = make_inputs()
    out = dict(n_img=np.array(N_IMG), n_cls=np.array(N_CLS), cases=np.array(CASES, np.float64))
    for i, a in enumerate(anns):
        for key, v in a.items():
            out[f'{key}_{i}'] = v
        for c in range(N_CLS):
            out[f'det_{i}_{c}'] = results[i][c]
    # ---- the confusion matrix, image by image as calculate_confusion_matrix does
    for k, (score_thr, tp_iou_thr) in enumerate(CASES):
        cm = np.zeros((N_CLS + 1, N_CLS + 1))
        for a, res in zip(anns, results):
            cmx.analyze_per_img_dets(cm, a['bboxes'], a['labels'], res, score_thr, tp_iou_thr, None)
        out[f'cm_{k}'] = cm
    # ---- the per-image mAP, as bbox_map_eval drives eval_map
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    maps = []
    for a, res in zip(anns, results):
        mean_aps = [mean_ap.eval_map([res], [a], iou_thr=thr, logger='silent')[0] for thr in iou_thrs]
        maps.append(sum(mean_aps) / len(mean_aps))
    out['per_image_map'] = np.array(maps, np.float64)
    # ---- a fixture that could pass while proving nothing is refused here
    cm = out['cm_1']
    off_diag = cm[:N_CLS, :N_CLS].sum() - np.trace(cm[:N_CLS, :N_CLS])
    assert off_diag > 0 and cm[N_CLS, :N_CLS].sum() > 0 and cm[:N_CLS, N_CLS].sum() > 0, cm
    assert not np.array_equal(out['cm_0'], out['cm_1']) and not np.array_equal(out['cm_1'], out['cm_2'])
    twice, two_boxes = 0, 0
    for a, res in zip(anns, results):
        hits = [overlaps(d[d[:, 4] >= 0.3][:, :4], a['bboxes']) >= 0.5 for d in res]
        for c, h in enumerate(hits):
            if h.size:
                twice += int((h[:, a['labels'] == c].sum(axis=0) >= 2).sum())
                two_boxes += int((h.sum(axis=1) >= 2).sum())
    assert twice > 0, 'no box is matched by two detections of its label'
    assert two_boxes > 0, 'no detection matches two boxes'
    m = out['per_image_map']
    assert len(np.unique(m)) > 3 and ((m > 0) & (m < 1)).sum() >= 3, m
    scores = np.concatenate([r[:, 4] for res in results for r in res])
    assert len(np.unique(scores)) == len(scores)
    path = os.path.join(HERE, 'result_analysis_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; cm(.3, .5) =', cm.astype(int).tolist(), 'maps', np.round(m, 3).tolist(),
          'twice', twice, 'two_boxes', two_boxes)


if __name__ == '__main__':
    main()
