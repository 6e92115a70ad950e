"""Generate tests/golden/voc_eval_reference.npz from the reference's own VOC evaluation (run by path, refload.py):
  * bbox_overlaps (numpy)   mmdet/core/evaluation/bbox_overlaps.py:5-65
  * tpfp_default            mmdet/core/evaluation/mean_ap.py:168-267
  * eval_map                mmdet/core/evaluation/mean_ap.py:297-440   (logger='silent', nproc=1)
for the two protocols SdgodDataset.evaluate reaches - ('voc07', legacy coordinates) and (None, modern coordinates) - at
IoU 0.5 and 0.75 (both exact in binary).  Seeded inputs: 8 images, 3 classes, 0-6 regular and 0-2 ignored boxes per image,
0-12 detections per (image, class) made of jittered boxes, a second jittered copy (two detections contest one box) and
random boxes; all scores distinct (the reference's unstable sorts cannot matter), half of the coordinates fractional.
Three shims let mean_ap.py import here: np.bool, a stub ``terminaltables`` and ``mmcv.is_str``.
Run here only:  python tests/golden/make_golden_voc_eval.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import refload  # noqa: E402

N_IMG, N_CLS, W, H = 8, 3, 200, 120
PROTOCOLS = (('voc07', True), (None, False))
THRS = (0.5, 0.75)


def _boxes(rs, n, fractional):
    x1, y1 = rs.uniform(0, W - 40, n), rs.uniform(0, H - 30, n)
    b = np.stack([x1, y1, x1 + rs.uniform(8, 70, n), y1 + rs.uniform(8, 50, n)], axis=1)
    return (b if fractional else np.round(b)).astype(np.float32)


def make_inputs(seed=7):
    rs = np.random.RandomState(seed)
    anns, results = [], []
    scores = rs.permutation(N_IMG * N_CLS * 12).astype(np.float32) / np.float32(N_IMG * N_CLS * 12 + 1)   # all distinct
    k = 0
    for i in range(N_IMG):
        frac = i % 2 == 1
        n_reg, n_ign = (0, 0) if i == 0 else (rs.randint(0, 7), rs.randint(0, 3))
        gt, ign = _boxes(rs, n_reg, frac), _boxes(rs, n_ign, frac)
        gl, il = rs.randint(0, N_CLS, n_reg).astype(np.int64), rs.randint(0, N_CLS, n_ign).astype(np.int64)
        anns.append(dict(bboxes=gt, labels=gl, bboxes_ignore=ign, labels_ignore=il))
        per_class = []
        for c in range(N_CLS):
            src = np.concatenate([gt[gl == c], ign[il == c]])
            parts = []
            if len(src):
                parts.append(src + rs.uniform(-4, 4, src.shape))
                parts.append(src + rs.uniform(-6, 6, src.shape))
            parts.append(_boxes(rs, rs.randint(0, 4), True))
            d = np.concatenate(parts)[:12]
            d = d if frac else np.round(d)
            d = d[rs.permutation(len(d))]
            per_class.append(np.concatenate([d, scores[k:k + len(d), None]], axis=1).astype(np.float32))
            k += len(d)
        results.append(per_class)
    return anns, results


def main():
    refload.install()
    np.bool = bool                                                   # (mean_ap.py:203 predates numpy 1.24)
    sys.modules['terminaltables'] = types.SimpleNamespace(AsciiTable=None)
    sys.modules['mmcv'].is_str = lambda x: isinstance(x, str)
    mean_ap = refload.ref('mmdet.core.evaluation.mean_ap')
    overlaps = refload.ref('mmdet.core.evaluation.bbox_overlaps', 'bbox_overlaps')
    anns, results = make_inputs()
    out = dict(n_img=np.array(N_IMG), n_cls=np.array(N_CLS), thrs=np.array(THRS))
    for i, a in enumerate(anns):
        for key, v in a.items():
            out[f'{key}_{i}'] = v
        for c in range(N_CLS):
            out[f'det_{i}_{c}'] = results[i][c]
    ignored_by_ignore, means = 0, {}
    for p, (dataset, legacy) in enumerate(PROTOCOLS):
        for i, a in enumerate(anns):
            for c in range(N_CLS):
                g, ig = a['bboxes'][a['labels'] == c], a['bboxes_ignore'][a['labels_ignore'] == c]
                out[f'iou_{p}_{i}_{c}'] = overlaps(results[i][c], np.vstack((g, ig)), use_legacy_coordinate=legacy)
                for t, thr in enumerate(THRS):
                    tp, fp = mean_ap.tpfp_default(results[i][c], g, ig, thr, None, legacy)
                    out[f'tp_{p}_{t}_{i}_{c}'], out[f'fp_{p}_{t}_{i}_{c}'] = tp[0], fp[0]
                    ignored_by_ignore += int(((tp[0] == 0) & (fp[0] == 0)).sum())
        for t, thr in enumerate(THRS):
            m, per_class = mean_ap.eval_map(results, anns, iou_thr=thr, dataset=dataset, logger='silent', nproc=1,
                                            use_legacy_coordinate=legacy)
            out[f'mean_ap_{p}_{t}'] = np.array(m, dtype=np.float64)
            out[f'ap_{p}_{t}'] = np.array([r['ap'] for r in per_class], dtype=np.float32)
            out[f'num_gts_{p}_{t}'] = np.array([r['num_gts'] for r in per_class], dtype=np.int64)
            out[f'num_dets_{p}_{t}'] = np.array([r['num_dets'] for r in per_class], dtype=np.int64)
            means[p, t] = m
    # a fixture that could pass while proving nothing is refused here
    assert ignored_by_ignore > 0, 'no detection is ignored because of an ignored box'
    assert all(means[0, t] != means[1, t] for t in range(len(THRS))), means
    assert all(0 < v < 1 for v in means.values()), means
    path = os.path.join(HERE, 'voc_eval_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes;', {k: round(v, 4) for k, v in means.items()}, 'ignored', ignored_by_ignore)


if __name__ == '__main__':
    main()
