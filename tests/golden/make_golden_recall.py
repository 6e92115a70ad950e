"""Generate tests/golden/recall_reference.npz from the reference's own proposal-recall evaluation (run by path, refload.py):
  * bbox_overlaps (numpy)   mmdet/core/evaluation/bbox_overlaps.py:5-65
  * eval_recalls            mmdet/core/evaluation/recall.py:65-114  (-> _recalls, recall.py:11-41)
for budgets (1, 10, 100, 1000) and thresholds .5 ... .95 under both coordinate conventions.  Seeded inputs: 11 images whose
(boxes, proposals) counts are (0, 5), (4, 0), (6, 3), (1, 1), (9, 40), (70, 130), (3, 1100), (5, 64), (5, 65), (12, 12) and
(None, 0): no boxes, no proposals, more boxes than proposals (surplus rounds), more proposals than the largest budget, the
wave width and one beyond it; proposals are jittered copies of the boxes among random ones, in shuffled order; all scores
distinct (the reference's unstable sort cannot matter), every other image has rounded coordinates (ties between IoUs).
Three shims let recall.py run here: a stub ``terminaltables``, ``mmcv.utils.print_log`` (refload has it) and a proxy for the
module's ``np`` whose ``array`` falls back to an object array for ragged input (recall.py:110 calls np.array on a list of
matrices of different shapes, which numpy >= 1.24 refuses).
Run here only:  python tests/golden/make_golden_recall.py
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

W, H = 640, 360
COUNTS = ((0, 5), (4, 0), (6, 3), (1, 1), (9, 40), (70, 130), (3, 1100), (5, 64), (5, 65), (12, 12), (None, 0))
NUMS = (1, 10, 100, 1000)
THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)


class _RaggedNumpy:
    """numpy, except that ``array`` of a ragged list is the object array numpy < 1.24 made of it"""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def array(obj, *args, **kwargs):
        try:
            return np.array(obj, *args, **kwargs)
        except ValueError:
            out = np.empty(len(obj), dtype=object)
            for i, o in enumerate(obj):
                out[i] = o
            return out


def _boxes(rs, n):
    x1, y1 = rs.uniform(0, W - 80, n), rs.uniform(0, H - 60, n)
    return np.stack([x1, y1, x1 + rs.uniform(10, 160, n), y1 + rs.uniform(10, 120, n)], axis=1)


def make_inputs(seed=11):
    rs = np.random.RandomState(seed)
    total = sum(p for _, p in COUNTS)
    scores = rs.permutation(total).astype(np.float32) / np.float32(total + 1)          # all distinct
    gts, props, k = [], [], 0
    for i, (g, p) in enumerate(COUNTS):
        gt = None if g is None else _boxes(rs, g)
        parts = [np.zeros((0, 4))]
        if g:
            for spread in (3, 8, 20, 40):                # close and loose copies: recall grows with the budget
                parts.append(gt + rs.uniform(-spread, spread, gt.shape))
        parts.append(_boxes(rs, p))
        d = np.concatenate(parts)
        d = d[rs.permutation(len(d))[:p]]
        if i % 2 == 0:
            gt, d = (None if gt is None else np.round(gt)), np.round(d)
        gts.append(None if gt is None else gt.astype(np.float32))
        props.append(np.concatenate([d, scores[k:k + p, None]], axis=1).astype(np.float32))
        k += p
    return gts, props


def main():
    refload.install()
    sys.modules['terminaltables'] = types.SimpleNamespace(AsciiTable=lambda rows: types.SimpleNamespace(table=str(rows)))
    recall = refload.ref('mmdet.core.evaluation.recall')
    recall.np = _RaggedNumpy()
    overlaps = refload.ref('mmdet.core.evaluation.bbox_overlaps', 'bbox_overlaps')
    gts, props = make_inputs()
    out = dict(n_img=np.array(len(gts)), nums=np.array(NUMS), thrs=THRS,
               has_gt=np.array([g is not None for g in gts]))
    for i, (g, p) in enumerate(zip(gts, props)):
        if g is not None:
            out[f'gt_{i}'] = g
        out[f'prop_{i}'] = p
    ars = {}
    for c, legacy in enumerate((False, True)):
        for i, (g, p) in enumerate(zip(gts, props)):
            if g is not None and len(g):
                ranked = p[np.argsort(p[:, 4])[::-1]][:NUMS[-1], :4]
                out[f'iou_{c}_{i}'] = overlaps(g, ranked, use_legacy_coordinate=legacy)
        r = recall.eval_recalls(gts, props, list(NUMS), THRS, logger='silent', use_legacy_coordinate=legacy)
        assert r.shape == (len(NUMS), len(THRS)) and r.dtype == np.float64
        out[f'recalls_{c}'] = r
        ars[c] = r.mean(axis=1)
    # a fixture that could pass while proving nothing is refused here
    cnt = [(0 if g is None else len(g), len(p)) for g, p in zip(gts, props)]
    assert any(g > p > 0 for g, p in cnt), 'no image has surplus rounds (-1)'
    assert any(g > 0 and p == 0 for g, p in cnt), 'no image has boxes and no proposals (0.0)'
    assert any(g is None for g in gts), 'no image has None boxes'
    assert any(p > NUMS[-1] for _, p in cnt), 'no image exceeds the largest budget'
    assert all(len(set(np.round(a, 12))) == len(NUMS) and (np.diff(a) > 0).all() for a in ars.values()), ars
    assert not np.array_equal(out['recalls_0'], out['recalls_1']), 'the two conventions agree everywhere'
    s = np.concatenate([p[:, 4] for p in props])
    assert len(np.unique(s)) == len(s), 'scores are not distinct'
    path = os.path.join(HERE, 'recall_reference.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes; AR modern', np.round(ars[0], 3), 'legacy', np.round(ars[1], 3))


if __name__ == '__main__':
    main()
