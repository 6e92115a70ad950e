"""Inputs shared by tests/test_result_analysis.py (host) and tests/test_hip_confusion.py (GPU): the reference fixture, the hand
cases with their matrices written out, a seeded split, and a 4-image tools/make_synthetic_coco.py tree with fabricated
results, a config and a pickle.  Not a test module."""
import importlib.util
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'result_analysis_reference.npz')
TOOLS = os.path.join(ROOT, 'tools', 'analysis_tools')
Z5 = np.zeros((0, 5), np.float32)


def load_fixture():
    z = np.load(GOLDEN)
    n, C = int(z['n_img']), int(z['n_cls'])
    anns = [{k: z[f'{k}_{i}'] for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore')} for i in range(n)]
    results = [[z[f'det_{i}_{c}'] for c in range(C)] for i in range(n)]
    return z, anns, results, n, C


def _res(C, **per_class):
    """per-class list of [k, 5] arrays from c<index>=[[x1, y1, x2, y2, score], ...]"""
    out = [Z5] * C
    for k, rows in per_class.items():
        out[int(k[1:])] = np.array(rows, np.float32).reshape(-1, 5)
    return out


def _ann(boxes, labels):
    return dict(bboxes=np.array(boxes, np.float32).reshape(-1, 4), labels=np.array(labels, np.int64))


# name -> (num_classes, [annotation], [result], score_thr, tp_iou_thr, expected matrix)
HAND = {
    # the reference's own answer for these inputs (analyze_per_img_dets run by path, as the fixture's generator runs it): the class-0
    # detection over the upper half of box 0 has IoU exactly 0.5 with it; the far one is a background false positive; the
    # class-2 detection is under the score threshold, so box 1 (label 2) is a false negative
    'a': (3, [_ann([[0, 0, 100, 100], [50, 50, 150, 150]], [0, 2])],
          [_res(3, c0=[[0, 0, 100, 50, .9], [300, 300, 310, 310, .8]], c2=[[40, 40, 150, 150, .2]])], .3, .5,
          [[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 0]]),
    # IoU exactly 0.5 counts at 0.5 ...
    'b50': (1, [_ann([[0, 0, 10, 10]], [0])], [_res(1, c0=[[0, 0, 10, 5, .9]])], 0, .5, [[1, 0], [0, 0]]),
    # ... and not at 0.75: a background false positive and a false negative
    'b75': (1, [_ann([[0, 0, 10, 10]], [0])], [_res(1, c0=[[0, 0, 10, 5, .9]])], 0, .75, [[0, 1], [1, 0]]),
    # one class-1 detection over two nearly identical boxes of labels 0 and 2: both cells, both boxes false negatives
    'c': (3, [_ann([[10, 10, 60, 60], [11, 10, 61, 60]], [0, 2])], [_res(3, c1=[[10, 10, 60, 60, .7]])], 0, .5,
          [[0, 1, 0, 1], [0, 0, 0, 0], [0, 1, 0, 1], [0, 0, 0, 0]]),
    # two detections of its label on one box: the cell is 2, no false negative, nothing claimed
    'd': (2, [_ann([[10, 10, 60, 60]], [1])], [_res(2, c1=[[10, 10, 60, 60, .9], [11, 10, 60, 60, .8]])], 0, .5,
          [[0, 0, 0], [0, 2, 0], [0, 0, 0]]),
}


def random_split(seed, n_img, C, max_boxes=12, max_dets=30, fractional=True, W=300, H=200):
    """(annotations, results): per image 0 .. max_boxes boxes with random labels, and 0 .. max_dets detections over the
    classes - jittered copies of the boxes under their own and under OTHER classes, and random boxes; scores with one or
    six decimals; some images without boxes, some without detections"""
    rs = np.random.RandomState(seed)
    anns, results = [], []
    for i in range(n_img):
        k = 0 if rs.randint(8) == 0 else rs.randint(0, max_boxes + 1)
        m = 0 if rs.randint(8) == 0 else rs.randint(0, max_dets + 1)
        xy = rs.uniform(0, [W - 60, H - 60], (k, 2))
        g = np.concatenate([xy, xy + rs.uniform(6, 60, (k, 2))], 1)
        gl = rs.randint(0, C, k)
        src = rs.randint(0, k, m // 2) if k else np.zeros(0, int)
        hit = g[src] + rs.uniform(-5, 5, (len(src), 4))
        xy = rs.uniform(0, [W - 60, H - 60], (m - len(src), 2))
        d = np.concatenate([hit, np.concatenate([xy, xy + rs.uniform(6, 60, (len(xy), 2))], 1)])
        if not fractional:
            g, d = np.round(g), np.round(d)
        own = rs.randint(3, size=len(src)) > 0                       # two thirds under the box's own label
        dl = np.concatenate([np.where(own, gl[src], rs.randint(0, C, len(src))), rs.randint(0, C, m - len(src))]).astype(int)
        sc = np.round(rs.uniform(0, 1, (m, 1)), 1 if rs.randint(2) else 6)
        d = np.concatenate([d, sc], 1).astype(np.float32)
        anns.append(dict(bboxes=g.astype(np.float32), labels=gl.astype(np.int64)))
        results.append([d[dl == c] for c in range(C)])
    return anns, results


def load_tool(name):
    """tools/analysis_tools/<name>.py by path"""
    spec = importlib.util.spec_from_file_location(f'oadg_analysis_{name}', os.path.join(TOOLS, f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def synthetic_tree(tmp_path, monkeypatch, n=4, H=64, W=128, boxes=3):
    """a tools/make_synthetic_coco.py tree of ``n`` images under tmp_path, a config whose data.test reads it, fabricated
    results (per box a jittered detection of its label, one of ANOTHER label, one far away; image 0 perfect, the last image
    without detections) and their pickle -> dict(cfg, pkl, results, ann, prefix)"""
    spec = importlib.util.spec_from_file_location('make_synthetic_coco_tool', os.path.join(ROOT, 'tools', 'make_synthetic_coco.py'))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    root = tmp_path / 'tree'
    monkeypatch.setattr(sys, 'argv', ['make_synthetic_coco.py', str(root), '--n', str(n), '--height', str(H), '--width', str(W),
                                      '--boxes', str(boxes)])
    maker.main()
    ann, prefix = str(root / 'train.json'), str(root / 'img') + '/'
    cfg = tmp_path / 'cfg.py'
    cfg.write_text(f"data = dict(test=dict(type='CityscapesDataset', ann_file={ann!r}, img_prefix={prefix!r}, pipeline=[]))\n"
                   "evaluation = dict(interval=1, metric='bbox', save_best='auto')\n")
    from oadg_amd.datasets import CityscapesDataset
    ds = CityscapesDataset(ann_file=ann, img_prefix=prefix, test_mode=True, device='cpu')
    rs = np.random.RandomState(4)
    results = []
    for i in range(n):
        a = ds.get_ann_info(i)
        per_class = [[] for _ in ds.CLASSES]
        if i < n - 1:
            for b, l in zip(a['bboxes'], a['labels']):
                jit = 0 if i == 0 else 3
                per_class[l].append(np.append(b + rs.uniform(-jit, jit, 4), rs.uniform(0.5, 1)))
                if i > 0:
                    per_class[(l + 1) % 8].append(np.append(b + rs.uniform(-2, 2, 4), rs.uniform(0.35, 0.9)))
                    per_class[l].append(np.append([W - 12, H - 10, W - 2, H - 2], rs.uniform(0.31, 0.6)))
        results.append([np.array(p, np.float32).reshape(-1, 5) for p in per_class])
    pkl = tmp_path / 'results.pkl'
    with open(pkl, 'wb') as f:
        pickle.dump(results, f)
    return dict(cfg=str(cfg), pkl=str(pkl), results=results, ann=ann, prefix=prefix, n=n, H=H, W=W)
