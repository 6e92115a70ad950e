"""Result analysis on the host (oadg_amd.evaluation: confusion_per_image, pack_confusion_segments, confusion_counts_host,
calculate_confusion_matrix, voc_accumulate_per_image, per_image_map, rank_images), pinned to the reference's own output
(tests/golden/result_analysis_reference.npz, written by make_golden_result_analysis.py from the reference's
confusion_matrix.py and mean_ap.py), and the three tools of tools/analysis_tools on a 4-image synthetic tree.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import confusion_cases as K
from oadg_amd import evaluation as E
from test_voc_eval import PROTOCOLS
from test_voc_eval import load_fixture as load_voc_fixture

ROOT = K.ROOT


def _sum_per_image(anns, results, C, score_thr, tp_iou_thr, nms_iou_thr=None):
    cm = np.zeros((C + 1, C + 1))
    for a, r in zip(anns, results):
        E.confusion_per_image(cm, a['bboxes'], a['labels'], r, score_thr, tp_iou_thr, nms_iou_thr)
    return cm


def test_fixture_says_something():
    z, anns, results, n, C = K.load_fixture()
    assert (n, C) == (10, 3) and z['cases'].tolist() == [[0.0, 0.5], [0.3, 0.5], [0.3, 0.75]]
    cm = z['cm_1']
    assert cm[:C, :C].sum() - np.trace(cm[:C, :C]) > 0 and cm[C, :C].sum() > 0 and cm[:C, C].sum() > 0
    assert not np.array_equal(z['cm_0'], z['cm_1']) and not np.array_equal(z['cm_1'], z['cm_2'])
    m = z['per_image_map']
    assert len(np.unique(m)) > 3 and ((m > 0) & (m < 1)).sum() >= 3
    assert any(len(a['bboxes_ignore']) for a in anns) and len(anns[0]['bboxes']) == 0


def test_confusion_equals_the_reference():
    z, anns, results, n, C = K.load_fixture()
    for k, (score_thr, tp_iou_thr) in enumerate(z['cases'].tolist()):
        want = z[f'cm_{k}']
        got = _sum_per_image(anns, results, C, score_thr, tp_iou_thr)
        assert got.dtype == np.float64 and np.array_equal(got, want), (k, got, want)
        pack = E.pack_confusion_segments(results, anns, C, score_thr)
        counts = E.confusion_counts_host(pack, tp_iou_thr)
        assert counts.dtype == np.int64 and counts.shape == (C + 1, C + 1) and np.array_equal(counts, want), (k, counts)


def test_per_image_map_equals_the_reference():
    z, anns, results, n, C = K.load_fixture()
    got = E.per_image_map(results, anns, C, device=None)
    print('per-image mAP', got.tolist(), 'reference', z['per_image_map'].tolist())
    assert got.dtype == np.float64 and np.array_equal(got, z['per_image_map'])
    # (bbox, segm) tuples: the bbox part
    assert np.array_equal(E.per_image_map([(r, None) for r in results], anns, C), got)
    # the thresholds are np.float64 in the reference, so its comparison is a float64 one: image 4 holds an IoU of exactly
    # fp32(0.7) < 0.7, which does not pass 0.7 there (it would pass the fp32-rounded threshold of the VOC protocol)
    a, r = anns[4], results[4]
    iou = E.bbox_overlaps_voc(r[2][:, :4], np.vstack((a['bboxes'][a['labels'] == 2], a['bboxes_ignore'][a['labels_ignore'] == 2])))
    assert (iou.max(axis=1) == np.float32(0.7)).any() and float(np.float32(0.7)) < 0.7 < E._f32_at_least(0.7)
    assert E._f32_at_least(0.5) == 0.5 and E._f32_at_least(0.75) == 0.75 and np.float32(E._f32_at_least(0.6)) == np.float32(0.6)
    rounded = np.mean([E.eval_map_voc([r], [a], C, float(t))[0] for t in E.IOU_THRS])
    assert rounded != got[4]


@pytest.mark.parametrize('p', [0, 1])
def test_voc_accumulate_per_image_is_the_one_image_eval_map(p):
    z, anns, results, n, C = load_voc_fixture()
    dataset, legacy = PROTOCOLS[p]
    thrs = [0.5, 0.75]
    pack = E.pack_voc_segments(results, anns, C)
    flags = E.voc_flags_host(pack, thrs, legacy)
    seen = set()
    for t, thr in enumerate(thrs):
        got = E.voc_accumulate_per_image(pack, flags[t], dataset)
        want = [E.eval_map_voc([results[i]], [anns[i]], C, thr, dataset, legacy)[0] for i in range(n)]
        assert got.tolist() == want, (p, t)
        seen |= set(want)
        assert E.voc_accumulate_per_image(pack, flags, dataset)[t].tolist() == want          # all thresholds in one call
    assert len(seen) > 3 and want[0] == 0.0                          # (image 0 has no box)


def test_hand_cases_on_the_host():
    for name, (C, anns, results, score_thr, thr, want) in K.HAND.items():
        assert _sum_per_image(anns, results, C, score_thr, thr).tolist() == want, name
        assert E.confusion_counts_host(E.pack_confusion_segments(results, anns, C, score_thr), thr).tolist() == want, name
    # the threshold is rounded to fp32: an IoU of exactly fp32(0.7) passes 0.7 (in float64 it would not)
    a, r = [K._ann([[0, 0, 10, 10]], [0])], [K._res(1, c0=[[0, 0, 10, 7, 1.0]])]
    assert float(E.bbox_overlaps_voc(r[0][0][:, :4], a[0]['bboxes'])[0, 0]) < 0.7
    assert _sum_per_image(a, r, 1, 0, 0.7).tolist() == [[1, 0], [0, 0]]
    # ... and so is the score threshold: a score of fp32(0.3) passes 0.3
    r = [K._res(1, c0=[[0, 0, 10, 10, 0.3]])]
    assert float(r[0][0][0, 4]) > 0.3 - 1e-7 and _sum_per_image(a, r, 1, 0.3, 0.5).tolist() == [[1, 0], [0, 0]]
    assert E.confusion_counts_host(E.pack_confusion_segments(r, a, 1, 0.3), 0.5).tolist() == [[1, 0], [0, 0]]
    # bboxes_ignore takes no part
    a2 = [dict(a[0], bboxes_ignore=np.array([[0, 0, 10, 10]], np.float32), labels_ignore=np.array([0]))]
    assert E.confusion_counts_host(E.pack_confusion_segments(r, a2, 1, 0.3), 0.5).tolist() == [[1, 0], [0, 0]]


def test_pack_layout_and_its_errors():
    z, anns, results, n, C = K.load_fixture()
    pk = E.pack_confusion_segments(results, anns, C, 0.3)
    assert pk['num_classes'] == C and pk['det_off'].shape == pk['gt_off'].shape == (n + 1,)
    assert pk['dets'].dtype == pk['gts'].dtype == np.float32 and pk['dets'].shape[1:] == pk['gts'].shape[1:] == (4,)
    assert all(pk[k].dtype == np.int32 for k in ('det_cls', 'det_off', 'gt_lab', 'gt_off'))
    assert all(pk[k].flags['C_CONTIGUOUS'] for k in ('dets', 'det_cls', 'det_off', 'gts', 'gt_lab', 'gt_off'))
    assert pk['dets'].ctypes.data % 16 == 0 and pk['gts'].ctypes.data % 16 == 0
    assert pk['det_off'][0] == 0 and pk['det_off'][-1] == len(pk['dets']) == len(pk['det_cls'])
    assert pk['gt_off'][-1] == len(pk['gts']) == len(pk['gt_lab'])
    dropped = 0
    for i in range(n):
        kept = [r[r[:, 4] >= np.float32(0.3)] for r in results[i]]
        dropped += sum(len(r) - len(q) for r, q in zip(results[i], kept))
        sl = slice(pk['det_off'][i], pk['det_off'][i + 1])
        assert np.array_equal(pk['dets'][sl], np.concatenate(kept)[:, :4])
        assert pk['det_cls'][sl].tolist() == [c for c, q in enumerate(kept) for _ in range(len(q))]
        g = slice(pk['gt_off'][i], pk['gt_off'][i + 1])
        assert np.array_equal(pk['gts'][g], anns[i]['bboxes']) and np.array_equal(pk['gt_lab'][g], anns[i]['labels'])
    assert dropped > 0
    assert E._aligned16(np.zeros(9, np.float32)[1:]).ctypes.data % 16 == 0
    empty = E.pack_confusion_segments([], [], 3)
    assert empty['det_off'].tolist() == [0] and empty['dets'].shape == (0, 4) and E.confusion_counts_host(empty).sum() == 0
    for bad in (-1, 3):
        with pytest.raises(ValueError, match='label outside'):
            E.pack_confusion_segments([K._res(3)], [K._ann([[0, 0, 1, 1]], [bad])], 3)
        with pytest.raises(ValueError, match='label outside'):
            E.confusion_per_image(np.zeros((4, 4)), np.zeros((1, 4)), [bad], K._res(3))
    with pytest.raises(ValueError, match='classes of detections'):
        E.pack_confusion_segments([K._res(2)], [K._ann([], [])], 3)
    with pytest.raises(ValueError, match='annotations'):
        E.pack_confusion_segments([K._res(3)], [], 3)
    with pytest.raises(ValueError, match='boxes with'):
        E.pack_confusion_segments([K._res(3)], [dict(bboxes=np.zeros((2, 4)), labels=np.zeros(1, int))], 3)


def test_nms_host_is_the_oracle_nms_with_a_score_threshold():
    import torch
    from oracle import nms as O
    rs = np.random.RandomState(2)
    suppressed = dropped = 0
    for trial in range(6):
        m = (0, 1, 2, 17, 40, 64)[trial]
        xy = rs.uniform(0, 60, (m, 2))
        d = np.concatenate([xy, xy + rs.uniform(10, 40, (m, 2)), np.round(rs.uniform(0, 1, (m, 1)), 1)], 1).astype(np.float32)
        for iou_thr, score_thr in ((0.5, 0.0), (0.3, 0.3)):
            keep = d[d[:, 4] > np.float32(score_thr)]                 # mmcv: scores > score_threshold survive
            want, _ = O.nms(torch.from_numpy(keep[:, :4].copy()), torch.from_numpy(keep[:, 4].copy()), iou_thr)
            got = E.nms_host(d, iou_thr, score_thr)
            assert np.array_equal(got, want.numpy()), (trial, iou_thr)
            suppressed += len(keep) - len(got)
            dropped += m - len(keep)
    assert suppressed > 0 and dropped > 0                             # (both the threshold and the suppression bit)


class _Split:
    """the two things calculate_confusion_matrix reads of a dataset"""

    def __init__(self, anns, C):
        self.anns, self.CLASSES = anns, tuple(f'c{i}' for i in range(C))

    def __len__(self):
        return len(self.anns)

    def get_ann_info(self, i):
        return self.anns[i]


def test_calculate_confusion_matrix_on_the_host():
    z, anns, results, n, C = K.load_fixture()
    ds = _Split(anns, C)
    got = E.calculate_confusion_matrix(ds, results, 0.3, None, 0.5, device=None)
    assert got.dtype == np.float64 and np.array_equal(got, z['cm_1'])
    assert np.array_equal(E.calculate_confusion_matrix(ds, [(r, None) for r in results], 0.3, device=None), got)
    with_nms = E.calculate_confusion_matrix(ds, results, 0.3, 0.3, 0.5, device=None)
    assert np.array_equal(with_nms, _sum_per_image(anns, results, C, 0.3, 0.5, nms_iou_thr=0.3))
    assert with_nms.sum() < got.sum()                                # (the second copies of the detections are suppressed)
    with pytest.raises(ValueError, match='results for'):
        E.calculate_confusion_matrix(ds, results[:-1], device=None)


def test_ranking_follows_the_reference():
    maps = [0.5, 0.1, 0.5, 0.9, 0.1, 0.3]
    good, bad = E.rank_images(maps, 2)
    assert bad == [(1, 0.1), (4, 0.1)] and good == [(2, 0.5), (3, 0.9)]          # stable: equal mAPs keep the image order
    good, bad = E.rank_images(maps, 20)                                          # 2 * 20 > 6: topk becomes 3
    assert bad == [(1, 0.1), (4, 0.1), (5, 0.3)] and good == [(0, 0.5), (2, 0.5), (3, 0.9)]
    good, bad = E.rank_images(maps[:5], 3)                                       # 5 // 2 = 2: the middle image in neither
    assert [i for i, _ in bad] == [1, 4] and [i for i, _ in good] == [2, 3]
    good, bad = E.rank_images(np.array([0.25, 0.25, 0.25, 0.25]), 1)
    assert bad == [(0, 0.25)] and good == [(3, 0.25)]
    with pytest.raises(AssertionError):
        E.rank_images(maps, 0)


def test_plot_writes_a_png_and_a_zero_row_does_not_raise(tmp_path, capsys):
    from PIL import Image
    T = K.load_tool('confusion_matrix')
    cm = np.array([[3, 1, 0], [0, 0, 0], [2, 0, 0]], np.float64)      # row 1 sums to 0: the reference raises on int(nan)
    T.plot_confusion_matrix(cm, ['car', 'bus', 'background'], save_dir=str(tmp_path / 'out'), color_theme='viridis')
    with Image.open(tmp_path / 'out' / 'confusion_matrix.png') as im:
        im.load()
        assert im.format == 'PNG' and im.size[0] > 100 and im.size[1] > 100
    with pytest.raises(NotImplementedError, match='--show'):
        T.parse_args(['cfg.py', 'r.pkl', 'out', '--show'])
    with pytest.raises(SystemExit):
        T.parse_args(['--help'])
    assert 'printed as 0%' in ' '.join(capsys.readouterr().out.split())          # (--help states the deviation)
    A = K.load_tool('analyze_results')
    with pytest.raises(SystemExit):
        A.parse_args(['--help'])
    assert '.png' in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match='--show'):
        A.parse_args(['cfg.py', 'r.pkl', 'out', '--show'])


def test_eval_metric_and_confusion_matrix_tools_on_a_synthetic_tree(tmp_path, monkeypatch):
    from PIL import Image
    from oadg_amd.datasets import CityscapesDataset
    t = K.synthetic_tree(tmp_path, monkeypatch)
    ds = CityscapesDataset(ann_file=t['ann'], img_prefix=t['prefix'], test_mode=True, device='cpu')
    env = dict(os.environ, PYTHONPATH=ROOT)
    # ---- eval_metric.py: prints dataset.evaluate's dict (the hook's keys of cfg.evaluation dropped)
    r = subprocess.run([sys.executable, os.path.join(K.TOOLS, 'eval_metric.py'), t['cfg'], t['pkl'], '--eval', 'bbox'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = ds.evaluate(t['results'], metric=['bbox'])
    assert 0 < want['bbox_mAP'] < 1
    assert r.stdout.strip().splitlines()[-1] == str(want)
    r = subprocess.run([sys.executable, os.path.join(K.TOOLS, 'eval_metric.py'), t['cfg'], t['pkl'], '--eval', 'bbox',
                        '--eval-options', 'metric_items=mAP_50'], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1] == str(ds.evaluate(t['results'], metric=['bbox'], metric_items='mAP_50'))
    # ---- confusion_matrix.py on the host path: the JSON holds the host function's counts
    out = tmp_path / 'cm'
    r = subprocess.run([sys.executable, os.path.join(K.TOOLS, 'confusion_matrix.py'), t['cfg'], t['pkl'], str(out),
                        '--device', 'host', '--score-thr', '0.3'], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    js = json.load(open(out / 'confusion_matrix.json'))
    want = E.calculate_confusion_matrix(ds, t['results'], 0.3, None, 0.5, device=None)
    assert js['labels'] == list(ds.CLASSES) + ['background'] and js['device'] == 'host'
    assert js['counts'] == want.astype(np.int64).tolist()
    C = len(ds.CLASSES)
    assert np.trace(want[:C, :C]) > 0 and want[:C, :C].sum() > np.trace(want[:C, :C]) and want[C].sum() > 0 and want[:, C].sum() > 0
    with Image.open(out / 'confusion_matrix.png') as im:
        im.load()
        assert im.format == 'PNG'
    r = subprocess.run([sys.executable, os.path.join(K.TOOLS, 'confusion_matrix.py'), t['cfg'], t['pkl'], str(out), '--show'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and '--show' in r.stderr
