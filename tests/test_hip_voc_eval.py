"""GPU: csrc/voc_eval.hip (oadg_voc_tpfp.voc_tpfp, evaluation.eval_map_voc(device=...)) against the reference's own output
(tests/golden/voc_eval_reference.npz) and, bit for bit, against the host functions of oadg_amd.evaluation on hand-built
segments and a seeded sweep; tools/test_dwd.py end to end on two tiny VOC trees."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import oadg_voc_tpfp
from oadg_amd import evaluation as E
from test_sdgod_dataset import _obj, write_voc
from test_voc_eval import PROTOCOLS, load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z4 = np.zeros((0, 4), np.float32)
Z5 = np.zeros((0, 5), np.float32)


def _pack(segs):
    """segs: list of (dets [m, 5], regular boxes [k, 4], ignored boxes [j, 4]) -> the arrays of oadg_voc_tpfp"""
    d = [np.asarray(s[0], np.float32).reshape(-1, 5) for s in segs]
    g = [np.vstack((np.asarray(s[1], np.float32).reshape(-1, 4), np.asarray(s[2], np.float32).reshape(-1, 4))) for s in segs]
    off = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)      # noqa: E731
    return dict(dets=np.concatenate(d + [Z5]), det_off=off(d), gts=np.concatenate(g + [Z4]), gt_off=off(g),
                gt_reg=np.array([len(np.asarray(s[1]).reshape(-1, 4)) for s in segs], np.int32), num_classes=1)


def _host(pack, thrs, legacy):
    """(iou_max, iou_arg, flags) of every detection from the host functions"""
    D = len(pack['dets'])
    m, a = np.zeros(D, np.float32), np.full(D, -1, np.int32)
    for s in range(len(pack['gt_reg'])):
        d0, d1, g0, g1 = pack['det_off'][s], pack['det_off'][s + 1], pack['gt_off'][s], pack['gt_off'][s + 1]
        m[d0:d1], a[d0:d1] = E.voc_match(pack['dets'][d0:d1], pack['gts'][g0:g1], legacy)
    return m, a, E.voc_flags_host(pack, thrs, legacy)


def _device(pack, thrs, legacy, dev, fill=0xFF, workspace=None):
    up = [torch.from_numpy(pack[k]).to(dev) for k in ('dets', 'det_off', 'gts', 'gt_off', 'gt_reg')]
    D = len(pack['dets'])
    raw = [torch.full((n,), fill, dtype=torch.uint8, device=dev) for n in (4 * D, 4 * D, len(thrs) * D)]
    out = (raw[0].view(torch.float32), raw[1].view(torch.int32), raw[2].view(len(thrs), D))
    oadg_voc_tpfp.voc_tpfp(*up, thrs, legacy, out=out, workspace=workspace)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _check(segs, thrs, legacy, dev, fill=0xFF):
    pack = _pack(segs)
    want, got = _host(pack, thrs, legacy), _device(pack, thrs, legacy, dev, fill)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), 'iou_max bits'
    assert np.array_equal(got[1], want[1]), 'iou_arg'
    assert np.array_equal(got[2], want[2]), 'flags'
    return got


def test_device_equals_the_reference_fixture(dev):
    z, anns, results, n, C = load_fixture()
    thrs = [float(t) for t in z['thrs']]
    pack = E.pack_voc_segments(results, anns, C)
    for p, (dataset, legacy) in enumerate(PROTOCOLS):
        iou_max, iou_arg, flags = _device(pack, thrs, legacy, dev)
        for i in range(n):
            for c in range(C):
                s = i * C + c
                sl = slice(pack['det_off'][s], pack['det_off'][s + 1])
                ious = z[f'iou_{p}_{i}_{c}']
                if ious.shape[1]:
                    assert np.array_equal(iou_max[sl].view(np.uint32), ious.max(axis=1).view(np.uint32)), (p, i, c)
                    assert np.array_equal(iou_arg[sl], ious.argmax(axis=1)), (p, i, c)
                else:
                    assert (iou_arg[sl] == -1).all() and (iou_max[sl] == 0).all()
                for t in range(len(thrs)):
                    assert np.array_equal(flags[t, sl] == 1, z[f'tp_{p}_{t}_{i}_{c}'] == 1), (p, t, i, c)
                    assert np.array_equal(flags[t, sl] == 2, z[f'fp_{p}_{t}_{i}_{c}'] == 1), (p, t, i, c)
        per_thr = E.eval_map_voc_thrs(results, anns, C, thrs, dataset, legacy, device=dev)
        for t, (m, per_class) in enumerate(per_thr):
            assert [r['num_gts'] for r in per_class] == z[f'num_gts_{p}_{t}'].tolist()
            assert np.abs(np.array([r['ap'] for r in per_class], np.float64) - z[f'ap_{p}_{t}']).max() <= 1e-6
            assert abs(m - float(z[f'mean_ap_{p}_{t}'])) <= 1e-6
            assert m == E.eval_map_voc(results, anns, C, thrs[t], dataset, legacy)[0]            # host path: the same number


BOX = np.array([[10, 10, 50, 50]], np.float32)


def _d(*rows):
    return np.array(rows, np.float32).reshape(-1, 5)


def test_empty_segments_and_ignored_boxes(dev):
    segs = [(Z5, BOX, Z4),                                           # no detections
            (_d([10, 10, 50, 50, 0.9], [0, 0, 5, 5, 0.2]), Z4, Z4),   # no boxes
            (Z5, Z4, Z4),                                            # neither
            (_d([10, 10, 50, 50, 0.9], [80, 80, 90, 90, 0.8]), Z4, BOX),        # only an ignored box
            (_d([10, 10, 50, 50, 0.7]), BOX, BOX)]                   # a regular box and an identical ignored one
    for fill in (0xFF, 0x7F):                                        # (0xFF is also the bytes of iou_arg = -1)
        iou_max, iou_arg, flags = _check(segs, [0.5], True, dev, fill)
        assert iou_arg.tolist() == [-1, -1, 0, 0, 0] and flags[0].tolist() == [2, 2, 0, 2, 1]
    assert _device(_pack([(Z5, Z4, Z4)]), [0.5], True, dev)[2].shape == (1, 0)


def test_contested_box_equal_scores_and_touching_boxes(dev):
    segs = [(_d([12, 10, 50, 50, 0.6], [10, 10, 50, 50, 0.9], [11, 10, 50, 50, 0.8]), BOX, Z4),     # the highest score wins
            (_d([12, 10, 50, 50, 0.5], [10, 10, 50, 50, 0.5], [10, 11, 50, 50, 0.5]), BOX, Z4),     # equal scores: index 0
            (_d([10, 10, 50, 50, -0.0], [10, 10, 50, 50, 0.0]), BOX, Z4),                           # -0.0 is 0.0: index 0
            (_d([10, 10, 50, 50, -0.5], [10, 10, 50, 50, -0.25]), BOX, Z4)]                         # negative scores order too
    _, _, flags = _check(segs, [0.5], False, dev)
    assert flags[0].tolist() == [2, 1, 2, 1, 2, 2, 1, 2, 2, 1]
    # touching boxes: IoU 0 in modern coordinates, 11 / 231 in legacy ones; a threshold between the two tells them apart
    touch = [(_d([10, 0, 20, 10, 0.9]), np.array([[0, 0, 10, 10]], np.float32), Z4)]
    m0, _, f0 = _check(touch, [0.04], False, dev)
    m1, _, f1 = _check(touch, [0.04], True, dev)
    assert m0[0] == 0 and m1[0] == np.float32(11) / np.float32(231) and f0[0].tolist() == [2] and f1[0].tolist() == [1]


def test_wide_segments_cross_the_wave_and_the_lds_chunk(dev):
    rs = np.random.RandomState(3)
    # 300 detections on one box: five passes of the 64 lanes, groups of equal scores
    d = np.concatenate([BOX + rs.uniform(-12, 12, (300, 4)), np.round(rs.uniform(0, 1, (300, 1)), 1)], 1)
    _, _, flags = _check([(d, BOX, Z4)], [0.5, 0.75], True, dev)
    assert (flags == 1).sum(axis=1).tolist() == [1, 1]
    # 3 detections on 130 regular boxes: the boxes take two LDS chunks and the claim keys live in the workspace; two
    # detections contest box 129, one takes box 5 - and the same with the last 30 boxes ignored
    xs, ys = np.meshgrid(np.arange(13) * 40.0, np.arange(10) * 40.0)
    boxes = np.stack([xs.ravel(), ys.ravel(), xs.ravel() + 30, ys.ravel() + 30], 1).astype(np.float32)
    d3 = np.concatenate([boxes[[129, 5, 129]] + [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]], [[0.5], [0.4], [0.7]]], 1)
    iou_max, iou_arg, flags = _check([(d3, boxes, Z4), (d3, boxes[:100], boxes[100:])], [0.5, 0.99], True, dev)
    assert iou_arg.tolist() == [129, 5, 129] * 2
    assert flags.tolist() == [[2, 1, 1, 0, 1, 0], [1, 2, 2, 0, 2, 2]]
    # a contested box among 130 with the detections spread over several lanes' passes
    many = np.concatenate([boxes[rs.randint(100, 130, 200)] + rs.uniform(-3, 3, (200, 4)), rs.uniform(0, 1, (200, 1))], 1)
    _check([(many, boxes, Z4), (d3, BOX, Z4), (many[:70], boxes[:129], boxes[129:])], [0.5, 0.6, 0.7, 0.8], True, dev)


def test_short_workspace_threshold_count_and_repeatability(dev):
    rs = np.random.RandomState(5)
    boxes = np.round(rs.uniform(0, 200, (40, 2)))
    boxes = np.concatenate([boxes, boxes + np.round(rs.uniform(10, 60, (40, 2)))], 1).astype(np.float32)
    d = np.concatenate([boxes[rs.randint(0, 40, 90)] + rs.uniform(-5, 5, (90, 4)), rs.uniform(0, 1, (90, 1))], 1)
    pack = _pack([(d, boxes[:30], boxes[30:])])
    thrs = [0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85]
    with pytest.raises(RuntimeError, match='argument error -2'):                     # OADG_ESIZE
        _device(pack, thrs, True, dev, workspace=torch.empty(8 * 40 * 8 - 8, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='thresholds'):
        _device(pack, thrs + [0.9], True, dev)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_voc_tpfp.voc_tpfp(*[torch.from_numpy(pack[k]) for k in ('dets', 'det_off', 'gts', 'gt_off', 'gt_reg')], [0.5], True)
    a = _check([(d, boxes[:30], boxes[30:])], thrs, True, dev)
    b = _device(pack, thrs, True, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert len({tuple(f) for f in a[2].tolist()}) > 1                                # the thresholds do not all agree


@pytest.mark.parametrize('legacy', [True, False])
@pytest.mark.parametrize('fractional', [False, True])
def test_seeded_sweep_equals_the_host(dev, legacy, fractional):
    rs = np.random.RandomState(11 + 2 * legacy + fractional)
    segs = []
    for _ in range(200):
        k, m = rs.randint(0, 41), rs.randint(0, 41)
        xy = rs.uniform(0, 160, (k, 2))
        g = np.concatenate([xy, xy + rs.uniform(4, 60, (k, 2))], 1)
        src = g[rs.randint(0, k, m // 2)] + rs.uniform(-5, 5, (m // 2, 4)) if k else np.zeros((0, 4))
        xy = rs.uniform(0, 160, (m - len(src), 2))
        d = np.concatenate([src, np.concatenate([xy, xy + rs.uniform(4, 60, (len(xy), 2))], 1)])
        if not fractional:
            g, d = np.round(g), np.round(d)
        scores = np.round(rs.uniform(0, 1, (m, 1)), 1 if rs.randint(2) else 6)        # (one decimal: equal scores)
        n_reg = rs.randint(0, k + 1)
        segs.append((np.concatenate([d, scores], 1), g[:n_reg], g[n_reg:]))
    _, _, flags = _check(segs, [0.5, 0.75], legacy, dev)
    assert {0, 1, 2} <= set(np.unique(flags).tolist())


def test_sdgod_evaluate_matches_on_the_device(dev, tmp_path):
    from oadg_amd.datasets import SdgodDataset
    from test_voc_eval import EVAL_TREE, _tree_results
    prefix = write_voc(str(tmp_path), EVAL_TREE)
    ds = SdgodDataset(ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix, device='cpu', test_mode=True)
    assert E.voc_device() is not None
    res = _tree_results()
    assert ds.evaluate(res, iou_thr=[0.5, 0.75]) == ds.evaluate(res, iou_thr=[0.5, 0.75], device=None)


def test_test_dwd_cli_on_two_tiny_voc_trees(tmp_path):
    trees = []
    # three images per tree, two tested: the scored set has to be cut to the tested one (first_images)
    for k, names in enumerate((('a', 'b', 'c'), ('d', 'e', 'f'))):
        tree = {n: (96, 160, True, [_obj('car', (10 + 5 * k, 20, 90, 70)), _obj('person', (100, 10, 140, 80), 1)]) for n in names}
        trees.append(write_voc(str(tmp_path / f'dom{k}'), tree))
    cfg = tmp_path / 'dwd_tiny.py'
    cfg.write_text(
        f"_base_ = ['{ROOT}/configs/oadg/faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod_test.py']\n"
        "img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)\n"
        "test_pipeline = [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', img_scale=(320, 192), flip=False,\n"
        "    transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **img_norm_cfg),\n"
        "                dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),\n"
        "                dict(type='Collect', keys=['img'])])]\n"
        "data = dict(test=[" + ', '.join(
            f"dict(type='SdgodDataset', ann_file=['{t}ImageSets/Main/train.txt'], img_prefix=['{t}'], pipeline=test_pipeline)"
            for t in trees) + "])\n")
    wd = tmp_path / 'eval'
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test_dwd.py'), str(cfg), 'none', '--eval', 'mAP',
                        '--max-samples', '2', '--work-dir', str(wd), '--out', str(tmp_path / 'r.pkl')],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    dicts = [ln for ln in r.stdout.splitlines() if ln.startswith("{'0_AP50'")]
    assert len(dicts) == 2, r.stdout[-2000:]
    summary = [ln for ln in r.stdout.splitlines() if ln.startswith('AP50 per split: ')]
    assert len(summary) == 1 and len(summary[0].split()) == 7                        # two numbers, 'mean', their mean
    files = [f for f in os.listdir(wd) if f.startswith('eval_') and f.endswith('.json')]
    assert len(files) == 1
    ev = json.load(open(wd / files[0]))
    assert len(ev) == 2 and all(list(e['metric']) == ['0_AP50', '0_mAP'] and 0.0 <= e['metric']['0_mAP'] <= 1.0 for e in ev)
    assert not (tmp_path / 'r.pkl').exists()
    for i in range(2):
        with open(tmp_path / f'r_{i}.pkl', 'rb') as f:
            assert len(pickle.load(f)) == 2
    assert r.stdout.count(': 2 images in ') == 2
