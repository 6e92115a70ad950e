"""The reference's VOC protocol on the host (oadg_amd.evaluation: bbox_overlaps_voc, tpfp_default, average_precision
'11points', eval_map_voc), pinned to the reference's own output (tests/golden/voc_eval_reference.npz, written by
make_golden_voc_eval.py from mean_ap.py / bbox_overlaps.py), SdgodDataset.evaluate on a VOC tree with ``difficult`` objects,
ConcatDataset from a list-valued ``ann_file`` and the five-domain test config.  No GPU."""
import os

import numpy as np
import pytest

from oadg_amd import evaluation as E
from test_sdgod_dataset import _obj, write_voc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'voc_eval_reference.npz')
DWD_TEST_CFG = os.path.join(ROOT, 'configs', 'oadg', 'faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod_test.py')
PROTOCOLS = (('voc07', True), (None, False))          # make_golden_voc_eval.PROTOCOLS


def load_fixture():
    z = np.load(GOLDEN)
    n, C = int(z['n_img']), int(z['n_cls'])
    anns = [{k: z[f'{k}_{i}'] for k in ('bboxes', 'labels', 'bboxes_ignore', 'labels_ignore')} for i in range(n)]
    results = [[z[f'det_{i}_{c}'] for c in range(C)] for i in range(n)]
    return z, anns, results, n, C


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_fixture_says_something():
    z, anns, results, n, C = load_fixture()
    assert (n, C) == (8, 3) and list(z['thrs']) == [0.5, 0.75]
    for t in range(2):
        assert 0 < float(z[f'mean_ap_0_{t}']) < 1 and float(z[f'mean_ap_0_{t}']) != float(z[f'mean_ap_1_{t}'])
    ignored = sum(int(((z[f'tp_0_0_{i}_{c}'] == 0) & (z[f'fp_0_0_{i}_{c}'] == 0)).sum()) for i in range(n) for c in range(C))
    assert ignored > 0                                   # a detection whose best box is a difficult one
    scores = np.concatenate([r[:, 4] for res in results for r in res])
    assert len(np.unique(scores)) == len(scores)         # the reference's unstable sorts cannot matter
    assert any(len(a['bboxes_ignore']) for a in anns) and len(anns[0]['bboxes']) == 0


def test_iou_bits_and_flags_equal_the_reference():
    z, anns, results, n, C = load_fixture()
    for p, (_, legacy) in enumerate(PROTOCOLS):
        for i, a in enumerate(anns):
            for c in range(C):
                g, ig = a['bboxes'][a['labels'] == c], a['bboxes_ignore'][a['labels_ignore'] == c]
                d = results[i][c]
                got = E.bbox_overlaps_voc(d[:, :4], np.vstack((g, ig)), legacy)
                want = z[f'iou_{p}_{i}_{c}']
                assert got.dtype == np.float32 and got.shape == want.shape
                assert np.array_equal(_bits(got), _bits(want)), (p, i, c)
                for t, thr in enumerate(z['thrs']):
                    tp, fp = E.tpfp_default(d, g, ig, float(thr), legacy)
                    assert tp.dtype == np.float32 and np.array_equal(tp, z[f'tp_{p}_{t}_{i}_{c}']), (p, t, i, c)
                    assert np.array_equal(fp, z[f'fp_{p}_{t}_{i}_{c}']), (p, t, i, c)


def test_eval_map_voc_equals_the_reference():
    z, anns, results, n, C = load_fixture()
    for p, (dataset, legacy) in enumerate(PROTOCOLS):
        for t, thr in enumerate(z['thrs']):
            m, per_class = E.eval_map_voc(results, anns, C, float(thr), dataset, legacy)
            assert [r['num_gts'] for r in per_class] == z[f'num_gts_{p}_{t}'].tolist()
            assert [r['num_dets'] for r in per_class] == z[f'num_dets_{p}_{t}'].tolist()
            ap = np.array([r['ap'] for r in per_class], np.float64)
            print(p, t, 'ap', ap, 'reference', z[f'ap_{p}_{t}'], 'mean', m, float(z[f'mean_ap_{p}_{t}']))
            assert np.abs(ap - z[f'ap_{p}_{t}']).max() <= 1e-6
            assert abs(m - float(z[f'mean_ap_{p}_{t}'])) <= 1e-6
    both = E.eval_map_voc_thrs(results, anns, C, [0.5, 0.75], 'voc07', True)
    assert [m for m, _ in both] == [E.eval_map_voc(results, anns, C, thr, 'voc07', True)[0] for thr in (0.5, 0.75)]


def test_average_precision_11points_by_hand():
    # 4 regular boxes; detections by score: tp fp tp tp fp  ->  recall .25 .25 .5 .75 .75, precision 1 1/2 2/3 3/4 3/5
    rec = np.array([0.25, 0.25, 0.5, 0.75, 0.75])
    pre = np.array([1.0, 1 / 2, 2 / 3, 3 / 4, 3 / 5], np.float32)
    # recall >= 0, .1, .2: best precision 1; >= .3 ... .7: 3/4; >= .8, .9, 1: none
    want = (3 * 1.0 + 5 * 0.75) / 11
    assert abs(E.average_precision(rec, pre, mode='11points') - want) < 1e-6
    # area mode is the default and is what it was: 0.25 * 1 + 0.5 * 0.75
    assert E.average_precision(rec, pre) == E.average_precision(rec, pre, mode='area')
    assert abs(E.average_precision(rec, pre.astype(np.float64)) - (0.25 + 0.5 * 0.75)) < 1e-12
    assert E.average_precision(np.zeros(0), np.zeros(0), mode='11points') == 0.0
    with pytest.raises(ValueError, match='11points'):
        E.average_precision(rec, pre, mode='12points')


def test_fixed_rules_stable_order_and_fp32_threshold():
    # equal scores: the lower index claims the box (per image) ...
    gt = np.array([[10, 10, 50, 50]], np.float32)
    d = np.array([[12, 10, 50, 50, 0.5], [10, 10, 50, 50, 0.5], [10, 10, 50, 50, 0.9]], np.float32)
    assert E.voc_flags(d[:2], gt, 1, 0.5).tolist() == [E.FLAG_TP, E.FLAG_FP]
    assert E.voc_flags(d, gt, 1, 0.5).tolist() == [E.FLAG_FP, E.FLAG_FP, E.FLAG_TP]
    # ... a regular box and an identical ignored one: the first (regular) is the argmax; only ignored: neither tp nor fp
    assert E.voc_flags(d[2:], np.vstack((gt, gt)), 1, 0.5).tolist() == [E.FLAG_TP]
    assert E.voc_flags(d[2:], gt, 0, 0.5).tolist() == [E.FLAG_IGNORED]
    tp, fp = E.tpfp_default(d[2:], np.zeros((0, 4)), gt, 0.5)
    assert tp.tolist() == [0] and fp.tolist() == [0]
    tp, fp = E.tpfp_default(d[2:], np.zeros((0, 4)), np.zeros((0, 4)), 0.5)
    assert tp.tolist() == [0] and fp.tolist() == [1]
    # the threshold is rounded to fp32: an IoU of exactly fp32(0.7) passes 0.7 (in float64 it would not: fp32(0.7) < 0.7)
    g = np.array([[0, 0, 10, 10]], np.float32)
    dd = np.array([[0, 0, 10, 7, 1.0]], np.float32)
    iou = E.bbox_overlaps_voc(dd[:, :4], g)[0, 0]
    assert iou == np.float32(0.7) and float(iou) < 0.7
    assert E.voc_flags(dd, g, 1, 0.7).tolist() == [E.FLAG_TP]
    # touching boxes overlap by one pixel column in legacy coordinates only
    a, b = np.array([[0, 0, 10, 10]], np.float32), np.array([[10, 0, 20, 10]], np.float32)
    assert E.bbox_overlaps_voc(a, b)[0, 0] == 0 and E.bbox_overlaps_voc(a, b, True)[0, 0] == np.float32(11) / np.float32(231)


def test_pack_orders_segments_regular_before_ignored():
    z, anns, results, n, C = load_fixture()
    pk = E.pack_voc_segments(results, anns, C)
    assert pk['det_off'].dtype == np.int32 and pk['det_off'].shape == (n * C + 1,) and pk['gt_reg'].shape == (n * C,)
    for i, a in enumerate(anns):
        for c in range(C):
            s = i * C + c
            g, ig = a['bboxes'][a['labels'] == c], a['bboxes_ignore'][a['labels_ignore'] == c]
            assert np.array_equal(pk['gts'][pk['gt_off'][s]:pk['gt_off'][s + 1]], np.vstack((g, ig)))
            assert pk['gt_reg'][s] == len(g)
            assert np.array_equal(pk['dets'][pk['det_off'][s]:pk['det_off'][s + 1]], results[i][c])
    # annotations without the ignore keys (the synthetic set's form) and an empty split
    pk2 = E.pack_voc_segments(results, [dict(bboxes=a['bboxes'], labels=a['labels']) for a in anns], C)
    assert np.array_equal(pk2['gt_reg'], pk['gt_reg']) and np.array_equal(np.diff(pk2['gt_off']), pk['gt_reg'])
    assert E.eval_map_voc([], [], 3)[0] == 0.0
    none = E.eval_map_voc([[np.zeros((0, 5), np.float32)] * 3], [dict(bboxes=np.zeros((0, 4)), labels=np.zeros(0))], 3)
    assert none[0] == 0.0 and [r['num_gts'] for r in none[1]] == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ SdgodDataset.evaluate
EVAL_TREE = {
    'a': (80, 100, True, [_obj('car', (10, 20, 50, 60)), _obj('person', (5, 5, 30, 30), 1), _obj('bus', (40, 30, 90, 75), 0),
                          _obj('car', (60, 5, 95, 25), 1)]),
    'b': (40, 64, True, [_obj('truck', (2, 3, 40, 38)), _obj('car', (30, 5, 60, 30))]),
    'c': (48, 64, True, [_obj('bike', (1, 2, 20, 30), 1), _obj('car', (20, 2, 60, 40))]),
}
CAR, PERSON, BUS, TRUCK = 2, 4, 0, 6


def _tree_results():
    def per_class(k):
        return [np.array(k.get(c, np.zeros((0, 5))), np.float32).reshape(-1, 5) for c in range(7)]
    return [
        # a: the car found; a detection on the DIFFICULT car (ignored, not a false positive) outscores everything; a
        #    detection on the difficult person; a loose detection of the bus that passes IoU 0.5 only with the + 1 extents
        per_class({CAR: [[9, 19, 49, 59, 0.8], [59, 4, 94, 24, 0.95], [100, 100, 120, 110, 0.3]],
                     PERSON: [[4, 4, 29, 29, 0.7]], BUS: [[39, 29, 89, 51, 0.6]]}),
        # b, c: over the three regular cars the detections by score read tp fp tp fp fp fp - 11 points and area disagree
        per_class({CAR: [[29, 4, 59, 29, 0.5], [0, 0, 12, 12, 0.6]], TRUCK: [[1, 2, 39, 37, 0.9]]}),
        per_class({CAR: [[19, 1, 30, 39, 0.4]]}),
    ]


def test_sdgod_evaluate_is_the_voc07_protocol_not_eval_map(tmp_path):
    from oadg_amd.datasets import SdgodDataset
    prefix = write_voc(str(tmp_path), EVAL_TREE)
    ds = SdgodDataset(ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix, device='cpu', test_mode=True)
    assert ds.year == 2007 and len(ds) == 3
    results = _tree_results()
    anns = [ds.get_ann_info(i) for i in range(3)]
    assert sum(len(a['bboxes_ignore']) for a in anns) == 3
    want50, per = E.eval_map_voc(results, anns, 7, 0.5, 'voc07', True)
    want75, _ = E.eval_map_voc(results, anns, 7, 0.75, 'voc07', True)
    got = ds.evaluate(results, metric='mAP', device=None)
    assert list(got) == ['AP50', 'mAP'] and got['AP50'] == round(want50, 3) and got['mAP'] == want50
    two = ds.evaluate(results, metric=['mAP'], iou_thr=[0.5, 0.75], device=None)
    assert list(two) == ['AP50', 'AP75', 'mAP'] and two['AP75'] == round(want75, 3) and two['mAP'] == (want50 + want75) / 2
    # difficult objects are not ground truth: num_gts counts the regular ones (cars: 3, not 4; no person, no bike at all)
    assert [r['num_gts'] for r in per] == [1, 0, 3, 0, 0, 0, 1]
    # ... and it is NOT what eval_map says of the same inputs (bboxes_ignore never read: the detections on the difficult
    # objects are false positives there; area AP; modern extents)
    old, _ = E.eval_map(results, E.dataset_box_anns(ds), 7, iou_thr=0.5)
    assert abs(old - want50) > 1e-3
    area, _ = E.eval_map_voc(results, anns, 7, 0.5, None, True)
    modern, _ = E.eval_map_voc(results, anns, 7, 0.5, 'voc07', False)
    assert area != want50 and modern != want50             # each of the three differences shows on this tree
    # the names the reference rejects stay rejected by name
    with pytest.raises(NotImplementedError, match="'recall'"):
        ds.evaluate(results, metric='recall')
    with pytest.raises(NotImplementedError, match="'scale_ranges'"):
        ds.evaluate(results, metric='mAP', scale_ranges=[(0, 32)])
    # a VOC2012 prefix: area mode, still the legacy coordinates
    p12 = write_voc(str(tmp_path / 'y12'), EVAL_TREE, year='VOC2012')
    d12 = SdgodDataset(ann_file=p12 + 'ImageSets/Main/train.txt', img_prefix=p12, device='cpu', test_mode=True)
    assert d12.year == 2012 and d12.evaluate(results, device=None)['mAP'] == area


def test_untouched_evaluators_return_what_they_returned(tmp_path):
    """XMLDataset and the synthetic set still go through eval_map (area mode, every box ground truth)"""
    from oadg_amd.datasets import XMLDataset
    from oadg_amd.pipelines import SyntheticCityscapes
    prefix = write_voc(str(tmp_path), EVAL_TREE)
    x = XMLDataset(ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix, device='cpu', test_mode=True,
                   classes=('bus', 'bike', 'car', 'motor', 'person', 'rider', 'truck'))
    results = _tree_results()
    m50, _ = E.eval_map(results, E.dataset_box_anns(x), 7, iou_thr=0.5)
    m75, _ = E.eval_map(results, E.dataset_box_anns(x), 7, iou_thr=0.75)
    assert x.evaluate(results, metric='mAP', iou_thr=[0.5, 0.75]) == {'AP50': round(m50, 3), 'AP75': round(m75, 3),
                                                                      'mAP': (m50 + m75) / 2}
    syn = SyntheticCityscapes(img_shape=(256, 512), num_boxes=5, num_classes=3, length=3, box_size=(16, 200), seed=7,
                              device='cpu', test_mode=True)
    rs = np.random.RandomState(0)
    res = []
    for b, l in (syn.boxes(i) for i in range(3)):
        hit = [b[l == c] + rs.uniform(-6, 6, b[l == c].shape).astype(np.float32) for c in range(3)]
        res.append([np.concatenate([h, rs.uniform(0.05, 1, (len(h), 1)).astype(np.float32)], 1) for h in hit])
    m, _ = E.eval_map(res, [syn.boxes(i) for i in range(3)], 3)
    assert syn.evaluate(res, metric='mAP') == {'AP50': round(m, 3), 'mAP': m}
    assert E.VOC_EVAL == dict(metrics=('mAP',), absent=('recall',), kwargs=('proposal_nums', 'iou_thr'),
                              absent_kwargs=('scale_ranges',))


# ------------------------------------------------------------------------------------------------ ConcatDataset, config
def test_concat_dataset_from_list_valued_ann_file(tmp_path):
    from oadg_amd.datasets import ConcatDataset, build_dataset
    p0 = write_voc(str(tmp_path / 'd0'), EVAL_TREE)
    p1 = write_voc(str(tmp_path / 'd1'), {'b': EVAL_TREE['b'], 'c': EVAL_TREE['c']})
    files = [p0 + 'ImageSets/Main/train.txt', p1 + 'ImageSets/Main/train.txt']
    ds = build_dataset(dict(type='SdgodDataset', ann_file=files, img_prefix=[p0, p1]), default_args=dict(device='cpu', test_mode=True))
    assert isinstance(ds, ConcatDataset) and len(ds) == 5 and [len(d) for d in ds.datasets] == [3, 2]
    assert ds.CLASSES == ds.datasets[0].CLASSES and ds.flag.tolist() == [1] * 5
    for i, (k, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]):             # across the seam
        a, b = ds.get_ann_info(i), ds.datasets[k].get_ann_info(j)
        assert all(np.array_equal(a[key], b[key]) for key in a)
    assert np.array_equal(ds.get_ann_info(-1)['bboxes'], ds.datasets[1].get_ann_info(1)['bboxes'])
    imgs, boxes, labels = ds.batch([3])
    assert tuple(imgs.shape) == (1, 40, 64, 3) and np.array_equal(boxes[0], ds.datasets[1].get_ann_info(0)['bboxes'])
    with pytest.raises(AssertionError, match='seam'):
        ds.batch([2, 3])
    res = _tree_results()
    got = ds.evaluate(res + res[1:], metric='mAP', device=None)
    assert list(got) == ['0_AP50', '0_mAP', '1_AP50', '1_mAP']
    assert got['0_mAP'] == ds.datasets[0].evaluate(res, device=None)['mAP']
    assert got['1_mAP'] == ds.datasets[1].evaluate(res[1:], device=None)['mAP']
    with pytest.raises(AssertionError, match='different sizes'):
        ds.evaluate(res, metric='mAP')
    # one img_prefix string for every list entry (both lists live under p0 here); a single-entry list is a ConcatDataset too
    one = build_dataset(dict(type='SdgodDataset', ann_file=[files[0], files[0]], img_prefix=p0), default_args=dict(device='cpu'))
    assert len(one) == 6 and isinstance(one, ConcatDataset)
    with pytest.raises(NotImplementedError, match='separate_eval'):
        build_dataset(dict(type='SdgodDataset', ann_file=files, img_prefix=[p0, p1], separate_eval=False),
                      default_args=dict(device='cpu'))


def test_dwd_test_config_has_the_five_domains():
    from oadg_amd import Config
    cfg = Config.fromfile(DWD_TEST_CFG)
    tests = cfg.data.test
    assert isinstance(tests, (list, tuple)) and len(tests) == 5
    ends = ['Daytime_Sunny/daytime_clear/VOC2007/', 'Daytime-Foggy/daytime_foggy/VOC2007/', 'Dusk-rainy/dusk_rainy/VOC2007/',
            'Night_rainy/night_rainy/VOC2007/', 'Night-Sunny/night_sunny/VOC2007/']
    for k, (t, end) in enumerate(zip(tests, ends)):
        assert t['type'] == 'SdgodDataset' and isinstance(t['ann_file'], (list, tuple)) and len(t['ann_file']) == 1
        assert t['img_prefix'][0].endswith(end)
        assert t['ann_file'][0].endswith(end + 'ImageSets/Main/' + ('test.txt' if k == 0 else 'train.txt'))
        assert [p['type'] for p in t['pipeline']] == ['LoadImageFromFile', 'MultiScaleFlipAug']
        assert tuple(t['pipeline'][1]['img_scale']) == (2048, 1024) and t['pipeline'][1]['flip'] is False
    assert cfg.data.val.ann_file.endswith('Daytime_Sunny/daytime_clear/VOC2007/ImageSets/Main/test.txt')
    assert dict(cfg.evaluation) == dict(interval=1, metric='mAP')
    assert cfg.data.train.type == 'RepeatDataset' and cfg.model.roi_head.bbox_head.num_classes == 7       # inherited


def test_test_dwd_scores_the_images_it_tested(tmp_path):
    """tools/test_dwd.py --max-samples: ``first_images`` cuts a dataset (plain, concatenated across the seam, synthetic) to
    its first n images without touching the original, and ``eval_kwargs_of`` drops the hook's keys"""
    import importlib.util
    from oadg_amd import Config
    from oadg_amd.datasets import build_dataset
    from oadg_amd.pipelines import SyntheticCityscapes
    spec = importlib.util.spec_from_file_location('oadg_tools_test_dwd', os.path.join(ROOT, 'tools', 'test_dwd.py'))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    p0 = write_voc(str(tmp_path / 'd0'), EVAL_TREE)
    p1 = write_voc(str(tmp_path / 'd1'), {'b': EVAL_TREE['b'], 'c': EVAL_TREE['c']})
    ds = build_dataset(dict(type='SdgodDataset', ann_file=[p0 + 'ImageSets/Main/train.txt', p1 + 'ImageSets/Main/train.txt'],
                            img_prefix=[p0, p1]), default_args=dict(device='cpu', test_mode=True))
    res = _tree_results()
    assert T.first_images(ds, 5) is ds and T.first_images(ds, 9) is ds
    four = T.first_images(ds, 4)                                       # all of the first tree, one image of the second
    assert len(four) == 4 and [len(d) for d in four.datasets] == [3, 1] and four.cumulative_sizes == [3, 4]
    assert len(ds) == 5 and [len(d) for d in ds.datasets] == [3, 2]    # the original is left alone
    got = four.evaluate(res + res[1:2], metric=['mAP'], device=None)
    assert got['0_mAP'] == ds.datasets[0].evaluate(res, device=None)['mAP']
    assert got['1_mAP'] == T.first_images(ds.datasets[1], 1).evaluate(res[1:2], device=None)['mAP']
    two = T.first_images(ds, 2)                                        # inside the first tree: the second holds nothing
    assert [len(d) for d in two.datasets] == [2, 0] and np.array_equal(two.get_ann_info(1)['bboxes'], ds.get_ann_info(1)['bboxes'])
    assert list(two.datasets[0].evaluate(res[:2], device=None)) == ['AP50', 'mAP']
    syn = SyntheticCityscapes(img_shape=(64, 128), num_boxes=3, num_classes=3, length=7, box_size=(8, 40), device='cpu')
    assert len(T.first_images(syn, 2)) == 2 and len(syn) == 7
    cfg = Config(dict(evaluation=dict(interval=1, save_best='auto', rule='greater', iou_thr=[0.5, 0.75], metric='bbox')))
    assert T.eval_kwargs_of(cfg, ['mAP'], {'iou_thr': '0.5'}) == dict(metric=['mAP'], iou_thr=0.5)
    assert T.eval_kwargs_of(cfg, ['mAP'], None) == dict(metric=['mAP'], iou_thr=[0.5, 0.75])
