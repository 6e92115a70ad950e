"""CPU: the COCO evaluation cut into the steps of the device path - ``pack_coco_segments``, ``coco_flags_host`` (the existing
``_evaluate_img`` per segment and area range: the yardstick of tests/test_hip_coco_eval.py), ``coco_accumulate``,
``coco_summarize`` - gives the twelve numbers of ``coco_eval_bbox`` with ==, and ``device=None`` leaves every caller on the
host path."""
import numpy as np
import pytest

from coco_cases import pack_segments, seeded_split, summary
from oadg_amd import evaluation as E

N_CLS = 5


@pytest.fixture(scope='module')
def split():
    return seeded_split(0, n_img=30, n_cls=N_CLS)


def test_the_split_says_something(split):
    gt_anns, results = split
    assert not gt_anns[3] and not any(len(r) for r in results[5])
    crowds = [g['iscrowd'] for per in gt_anns for g in per]
    assert 0.05 < np.mean(crowds) < 0.3
    assert all(g['area'] != g['bbox'][2] * g['bbox'][3] for per in gt_anns for g in per)
    scores = np.concatenate([r[:, 4] for per in results for r in per])
    assert len(np.unique(scores)) <= 11 < len(scores)                               # one decimal: ties
    assert max(len(r) for per in results for r in per) > 20                        # max_dets (2, 5, 20) cuts


@pytest.mark.parametrize('max_dets,names', [((1, 10, 100), None), ((2, 5, 20), None), (E.MMDET_MAX_DETS, E.MMDET_METRICS)])
def test_host_flags_and_accumulate_equal_the_host_evaluator(split, max_dets, names):
    gt_anns, results = split
    want = E.coco_eval_bbox(gt_anns, results, N_CLS, max_dets=max_dets, names=names)
    pack = E.pack_coco_segments(gt_anns, results, N_CLS, max_dets[-1])
    flags = E.coco_flags_host(pack)
    got = summary(pack, flags, max_dets, names)
    print(want)
    assert list(got) == list(want) and len(got) == 12
    assert got == want                                                              # all twelve, with ==
    assert all(v > 0 for v in want.values()) and want[list(want)[0]] < want[list(want)[1]] < 1
    assert set(np.unique(flags).tolist()) == {E.COCO_FP, E.COCO_TP, E.COCO_IGNORED}
    # an explicit selection of thresholds picks those rows; a threshold the host evaluator does not know is refused
    two = E.coco_flags_host(pack, [E.IOU_THRS[0], E.IOU_THRS[5]])
    assert np.array_equal(two, flags[:, [0, 5]])
    with pytest.raises(ValueError, match='IOU_THRS'):
        E.coco_flags_host(pack, [0.123])


def test_match_is_the_annotation_index_of_the_matched_box(split):
    gt_anns, results = split
    pack = E.pack_coco_segments(gt_anns, results, N_CLS, 100)
    flags, match = E.coco_flags_host(pack, want_match=True)
    assert match.shape == flags.shape == (4, 10, len(pack['dets'])) and match.dtype == np.int32
    n_gt = np.repeat(np.diff(pack['gt_off']), np.diff(pack['det_off']))
    assert (match >= -1).all() and (match < n_gt[None, None, :]).all()
    assert ((flags == E.COCO_TP) <= (match >= 0)).all() and ((flags == E.COCO_FP) <= (match == -1)).all()
    # a true positive's box is not a crowd and lies inside the area range
    g_first = np.repeat(pack['gt_off'][:-1], np.diff(pack['det_off']))
    for a, (lo, hi) in enumerate(E.AREA_RNG):
        tp = flags[a] == E.COCO_TP
        g = (g_first[None, :] + match[a])[tp]
        assert not pack['gt_crowd'][g].any() and (pack['gt_area'][g] >= lo).all() and (pack['gt_area'][g] <= hi).all()


def test_pack_invariants(split):
    gt_anns, results = split
    gt_anns = [list(per) for per in gt_anns]
    gt_anns[0] = gt_anns[0] + [dict(bbox=[1., 2., 3., 4.], category=N_CLS, area=12., iscrowd=0),
                               dict(bbox=[1., 2., 3., 4.], category=-1, area=12., iscrowd=0)]      # labels outside [0, K)
    full = E.pack_coco_segments(gt_anns, results, N_CLS, 1000)
    pack = E.pack_coco_segments(gt_anns, results, N_CLS, 7)
    S = len(gt_anns) * N_CLS
    for p in (full, pack):
        assert p['dets'].dtype == np.float64 and p['dets'].shape[1] == 4 and p['gts'].dtype == np.float64
        assert p['det_off'].dtype == p['gt_off'].dtype == np.int32 and p['gt_crowd'].dtype == np.uint8
        assert len(p['det_off']) == len(p['gt_off']) == S + 1 and p['det_off'][0] == p['gt_off'][0] == 0
        assert (np.diff(p['det_off']) >= 0).all() and (np.diff(p['gt_off']) >= 0).all()
        assert p['det_off'][-1] == len(p['dets']) == len(p['det_score']) == len(p['det_rank']) == len(p['det_cat'])
        assert p['gt_off'][-1] == len(p['gts']) == len(p['gt_area']) == len(p['gt_crowd']) == len(p['gt_cat'])
        assert all(a.flags['C_CONTIGUOUS'] for a in (p['dets'], p['gts'], p['gt_area'], p['gt_crowd'], p['det_score']))
    assert len(full['gts']) == sum(len(per) for per in gt_anns) - 2
    assert len(full['dets']) == sum(len(r) for per in results for r in per)
    assert (np.diff(pack['det_off']) == np.minimum(np.diff(full['det_off']), 7)).all() and np.diff(full['det_off']).max() > 7
    for s in range(S):
        i, k = divmod(s, N_CLS)
        raw = np.asarray(results[i][k], np.float64)
        order = np.argsort(-raw[:, 4], kind='mergesort')                             # descending and stable
        for p, cut in ((full, 1000), (pack, 7)):
            sl = slice(p['det_off'][s], p['det_off'][s + 1])
            r = raw[order[:cut]]
            assert np.array_equal(p['det_score'][sl], r[:, 4])
            assert np.array_equal(p['dets'][sl], np.stack([r[:, 0], r[:, 1], r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]], 1))
            assert np.array_equal(p['det_rank'][sl], np.arange(len(r))) and (p['det_cat'][sl] == k).all()
        own = [g for g in gt_anns[i] if g['category'] == k]                          # annotation order
        sl = slice(full['gt_off'][s], full['gt_off'][s + 1])
        assert np.array_equal(full['gts'][sl], np.array([g['bbox'] for g in own], np.float64).reshape(-1, 4))
        assert full['gt_area'][sl].tolist() == [g['area'] for g in own]
        assert full['gt_crowd'][sl].tolist() == [g['iscrowd'] for g in own] and (full['gt_cat'][sl] == k).all()
    # equal scores keep their positions
    same = [[np.array([[0, 0, 10, 10, .5], [1, 1, 11, 11, .5], [2, 2, 12, 12, .7], [3, 3, 13, 13, .5]], np.float32)]]
    p = E.pack_coco_segments([[]], same, 1, 3)
    assert p['dets'][:, 0].tolist() == [2, 0, 1] and p['det_rank'].tolist() == [0, 1, 2]
    empty = E.pack_coco_segments([], [], 3, 100)
    assert len(empty['dets']) == 0 and empty['det_off'].tolist() == [0] and empty['dets'].shape == (0, 4)


def test_accumulate_on_hand_segments():
    """one class, two images: a true positive at 0.9, a false positive at 0.8, a second true positive at 0.7 - precision
    1, 1/2, 2/3 -> envelope 1, 2/3, 2/3; recall 1/2 at the first and 1 at the third detection"""
    box = [10., 10., 40., 40.]
    far = [300., 300., 40., 40.]
    pack = pack_segments([([box + [0.9], far + [0.8]], [box], None, None), ([box + [0.7]], [box], None, None)])
    flags = E.coco_flags_host(pack)
    assert flags[0, 0].tolist() == [1, 0, 1]
    precision, recall = E.coco_accumulate(pack, flags, (1, 10, 100))
    assert recall[0, 0, 0, 2] == 1.0 and recall[0, 0, 0, 0] == 1.0                  # (one detection per image: both hits)
    p = precision[0, :, 0, 0, 2]
    eps = np.spacing(1)                                                             # (COCOeval's tp / (fp + tp + eps))
    assert (p[:51] == 1 / (1 + eps)).all() and (p[51:] == 2 / (3 + eps)).all()
    assert (precision[:, :, 0, 1, :] == -1).all() and (recall[:, 0, 1, :] == -1).all()      # no 'small' box: undefined
    # no detections at all: recall 0 and precision 0 where a box counts
    none = pack_segments([([], [box], None, None)])
    precision, recall = E.coco_accumulate(none, E.coco_flags_host(none), (1, 10, 100))
    assert (recall[:, 0, 0, :] == 0).all() and (precision[:, :, 0, 0, :] == 0).all() and (recall[:, 0, 1, :] == -1).all()


def _three_image_set_and_results():
    """the dataset of tests/test_eval_hook.py's bbox case, rebuilt"""
    from oadg_amd.pipelines import SyntheticCityscapes
    ds = SyntheticCityscapes(img_shape=(256, 512), num_boxes=5, num_classes=3, length=3, box_size=(16, 200), seed=7,
                             device='cpu', test_mode=True)
    rs = np.random.RandomState(0)
    results = []
    for i in range(len(ds)):
        b, l = ds.boxes(i)
        per_class = []
        for c in range(3):
            g = b[l == c]
            hit = g + rs.uniform(-6, 6, g.shape).astype(np.float32)
            miss = np.array([[10., 10., 60., 40.], [300., 100., 420., 230.]], np.float32)[:rs.randint(0, 3)]
            boxes = np.concatenate([hit, miss])
            per_class.append(np.concatenate([boxes, rs.uniform(0.05, 1, (len(boxes), 1)).astype(np.float32)], 1))
        results.append(per_class)
    return ds, results


def test_device_none_is_the_host_path_for_every_caller(monkeypatch):
    ds, results = _three_image_set_and_results()
    want = E.coco_eval_bbox(E.dataset_gt_anns(ds), results, 3, max_dets=E.MMDET_MAX_DETS, names=E.MMDET_METRICS)
    assert 0 < want['mAP'] < want['mAP_50']
    expect = {f'bbox_{k}': float(f'{want[k]:.3f}') for k in E.MMDET_METRICS[:6]}
    expect['bbox_mAP_copypaste'] = ' '.join(f'{want[k]:.3f}' for k in E.MMDET_METRICS[:6])

    def no_device(*a, **k):
        raise AssertionError('device=None reached the device path')
    monkeypatch.setattr(E, 'coco_flags_device', no_device)
    got = E.dataset_evaluate(ds, results, metric='bbox', device=None)
    assert got == expect and list(got) == list(expect)
    assert ds.evaluate(results, metric='bbox', device=None) == expect               # Dataset.evaluate forwards the keyword
    assert E.evaluate(results, ds, ['bbox'], 3, mmdet_style=True, device=None) == {'bbox': want}
    assert E.evaluate(results, ds, ['bbox'], 3, device=None) == {'bbox': E.coco_eval_bbox(E.dataset_gt_anns(ds), results, 3)}
    # 'auto' is voc_device(): without a device the host path, with one the device path - the named parameter never reaches
    # check_evaluate_args either way
    monkeypatch.setattr(E, 'voc_device', lambda: None)
    assert ds.evaluate(results, metric='bbox') == expect
    seen = []
    monkeypatch.setattr(E, 'voc_device', lambda: 'the device')
    monkeypatch.setattr(E, 'coco_flags_device', lambda pack, thrs, rng, device, **k: seen.append(device) or E.coco_flags_host(pack))
    assert ds.evaluate(results, metric='bbox') == expect and seen == ['the device']
    assert E.evaluate(results, ds, ['bbox'], 3, mmdet_style=True) == {'bbox': want} and len(seen) == 2
    with pytest.raises(NotImplementedError, match="'classwise'"):
        ds.evaluate(results, metric='bbox', classwise=True, device=None)
