"""GPU: csrc/coco_eval.hip (oadg_coco_match.coco_match, evaluation.coco_eval_bbox(device=...)) against the host evaluator,
byte for byte: flags and matched boxes of hand-built segments (with the expected values written out), empty segments, segments
across the kernel's staging capacities and a seeded sweep against ``coco_flags_host`` (= ``_evaluate_img``), and the twelve
numbers of a split and of a COCO-format dataset with ==."""
import json

import numpy as np
import pytest
import torch

import oadg_coco_match
from coco_cases import pack_segments, seeded_split
from oadg_amd import evaluation as E

pytestmark = pytest.mark.gpu
THRS = [float(E.IOU_THRS[0]), float(E.IOU_THRS[1])]          # 0.5 and 0.55
ALL, SMALL, MEDIUM, LARGE = range(4)
KEYS = oadg_coco_match.KEYS


def _cap(thrs):
    return [min(float(t), 1 - 1e-10) for t in thrs]


def _device(pack, thrs, dev, area_rng=E.AREA_RNG, fill=0xFF, workspace=None, want_match=True):
    up = [torch.from_numpy(pack[k]).to(dev) for k in KEYS]
    A, T, D = len(area_rng), len(thrs), len(pack['dets'])
    flags = torch.full((A, T, D), fill, dtype=torch.uint8, device=dev)
    match = torch.full((A * T * D * 4,), fill, dtype=torch.uint8, device=dev).view(torch.int32).view(A, T, D)
    oadg_coco_match.coco_match(*up, _cap(thrs), area_rng, out=(flags, match if want_match else None), workspace=workspace)
    torch.cuda.synchronize()
    return flags.cpu().numpy(), match.cpu().numpy()


def _check(segs, thrs, dev, fills=(0xFF,)):
    pack = segs if isinstance(segs, dict) else pack_segments(segs)
    want = E.coco_flags_host(pack, thrs, want_match=True)
    for fill in fills:
        got = _device(pack, thrs, dev, fill=fill)
        assert np.array_equal(got[0], want[0]), 'flags'
        assert np.array_equal(got[1], want[1]), 'match'
    return got


def _d(*rows):
    return np.array(rows, np.float64).reshape(-1, 5)


def _g(*rows):
    return np.array(rows, np.float64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------ hand cases
def test_iou_exactly_at_the_threshold(dev):
    """a 100 x 50 detection inside a 100 x 100 box: IoU = 5000 / 10000 = 0.5 - matched at 0.5, unmatched at 0.55"""
    flags, match = _check([(_d([0, 0, 100, 50, 0.9]), _g([0, 0, 100, 100]), None, None)], THRS, dev, fills=(0xFF, 0x7F))
    assert match[ALL, :, 0].tolist() == [0, -1] and flags[ALL, :, 0].tolist() == [1, 0]
    # the box (10000) is 'large': ignored in small / medium; the detection (5000) is 'medium'
    assert flags[SMALL, :, 0].tolist() == [2, 2] and flags[MEDIUM, :, 0].tolist() == [2, 0]
    assert flags[LARGE, :, 0].tolist() == [1, 2] and match[LARGE, :, 0].tolist() == [0, -1]


def test_equal_ious_take_the_later_box(dev):
    flags, match = _check([(_d([0, 0, 100, 90, 0.9]), _g([0, 0, 100, 100], [0, 0, 100, 100], [500, 500, 50, 50]), None, None)],
                          THRS, dev)
    assert match[ALL, :, 0].tolist() == [1, 1] and flags[ALL, :, 0].tolist() == [1, 1]


def test_a_regular_box_above_the_threshold_beats_an_ignored_box_with_a_higher_iou(dev):
    # box 0 is a crowd that holds the detection (IoU 1), box 1 a regular box with IoU 0.6; then the same with box 0 ignored by
    # its area field instead (IoU 1 as an ordinary box)
    segs = [(_d([0, 0, 100, 60, 0.9]), _g([0, 0, 200, 200], [0, 0, 100, 100]), None, [1, 0]),
            (_d([0, 0, 100, 100, 0.9]), _g([0, 0, 100, 100], [0, 0, 100, 60]), [500., 6000.], None)]
    flags, match = _check(segs, THRS, dev)
    # rows: t = 0.5, 0.55; columns: the two segments.  In 'all' segment 1's box 0 (area 500) is regular and fits exactly
    assert match[ALL].tolist() == [[1, 0], [1, 0]] and flags[ALL].tolist() == [[1, 1], [1, 1]]
    assert match[MEDIUM].tolist() == [[0, 1], [0, 1]] and flags[MEDIUM].tolist() == [[2, 1], [2, 1]]
    # (medium: segment 0's regular box has area 10000 - ignored there, the crowd takes the detection; segment 1's box 1, area
    #  6000, is regular, box 0 (500) is not)


def test_a_crowd_takes_any_number_of_detections(dev):
    """IoU with a crowd = intersection / the detection's area: two detections inside it, both ignored"""
    segs = [(_d([10, 10, 50, 50, 0.9], [100, 100, 80, 40, 0.8], [150, 150, 100, 100, 0.7]), _g([0, 0, 200, 200]), None, [1])]
    flags, match = _check(segs, THRS, dev)
    # the third lies half outside: intersection 50 x 50 of 100 x 100 = 0.25 - unmatched, and its own area is 'large'
    assert match[ALL].tolist() == [[0, 0, -1]] * 2 and flags[ALL].tolist() == [[2, 2, 0]] * 2
    assert flags[SMALL].tolist() == [[2, 2, 2]] * 2 and flags[LARGE].tolist() == [[2, 2, 0]] * 2


def test_area_bounds_are_inclusive(dev):
    """area exactly 1024 counts in all / small / medium, exactly 9216 in all / medium / large"""
    segs = [(_d([0, 0, 32, 32, 0.9], [300, 300, 96, 96, 0.8]), _g([0, 0, 32, 32], [300, 300, 96, 96]), [1024., 9216.], None)]
    flags, match = _check(segs, THRS, dev)
    assert (match == np.array([0, 1])).all()
    assert flags[:, 0].tolist() == [[1, 1], [1, 2], [1, 1], [2, 1]] and np.array_equal(flags[:, 0], flags[:, 1])


def test_an_unmatched_detection_outside_the_range_is_ignored(dev):
    segs = [(_d([400, 400, 10, 10, 0.9]), _g([0, 0, 50, 50]), None, None)]
    flags, match = _check(segs, THRS, dev)
    assert (match == -1).all() and flags[:, 0, 0].tolist() == [0, 0, 2, 2]            # 100 pixels: all, small


def test_greedy_order_the_higher_score_takes_the_better_box(dev):
    """box A = [0, 100), box B = [30, 130).  The detection scored 0.9 has IoU 0.96 with A and 0.56 with B and takes A; the
    one scored 0.8 fits A better still (0.98) but A is taken: it falls to B (71 / 129 = 0.5504)"""
    segs = [(_d([1, 0, 100, 100, 0.8], [2, 0, 100, 100, 0.9]), _g([0, 0, 100, 100], [30, 0, 100, 100]), None, None)]
    flags, match = _check(segs, THRS, dev)
    assert match[ALL].tolist() == [[0, 1], [0, 1]] and flags[ALL].tolist() == [[1, 1], [1, 1]]
    ten = _check(segs, [float(t) for t in E.IOU_THRS], dev)
    assert ten[1][ALL, 2].tolist() == [0, -1] and ten[0][ALL, 2].tolist() == [1, 0]   # t = 0.6: B is out of reach


def test_empty_segments(dev):
    box, det = _g([10, 10, 40, 40]), _d([10, 10, 40, 40, 0.9], [300, 300, 20, 20, 0.2])
    segs = [(_d(), box, None, None), (det, _g(), None, None), (_d(), _g(), None, None), (det[:1], box, None, None)]
    flags, match = _check(segs, THRS, dev, fills=(0xFF, 0x7F))
    assert match[ALL].tolist() == [[-1, -1, 0]] * 2 and flags[ALL].tolist() == [[0, 0, 1]] * 2
    assert flags[MEDIUM].tolist() == [[0, 2, 1]] * 2 and flags[LARGE].tolist() == [[2, 2, 2]] * 2    # (1600 and 400 pixels)
    none = pack_segments([(_d(), box, None, None), (_d(), _g(), None, None)])
    assert len(none['dets']) == 0
    flags, match = _device(none, THRS, dev)
    assert flags.shape == match.shape == (4, 2, 0)
    assert _device(pack_segments([]), THRS, dev)[0].shape == (4, 2, 0)


# ------------------------------------------------------------------------------------------------------------ capacities
def _grid(n):
    """n boxes of 30 x 30 ('small'), 40 apart"""
    xs, ys = np.meshgrid(np.arange(13) * 40.0, np.arange(12) * 40.0)
    assert n <= xs.size
    return np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 30.0), np.full(xs.size, 30.0)], 1)[:n]


def test_300_detections_on_3_boxes(dev):
    rs = np.random.RandomState(3)
    boxes = _g([10, 10, 40, 40], [100, 10, 40, 40], [10, 100, 60, 60])
    d = np.concatenate([boxes[rs.randint(0, 3, 300)] + rs.uniform(-6, 6, (300, 4)), np.round(rs.uniform(0, 1, (300, 1)), 1)], 1)
    assert 300 > 4 * oadg_coco_match.LDS_DETS
    flags, match = _check([(d, boxes, None, None)], [float(t) for t in E.IOU_THRS], dev)
    assert ((flags[ALL] == 1).sum(axis=1) <= 3).all() and (flags[ALL, 0] == 1).sum() == 3


@pytest.mark.parametrize('cap', sorted({oadg_coco_match.LDS_GTS, oadg_coco_match.LDS_DETS}))
def test_3_detections_on_one_box_more_than_a_capacity(dev, cap):
    """two detections contest the LAST box, one takes box 5; then the same with the tail of the boxes ignored by their area"""
    n = cap + 1
    boxes = _grid(n)
    d3 = np.concatenate([boxes[[n - 1, 5, n - 1]] + [[0, 0, 0, 0], [1, 0, 0, 0], [2, 0, 0, 0]], [[0.5], [0.4], [0.7]]], 1)
    area = np.full(n, 900.0)
    area[n - 30:] = 5000.0                                     # 'medium' by the area field: ignored in 'small'
    flags, match = _check([(d3, boxes, None, None), (d3, boxes, area, None)], THRS, dev)
    # in score order: the detection moved by 2 (IoU 28 / 32 = 0.875), then the unmoved one, then the one on box 5
    assert match[ALL, 0].tolist() == [n - 1, -1, 5] * 2 and flags[ALL, 0].tolist() == [1, 0, 1] * 2
    assert match[SMALL, 0].tolist() == [n - 1, -1, 5, n - 1, -1, 5] and flags[SMALL, 0].tolist() == [1, 0, 1, 2, 0, 1]
    assert flags[MEDIUM, 0].tolist() == [2, 2, 2, 1, 2, 2]     # (900-pixel detections are outside 'medium')


def test_boxes_and_detections_both_beyond_the_capacities(dev):
    rs = np.random.RandomState(4)
    n = oadg_coco_match.LDS_GTS + 1
    boxes = _grid(n)
    many = np.concatenate([boxes[rs.randint(n - 40, n, 130)] + rs.uniform(-3, 3, (130, 4)), rs.uniform(0, 1, (130, 1))], 1)
    crowd = (np.arange(n) % 9 == 0).astype(np.uint8)
    area = np.where(np.arange(n) % 4 == 0, 5000.0, 900.0)
    ten = [float(t) for t in E.IOU_THRS]
    segs = [(many, boxes, area, crowd), (many[:3], boxes[:3], None, None), (many[:70], boxes[:n - 1], area[:n - 1], None)]
    flags, match = _check(segs, ten, dev, fills=(0xFF, 0x7F))
    assert match.max() == n - 1 and {0, 1, 2} <= set(np.unique(flags[ALL]).tolist())


# ------------------------------------------------------------------------------------------------------------ seeded sweep
@pytest.mark.parametrize('fractional', [False, True])
def test_seeded_sweep_equals_the_host(dev, fractional):
    rs = np.random.RandomState(21 + fractional)
    segs = []
    for _ in range(200):
        k, m = rs.randint(0, 41), rs.randint(0, 41)
        xy = rs.uniform(0, 160, (k, 2))
        g = np.concatenate([xy, np.exp(rs.uniform(np.log(4), np.log(180), (k, 2)))], 1)
        src = g[rs.randint(0, k, m // 2)] + rs.uniform(-5, 5, (m // 2, 4)) if k else np.zeros((0, 4))
        xy = rs.uniform(0, 160, (m - len(src), 2))
        d = np.concatenate([src, np.concatenate([xy, np.exp(rs.uniform(np.log(4), np.log(180), (len(xy), 2)))], 1)])
        if not fractional:
            g, d = np.round(g), np.round(d)
        scores = np.round(rs.uniform(0, 1, (m, 1)), 1 if rs.randint(2) else 6)        # (one decimal: equal scores)
        segs.append((np.concatenate([d, scores], 1), g, None, rs.uniform(size=k) < 0.15))
    pack = pack_segments(segs)
    flags, match = _check(pack, [float(t) for t in E.IOU_THRS], dev)
    for a in range(4):                                         # a degenerate generator cannot hide a failure
        assert set(np.unique(flags[a]).tolist()) == {0, 1, 2}, a
        assert min((flags[a] == v).sum() for v in (0, 1, 2)) >= 100, a


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def split():
    return seeded_split(0, n_img=30, n_cls=5)


@pytest.mark.parametrize('max_dets,names', [(None, None), (E.MMDET_MAX_DETS, E.MMDET_METRICS)])
def test_coco_eval_bbox_on_the_device_equals_the_host(dev, split, max_dets, names):
    gt_anns, results = split
    want = E.coco_eval_bbox(gt_anns, results, 5, max_dets=max_dets, names=names)
    got = E.coco_eval_bbox(gt_anns, results, 5, max_dets=max_dets, names=names, device=dev)
    assert got == want and list(got) == list(want) and all(v > 0 for v in want.values())
    pack = E.pack_coco_segments(gt_anns, results, 5, 100)
    flags, match = E.coco_flags_device(pack, E.IOU_THRS, E.AREA_RNG, dev, want_match=True)
    want_flags, want_match = E.coco_flags_host(pack, want_match=True)
    assert np.array_equal(flags, want_flags) and np.array_equal(match, want_match)


def test_coco_format_dataset_evaluates_on_the_device(dev, tmp_path):
    from oadg_amd.datasets import CocoDataset
    gt_anns, results = seeded_split(2, n_img=6, n_cls=2)
    images = [dict(id=10 + i, file_name=f'{i}.png', height=384, width=640) for i in range(6)]
    anns = [dict(id=0, image_id=10 + i, category_id=3 + g['category'], iscrowd=g['iscrowd'], area=g['area'], bbox=g['bbox'])
            for i, per in enumerate(gt_anns) for g in per]
    for k, a in enumerate(anns):
        a['id'] = 100 + k
    assert any(a['iscrowd'] for a in anns)
    with open(tmp_path / 'ann.json', 'w') as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=3, name='car'), dict(id=4, name='person')]), f)
    ds = CocoDataset(str(tmp_path / 'ann.json'), classes=('car', 'person'), img_prefix=str(tmp_path), device='cpu', test_mode=True)
    assert len(ds) == 6 and E.voc_device() is not None
    got = ds.evaluate(results, metric='bbox')
    assert got == ds.evaluate(results, metric='bbox', device=None) and got['bbox_mAP'] > 0
    assert got == ds.evaluate(results, metric='bbox', device=dev)


# ------------------------------------------------------------------------------------------------ arguments, repeatability
def test_arguments_short_workspace_and_repeatability(dev):
    rs = np.random.RandomState(5)
    n = oadg_coco_match.LDS_GTS + 12
    boxes = _grid(n)
    d = np.concatenate([boxes[rs.randint(0, n, 90)] + rs.uniform(-5, 5, (90, 4)), rs.uniform(0, 1, (90, 1))], 1)
    pack = pack_segments([(d, boxes, None, rs.uniform(size=n) < 0.15), (d[:20], boxes[:9], None, None)])
    ten = [float(t) for t in E.IOU_THRS]
    with pytest.raises(ValueError, match='matchings per call'):
        _device(pack, ten + [0.96, 0.97, 0.98, 0.99, 0.995, 0.996, 0.997], dev)          # 17 x 4 = 68 > 64
    with pytest.raises(RuntimeError, match='argument error -2'):                          # OADG_ESIZE
        _device(pack, ten, dev, workspace=torch.empty(8 * len(pack['gts']) - 8, dtype=torch.uint8, device=dev))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_coco_match.coco_match(*[torch.from_numpy(pack[k]) for k in KEYS], _cap(ten), E.AREA_RNG)
    with pytest.raises(ValueError, match='contiguous'):
        up = [torch.from_numpy(pack[k]).to(dev) for k in KEYS]
        oadg_coco_match.coco_match(up[0].float(), *up[1:], _cap(ten), E.AREA_RNG)
    # sixteen thresholds x four ranges fill all 64 lanes; one threshold x one range uses one
    sixteen = _device(pack, ten + [0.96, 0.97, 0.98, 0.99, 0.995, 0.996], dev)
    a = _check(pack, ten, dev)
    assert np.array_equal(sixteen[0][:, :10], a[0]) and np.array_equal(sixteen[1][:, :10], a[1])
    one = _device(pack, [0.5], dev, area_rng=[E.AREA_RNG[1]])
    assert np.array_equal(one[0][0, 0], a[0][SMALL, 0]) and np.array_equal(one[1][0, 0], a[1][SMALL, 0])
    # match is optional: flags alone are the same bytes, and nothing touches the buffer that was not handed in
    alone, untouched = _device(pack, ten, dev, want_match=False)
    assert alone.tobytes() == a[0].tobytes() and (untouched == -1).all()
    b = _device(pack, ten, dev)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert len({tuple(f) for f in a[0][ALL].tolist()}) > 1                               # the thresholds do not all agree
