"""CPU: proposal recall on the host - ``eval_recalls`` against the reference's own output (tests/golden/recall_reference.npz,
made by tests/golden/make_golden_recall.py), hand cases with the values written out, the incremental form of the matching that
csrc/recall.hip runs, ``proposal_evaluate``'s three metrics, ``fast_eval_recall`` and the 'RPN' detector's surface."""
import json
import os
import sys

import numpy as np
import pytest

from oadg_amd import evaluation as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'recall_reference.npz')
CONVENTIONS = (False, True)                   # use_legacy_coordinate of recalls_0 / recalls_1

GTS = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]], np.float32)
PROPS = np.array([[0, 0, 10, 10, .9], [0, 0, 10, 5, .8], [20, 20, 30, 30, .7]], np.float32)


def load_fixture():
    z = np.load(GOLDEN)
    n = int(z['n_img'])
    gts = [z[f'gt_{i}'] if z['has_gt'][i] else None for i in range(n)]
    props = [z[f'prop_{i}'] for i in range(n)]
    return z, gts, props


def incremental_ious(pack, legacy):
    """the matching as csrc/recall.hip runs it, without a matrix: per box a cached (best IoU over the live columns, lowest
    column that attains it); a round takes the largest cached value at the lowest box, retires that box and its column and
    recomputes only the live boxes whose cached column has just retired"""
    props, p_off, gts, g_off, nums = (pack[k] for k in ('props', 'prop_off', 'gts', 'gt_off', 'nums'))
    out = np.full((len(nums), len(gts)), np.nan, np.float32)
    for i in range(len(g_off) - 1):
        g, p = gts[g_off[i]:g_off[i + 1]], props[p_off[i]:p_off[i + 1]]
        for k, num in enumerate(nums):
            n, o = min(int(num), len(p)), out[k, g_off[i]:g_off[i + 1]]
            if len(g) == 0:
                continue
            if n == 0:
                o[:] = 0
                continue
            dead = np.zeros(n, bool)

            def best(b):
                row = E.bbox_overlaps_voc(g[b:b + 1], p[:n], legacy)[0]
                row[dead] = -1
                return row.max(), int(row.argmax())
            val, col = map(list, zip(*[best(b) for b in range(len(g))]))
            live = n
            for j in range(len(g)):
                if live == 0:
                    o[j:] = -1
                    break
                b = int(np.argmax(val))
                o[j], c = val[b], col[b]
                val[b], col[b], dead[c] = -2.0, -1, True
                live -= 1
                if live:
                    for r in range(len(g)):
                        if val[r] > -2 and col[r] == c:
                            val[r], col[r] = best(r)
    return out


# ------------------------------------------------------------------------------------------------ the reference's output
@pytest.mark.parametrize('c', (0, 1))
def test_host_eval_recalls_equals_the_reference(c):
    z, gts, props = load_fixture()
    got = E.eval_recalls(gts, props, list(z['nums']), z['thrs'], logger='silent', use_legacy_coordinate=CONVENTIONS[c])
    assert got.dtype == np.float64 and got.shape == (4, 10)
    assert np.array_equal(got, z[f'recalls_{c}'])
    pack = E.pack_recall(gts, props, list(z['nums']))
    ious = E.recall_ious_host(pack, CONVENTIONS[c])
    assert (ious == -1).sum() > 0 and (ious == 0).sum() > 0                    # surplus rounds, and boxes without proposals
    for i, g in enumerate(gts):                                              # the IoUs themselves are the reference's
        if g is not None and len(g) and f'iou_{c}_{i}' in z.files:
            mine = E.bbox_overlaps_voc(g, pack['props'][pack['prop_off'][i]:pack['prop_off'][i + 1]], CONVENTIONS[c])
            assert np.array_equal(mine, z[f'iou_{c}_{i}'])


def test_the_fixture_proves_something():
    z, gts, props = load_fixture()
    ar = [z[f'recalls_{c}'].mean(axis=1) for c in (0, 1)]
    assert all((np.diff(a) > 0).all() for a in ar) and not np.array_equal(z['recalls_0'], z['recalls_1'])
    assert any(g is None for g in gts) and any(len(p) > 1000 for p in props)
    s = np.concatenate([p[:, 4] for p in props])
    assert len(np.unique(s)) == len(s)


@pytest.mark.parametrize('legacy', CONVENTIONS)
def test_the_incremental_matching_is_the_reference_loop(legacy):
    z, gts, props = load_fixture()
    pack = E.pack_recall(gts, props, list(z['nums']))
    assert np.array_equal(incremental_ious(pack, legacy), E.recall_ious_host(pack, legacy))


# ------------------------------------------------------------------------------------------------ by hand
def test_hand_case_round_order_and_recalls():
    pack = E.pack_recall([GTS], [PROPS], [1, 2, 3])
    assert pack['nums'].tolist() == [1, 2, 3] and pack['props'].dtype == np.float32 and pack['prop_off'].tolist() == [0, 3]
    ious = E.recall_ious_host(pack)
    assert ious.tolist() == [[1, -1, -1], [1, .5, -1], [1, 1, .5]]
    assert np.array_equal(incremental_ious(pack, False), ious)
    rec = E.eval_recalls([GTS], [PROPS], [1, 2, 3], [0.5, 0.75], logger='silent')
    assert rec.tolist() == [[1 / 3, 1 / 3], [2 / 3, 1 / 3], [1, 2 / 3]]
    assert E.eval_recalls([GTS], [PROPS], 3, None, logger='silent').tolist() == [[1.0]]          # an int, and the default 0.5


def test_a_zero_iou_box_consumes_the_lowest_live_proposal():
    gts = np.array([[0, 0, 10, 10], [100, 100, 110, 110]], np.float32)           # the second box meets no proposal
    props = np.array([[50, 50, 60, 60], [0, 0, 10, 10], [0, 0, 10, 8]], np.float32)          # [n, 4]: kept in this order
    pack = E.pack_recall([gts, gts[:1]], [props, props], [2, 3])
    ious = E.recall_ious_host(pack)
    # budget 2: box 0 takes column 1 (1.0), box 1 takes column 0 at IoU 0; the second image: 1.0
    assert ious[0].tolist() == [1, 0, 1] and ious[1].tolist() == [1, 0, 1]
    # the lowest live column went with the zero: with the boxes swapped, box 0 (IoU 0 everywhere) is round 2 all the same
    pack = E.pack_recall([gts[::-1]], [props[[1, 0]]], [2])
    assert E.recall_ious_host(pack).tolist() == [[1, 0]]
    # ... and it is gone: a third box that overlapped only column 0 finds nothing once the zero-IoU round has come first
    three = np.array([[100, 100, 110, 110], [200, 200, 210, 210], [50, 50, 60, 58]], np.float32)
    pack = E.pack_recall([three], [props[:1]], [1])
    assert E.recall_ious_host(pack).tolist() == [[np.float32(0.8), -1, -1]]
    assert np.array_equal(incremental_ious(pack, False), E.recall_ious_host(pack))


def test_budgets_are_capped_at_the_last_one_and_equal_scores_keep_index_order():
    pack = E.pack_recall([GTS], [PROPS], [5, 2])
    assert pack['nums'].tolist() == [2, 2] and len(pack['props']) == 2             # (ious[:, :5] of two columns)
    assert E.recall_ious_host(pack).tolist() == [[1, .5, -1], [1, .5, -1]]
    tied = np.array([[0, 0, 10, 5, .5], [0, 0, 10, 10, .5], [20, 20, 30, 30, .9], [0, 0, 10, 8, .5]], np.float32)
    pack = E.pack_recall([None], [tied], [4])
    assert pack['props'].tolist() == [[20, 20, 30, 30], [0, 0, 10, 5], [0, 0, 10, 10], [0, 0, 10, 8]]
    assert pack['gt_off'].tolist() == [0, 0] and pack['gts'].shape == (0, 4)
    assert pack['props'].ctypes.data % 16 == 0 and pack['gts'].ctypes.data % 16 == 0


def test_bad_inputs_raise_and_no_box_is_nan():
    bad = GTS.copy()
    bad[1, 2] = np.inf
    with pytest.raises(ValueError, match='not finite'):
        E.pack_recall([bad], [PROPS], [3])
    nanp = PROPS.copy()
    nanp[0, 0] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        E.pack_recall([GTS], [nanp], [3])
    nans = PROPS.copy()
    nans[1, 4] = np.nan
    with pytest.raises(ValueError, match='score is NaN'):
        E.pack_recall([GTS], [nans], [3])
    with pytest.raises(ValueError, match='images'):
        E.pack_recall([GTS], [PROPS, PROPS], [3])
    with pytest.raises(TypeError, match='proposal_nums'):
        E.eval_recalls([GTS], [PROPS])
    rec = E.eval_recalls([None, np.zeros((0, 4))], [PROPS, PROPS[:0]], [1, 3], [0.5, 0.75], logger='silent')
    assert rec.shape == (2, 2) and np.isnan(rec).all()


def test_thresholds_are_compared_in_fp64():
    v = np.float32(0.7)                               # 0.699999988: below the fp64 0.7, equal to it in fp32
    rec = E.recalls_from_ious(np.array([[v, 1.0]], np.float32), [0.7, float(v)])
    assert rec.tolist() == [[0.5, 1.0]]


def test_recall_summary_is_a_plain_table(capsys):
    text = E.print_recall_summary(np.array([[.25, .125], [1, .5]]), [100, 1000], [.5, .75], logger='silent')
    assert capsys.readouterr().out == ''
    rows = [ln for ln in text.splitlines() if ln.startswith('|')]
    assert [c.strip() for c in rows[1].split('|')[1:-1]] == ['100', '0.250', '0.125']
    assert [c.strip() for c in rows[2].split('|')[1:-1]] == ['1000', '1.000', '0.500']
    E.print_recall_summary(np.array([[.25]]), [1], [.5])
    assert '0.250' in capsys.readouterr().out


# ------------------------------------------------------------------------------------------------ proposal_evaluate
def _synthetic(n=3, num_boxes=4):
    from oadg_amd.pipelines import SyntheticCityscapes
    return SyntheticCityscapes(img_shape=(128, 256), num_boxes=num_boxes, num_classes=3, length=n, box_size=(16, 80),
                               device='cpu')


def _proposals(ds, seed=0):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(len(ds)):
        b = ds.boxes(i)[0]
        d = np.concatenate([b[:3] + rs.uniform(-3, 3, (3, 4)), b[:2] + rs.uniform(-12, 12, (2, 4)), rs.uniform(0, 100, (6, 4))])
        out.append(np.concatenate([d, np.arange(len(d), 0, -1)[:, None] / 20.0], axis=1).astype(np.float32))     # (tight ones first)
    return out


def test_proposal_fast_and_recall_dicts():
    ds = _synthetic()
    res = _proposals(ds)
    boxes = [ds.boxes(i)[0] for i in range(len(ds))]
    fast = E.proposal_evaluate(ds, res, 'proposal_fast', logger='silent', device=None, proposal_nums=(1, 3, 10))
    want = E.eval_recalls(boxes, res, [1, 3, 10], E.IOU_THRS, logger='silent').mean(axis=1)
    assert list(fast) == ['AR@1', 'AR@3', 'AR@10'] and list(fast.values()) == want.tolist()
    assert 0 < fast['AR@1'] < fast['AR@3'] <= fast['AR@10'] and all(type(v) is float for v in fast.values())
    one = E.proposal_evaluate(ds, res, ['recall'], logger='silent', device=None, proposal_nums=(3, 10))
    rec = E.eval_recalls(boxes, res, [3, 10], [0.5], logger='silent')
    assert list(one) == ['recall@3@0.5', 'recall@10@0.5'] and list(one.values()) == rec[:, 0].tolist()
    two = E.proposal_evaluate(ds, res, 'recall', logger='silent', device=None, proposal_nums=(3, 10), iou_thr=[0.5, 0.75])
    rec = E.eval_recalls(boxes, res, [3, 10], [0.5, 0.75], logger='silent')
    assert list(two) == ['recall@3@0.5', 'recall@3@0.75', 'recall@10@0.5', 'recall@10@0.75', 'AR@3', 'AR@10']
    assert [two['AR@3'], two['AR@10']] == rec.mean(axis=1).tolist() and two['recall@10@0.75'] == rec[1, 1]
    json.dumps(two)
    with pytest.raises(TypeError, match='one \\[n, 5\\] array of proposals per image'):
        E.proposal_evaluate(ds, [[r] for r in res], 'proposal_fast', device=None)
    with pytest.raises(KeyError, match='bbox'):
        E.proposal_evaluate(ds, res, 'bbox', device=None)
    with pytest.raises(ValueError, match='2 results for 3 images'):
        E.proposal_evaluate(ds, res[:2], 'recall', device=None)


def test_sdgod_recall_uses_the_legacy_extents(tmp_path):
    from oadg_amd.datasets import SdgodDataset, XMLDataset
    from test_sdgod_dataset import _obj, write_voc
    tree = {n: (96, 160, True, [_obj('car', (10, 20, 90, 70)), _obj('person', (100, 10, 140, 80))]) for n in ('a', 'b')}
    prefix = write_voc(str(tmp_path), tree)
    kw = dict(ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix, device='cpu', test_mode=True)
    ds = SdgodDataset(**kw)
    # the car: 71 / 80 = 0.8875 with modern extents, 72 / 81 = 0.8889 with the legacy ones; the person: 0.775 / 0.780
    res = [np.array([[9, 19, 80, 69, .9], [99, 9, 130, 79, .8]], np.float32)] * 2
    boxes = [ds.get_ann_info(i)['bboxes'] for i in range(2)]
    got = E.proposal_evaluate(ds, res, 'recall', logger='silent', device=None, proposal_nums=(1, 2), iou_thr=[0.5, 0.888])
    legacy = E.eval_recalls(boxes, res, [1, 2], [0.5, 0.888], logger='silent', use_legacy_coordinate=True)
    modern = E.eval_recalls(boxes, res, [1, 2], [0.5, 0.888], logger='silent')
    assert got['recall@2@0.888'] == legacy[1, 1] == 0.5 and modern[1, 1] == 0.0
    xml = XMLDataset(classes=SdgodDataset.CLASSES, **kw)
    got = E.proposal_evaluate(xml, res, 'recall', logger='silent', device=None, proposal_nums=(1, 2), iou_thr=[0.5, 0.888])
    assert got['recall@2@0.888'] == modern[1, 1]
    with pytest.raises(KeyError, match='proposal_fast'):
        E.proposal_evaluate(ds, res, 'proposal_fast', device=None)
    with pytest.raises(NotImplementedError, match="'recall'.*proposal_evaluate"):          # evaluate says where to go
        ds.evaluate(res, metric='recall')


def test_proposal_is_class_agnostic_where_bbox_is_not():
    ds = _synthetic(n=1, num_boxes=1)
    box, label = ds.boxes(0)
    c = int(label[0])
    other = (c + 1) % 3
    res = [[np.concatenate([box, [[0.9]]], axis=1).astype(np.float32) if k == other else np.zeros((0, 5), np.float32)
            for k in range(3)]]
    got = E.proposal_evaluate(ds, res, 'proposal', logger='silent', device=None)
    assert list(got) == ['AR@100', 'AR@300', 'AR@1000', 'AR_s@1000', 'AR_m@1000', 'AR_l@1000']
    assert got['AR@100'] == got['AR@1000'] == 1.0
    bbox = E.coco_eval_bbox(E.dataset_gt_anns(ds), res, 3, max_dets=E.MMDET_MAX_DETS, names=E.MMDET_METRICS)
    assert bbox['AR@1000'] == 0.0
    # the [n, 5] array of an RPN detector is the same list of detections; metric_items picks positions by name
    arr = [np.concatenate(res[0])]
    assert E.proposal_evaluate(ds, arr, 'proposal', logger='silent', device=None) == got
    assert E.proposal_evaluate(ds, arr, 'proposal', logger='silent', device=None, metric_items='AR@300') == {'AR@300': 1.0}
    with pytest.raises(KeyError, match='AR@7'):
        E.proposal_evaluate(ds, arr, 'proposal', device=None, metric_items=['AR@7'])
    with pytest.raises(NotImplementedError, match="'iou_thrs'"):
        E.proposal_evaluate(ds, arr, 'proposal', device=None, iou_thrs=[0.5])


def test_fast_eval_recall_drops_crowds_and_ignored(tmp_path):
    from oadg_amd.datasets import CocoDataset
    anns = [dict(id=1, image_id=1, category_id=1, bbox=[0, 0, 10, 10], area=100, iscrowd=0),
            dict(id=2, image_id=1, category_id=1, bbox=[20, 20, 10, 10], area=100, iscrowd=1),
            dict(id=3, image_id=1, category_id=2, bbox=[40, 40, 10, 10], area=100, iscrowd=0, ignore=True),
            dict(id=4, image_id=1, category_id=2, bbox=[60, 60, 10, 10], area=100, iscrowd=0)]
    path = tmp_path / 'a.json'
    path.write_text(json.dumps(dict(images=[dict(id=1, file_name='a.png', width=100, height=100),
                                            dict(id=2, file_name='b.png', width=100, height=100)],
                                    categories=[dict(id=1, name='x'), dict(id=2, name='y')], annotations=anns)))
    ds = CocoDataset(ann_file=str(path), classes=('x', 'y'), device='cpu', test_mode=True)
    boxes = E.coco_recall_boxes(ds)
    assert boxes[0].tolist() == [[0, 0, 10, 10], [60, 60, 70, 70]] and boxes[0].dtype == np.float32
    assert boxes[1].shape == (0, 4)
    res = [np.array([[0, 0, 10, 10, .9], [20, 20, 30, 30, .8], [40, 40, 50, 50, .7]], np.float32), np.zeros((0, 5), np.float32)]
    ar = ds.fast_eval_recall(res, [1, 3], [0.5, 0.75], logger='silent', device=None)
    assert ar.tolist() == [0.5, 0.5]                       # the crowd and the ignored box are not asked for
    fast = E.proposal_evaluate(ds, res, 'proposal_fast', logger='silent', device=None, proposal_nums=(1, 3))
    assert fast == {'AR@1': 0.5, 'AR@3': 0.5}


# ------------------------------------------------------------------------------------------------ the detector
def test_rpn_builds_from_the_new_configs_and_does_not_train():
    import torch
    from oadg_amd import Config, build_detector
    from oadg_amd.detectors import RPN
    for name, base, n_levels in (('rpn_r50_fpn_1x_cityscapes.py', 'faster_rcnn_r50_fpn_1x_cityscapes.py', 5),
                                 ('rpn_r101_dc5_1x_dwd_sdgod_test.py', 'faster_rcnn_r101_dc5_1x_dwd_oadg_sdgod_test.py', 1)):
        cfg = Config.fromfile(os.path.join(ROOT, 'configs', 'rpn', name))
        frcnn = Config.fromfile(os.path.join(ROOT, 'configs', 'oadg', base))
        assert cfg.model.type == 'RPN' and cfg.model.roi_head is None and list(cfg.model.test_cfg) == ['rpn']
        assert cfg.model.test_cfg.rpn == frcnn.model.test_cfg.rpn              # the proposals its second stage really sees
        assert cfg.data.test == frcnn.data.test
        cfg.model.pop('pretrained', None)
        cfg.model.backbone.init_cfg = None
        model = build_detector(cfg.model)
        assert isinstance(model, RPN) and not hasattr(model, 'roi_head')
        assert len(model.rpn_head.prior_generator.strides) == n_levels and (model.neck is None) == (n_levels == 1)
        keys = set(model.state_dict())
        assert keys and all(k.startswith(('backbone.', 'neck.', 'rpn_head.')) for k in keys)
    with pytest.raises(NotImplementedError, match='RPN.forward_train'):
        model(torch.zeros(1, 3, 32, 32), [dict()], return_loss=True, gt_bboxes=[torch.zeros(0, 4)])
    with pytest.raises(TypeError, match='roi_head'):
        build_detector(dict(cfg.model, roi_head=dict(type='StandardRoIHead')))


def test_rpn_results_are_drawn_as_twenty_proposals():
    from oadg_amd import visualization as V
    props = np.concatenate([np.tile([[2, 3, 40, 50]], (30, 1)), np.linspace(1, 0, 30)[:, None]], axis=1).astype(np.float32)
    items, text = V.proposal_items(props)
    assert len(items) == 3 * V.PROPOSAL_TOP_K == 60 and text.startswith(b'proposal|1.00')
    assert len(V.proposal_items(props, top_k=0)[0]) == 90 and len(V.proposal_items(props[:0])[0]) == 0


def test_the_test_tool_scores_the_images_it_tested_across_a_seam(tmp_path):
    """tools/test.py ``score_proposals``: the first len(results) images (tools/test_dwd.py's ``first_images``), a concatenation
    as ``ConcatDataset.evaluate`` scores it, a concatenation of one with that dataset's plain keys"""
    import importlib.util
    from oadg_amd.datasets import ConcatDataset, SdgodDataset
    from test_sdgod_dataset import _obj, write_voc
    spec = importlib.util.spec_from_file_location('oadg_tools_test_recall', os.path.join(ROOT, 'tools', 'test.py'))
    T = importlib.util.module_from_spec(spec)
    sys.path.insert(0, os.path.join(ROOT, 'tools'))                    # (the tools import each other by name)
    try:
        spec.loader.exec_module(T)
    finally:
        sys.path.pop(0)
    parts = []
    for k in range(2):
        tree = {n: (96, 160, True, [_obj('car', (10 + 5 * k, 20, 90, 70))]) for n in ('a', 'b')}
        prefix = write_voc(str(tmp_path / f'dom{k}'), tree)
        parts.append(SdgodDataset(ann_file=prefix + 'ImageSets/Main/train.txt', img_prefix=prefix, device='cpu', test_mode=True))
    res = [np.array([[9, 19, 80, 69, .9]], np.float32), np.array([[0, 0, 5, 5, .9]], np.float32),
           np.array([[14, 19, 89, 69, .9]], np.float32)]
    opts = dict(proposal_nums='(1, 2)', iou_thr='0.5')
    kw = dict(logger='silent', device=None, proposal_nums=(1, 2), iou_thr=0.5)
    got = T.score_proposals(ConcatDataset(parts), res, 'recall', opts)                      # three of the four images
    first, second = E.proposal_evaluate(parts[0], res[:2], 'recall', **kw), \
        E.proposal_evaluate(T._dwd_tool().first_images(parts[1], 1), res[2:], 'recall', **kw)
    assert got == {**{f'0_{k}': v for k, v in first.items()}, **{f'1_{k}': v for k, v in second.items()}}
    assert got['0_recall@2@0.5'] == 0.5 and got['1_recall@2@0.5'] == 1.0
    assert T.score_proposals(ConcatDataset(parts[:1]), res[:2], 'recall', opts) == first
    assert T.score_proposals(ConcatDataset(parts), res[:2], 'recall', opts) == first           # the second tree holds nothing
    assert len(parts[1]) == 2
    assert T.count_rows(res) == '3 proposals' and T.count_rows([[r, r[:0]] for r in res]) == '3 detections'
