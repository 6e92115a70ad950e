"""GPU: csrc/recall.hip against the host yardstick (evaluation.recall_ious_host, which tests/test_recall.py pins to the
reference's own output) - bit for bit -, the 'RPN' detector against the first stage of a Faster R-CNN with the same weights,
and the two command lines."""
import ast
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import oadg_recall
from oadg_amd import evaluation as E
from test_recall import CONVENTIONS, GTS, PROPS, load_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_CAP, G_CAP = oadg_recall.LDS_PROPS, oadg_recall.LDS_GTS


def _device(pack, legacy, dev, fill=0xFF, workspace=None):
    up = [torch.from_numpy(pack[k]).to(dev) for k in oadg_recall.KEYS]
    K, G = len(pack['nums']), len(pack['gts'])
    out = torch.full((4 * K * G,), fill, dtype=torch.uint8, device=dev).view(torch.float32).view(K, G)
    oadg_recall.recall_match(*up, pack['nums'], legacy, out=out, workspace=workspace)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(gts, props, nums, legacy, dev, fill=0xFF):
    pack = E.pack_recall(gts, props, nums)
    want, got = E.recall_ious_host(pack, legacy), _device(pack, legacy, dev, fill)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
        f'{int((got.view(np.uint32) != want.view(np.uint32)).sum())} of {got.size} matched IoUs differ'
    return got


def _image(rs, g, p, integer, W=320, H=200):
    """g boxes and p scored proposals: jittered copies of the boxes, exact copies (equal IoUs) and random boxes"""
    def boxes(n):
        x1, y1 = rs.uniform(0, W - 50, n), rs.uniform(0, H - 40, n)
        return np.stack([x1, y1, x1 + rs.uniform(6, 90, n), y1 + rs.uniform(6, 70, n)], axis=1)
    gt = boxes(g)
    parts = [np.zeros((0, 4))]
    if g:
        parts += [gt + rs.uniform(-s, s, gt.shape) for s in (2, 6, 15)] + [gt[: max(1, g // 3)]] * 2
    d = np.concatenate(parts + [boxes(p)])
    d = d[rs.permutation(len(d))[:p]]
    if integer:
        gt, d = np.round(gt), np.round(d)
    return gt.astype(np.float32), np.concatenate([d, rs.uniform(0, 1, (len(d), 1))], axis=1).astype(np.float32)


def _split(rs, counts, integer=None):
    pairs = [_image(rs, g, p, i % 2 == 0 if integer is None else integer) for i, (g, p) in enumerate(counts)]
    return [a for a, _ in pairs], [b for _, b in pairs]


# ------------------------------------------------------------------------------------------------ the kernel
def test_hand_cases(dev):
    got = _check([GTS], [PROPS], [1, 2, 3], False, dev)
    assert got.tolist() == [[1, -1, -1], [1, .5, -1], [1, 1, .5]]
    gts = np.array([[0, 0, 10, 10], [100, 100, 110, 110]], np.float32)           # the second box meets no proposal
    props = np.array([[50, 50, 60, 60], [0, 0, 10, 10], [0, 0, 10, 8]], np.float32)
    assert _check([gts, gts[:1]], [props, props], [2, 3], False, dev).tolist() == [[1, 0, 1], [1, 0, 1]]
    three = np.array([[100, 100, 110, 110], [200, 200, 210, 210], [50, 50, 60, 58]], np.float32)
    assert _check([three], [props[:1]], [1], False, dev, fill=0x7F).tolist() == [[np.float32(0.8), -1, -1]]
    got = _check([GTS], [PROPS], [5, 2], True, dev)                              # capped budgets; 11 x 6 of 11 x 11 pixels
    assert np.array_equal(got, np.array([[1, np.float32(66) / np.float32(121), -1]] * 2, np.float32))


def test_empty_images_of_every_kind(dev):
    none = np.zeros((0, 4), np.float32)
    for fill in (0xFF, 0x7F):
        got = _check([none, GTS, None, GTS, none, GTS], [PROPS, PROPS[:0], PROPS, PROPS, PROPS[:0], PROPS[:0]], [0, 1, 3], False,
                     dev, fill)
        assert got.shape == (3, 9) and (got[0] == 0).all()                       # a budget of 0: no column either
        assert got[2].tolist() == [0, 0, 0, 1, 1, .5, 0, 0, 0]
    assert _check([none, None], [PROPS, PROPS[:0]], [3], False, dev).shape == (1, 0)           # no box in the split
    assert _check([GTS], [PROPS[:0]], [3], False, dev).tolist() == [[0, 0, 0]]               # no proposal in the split
    assert _check([], [], [1, 3], False, dev).shape == (2, 0)                            # N = 0


@pytest.mark.parametrize('legacy', CONVENTIONS)
def test_the_wave_width(dev, legacy):
    rs = np.random.RandomState(3)
    counts = [(g, p) for g in (63, 64, 65) for p in (63, 64, 65)] + [(1, 65), (65, 1), (130, 129)]
    gts, props = _split(rs, counts)
    got = _check(gts, props, [1, 63, 64, 65, 200], legacy, dev)
    assert (got == -1).any() and (got > 0.5).any()


def test_either_side_of_the_lds_capacities(dev):
    rs = np.random.RandomState(4)
    # proposals: budgets one below, at and above the capacity see 1023 / 1024 / 1025 columns of the same image
    gts, props = _split(rs, [(7, P_CAP - 1), (7, P_CAP), (7, P_CAP + 1), (3, 2 * P_CAP + 5)])
    _check(gts, props, [P_CAP - 1, P_CAP, P_CAP + 1, 3 * P_CAP], False, dev)
    # boxes: cached pairs in LDS up to the capacity, in the workspace beyond - with fewer and with more columns than boxes
    gts, props = _split(rs, [(G_CAP - 1, 40), (G_CAP, 40), (G_CAP + 1, 40), (G_CAP + 1, 300), (G_CAP, 300)])
    got = _check(gts, props, [40, 300], True, dev, fill=0x7F)
    assert (got == -1).sum() >= 2 * (3 * G_CAP - 120)
    # both beyond at once
    gts, props = _split(rs, [(G_CAP + 1, P_CAP + 1), (2, 3)], integer=True)
    _check(gts, props, [P_CAP, P_CAP + 1], False, dev)


@pytest.mark.parametrize('legacy', CONVENTIONS)
def test_seeded_sweep_equals_the_host(dev, legacy):
    rs = np.random.RandomState(5 + legacy)
    counts = [(int(rs.randint(0, 41)), int(rs.randint(0, 301))) for _ in range(38)] + [(5, 0), (0, 7)]
    gts, props = _split(rs, counts)
    got = _check(gts, props, [1, 10, 100, 300], legacy, dev)
    assert (got == -1).any() and (got == 0).any() and len(np.unique(got)) > 100
    # ties occur: some IoU is attained by two proposals of an image with integer coordinates
    pack = E.pack_recall(gts, props, [300])
    tied = 0
    for i in range(0, 40, 2):
        m = E.bbox_overlaps_voc(pack['gts'][pack['gt_off'][i]:pack['gt_off'][i + 1]],
                                pack['props'][pack['prop_off'][i]:pack['prop_off'][i + 1]], legacy)
        tied += sum(int(row.size > 1 and (row == row.max()).sum() > 1 and row.max() > 0) for row in m)
    assert tied > 0


def test_arguments_workspace_and_repeatability(dev):
    rs = np.random.RandomState(6)
    gts, props = _split(rs, [(G_CAP + 3, 50), (5, 9)])
    pack = E.pack_recall(gts, props, [10, 50])
    a = _device(pack, False, dev)
    need = 2 * (8 * len(pack['gts']) + len(pack['props']))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    b = _device(pack, False, dev, fill=0x7F, workspace=ws)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    with pytest.raises(RuntimeError, match='oadg_recall_match'):
        _device(pack, False, dev, workspace=ws[:need - 1])
    with pytest.raises(ValueError, match='budgets'):
        _device(dict(pack, nums=np.arange(oadg_recall.MAX_NUMS + 1, dtype=np.int32)), False, dev)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        oadg_recall.recall_match(*[torch.from_numpy(pack[k]) for k in oadg_recall.KEYS], [1], False)
    # more budgets than one call takes: ious_device makes two calls
    nums = list(range(1, oadg_recall.MAX_NUMS + 4))
    pack = E.pack_recall(gts, props, nums)
    assert np.array_equal(E.recall_ious_device(pack, True, dev), E.recall_ious_host(pack, True))


@pytest.mark.parametrize('c', (0, 1))
def test_eval_recalls_on_the_device_equals_the_reference(dev, c):
    z, gts, props = load_fixture()
    got = E.eval_recalls(gts, props, list(z['nums']), z['thrs'], logger='silent', use_legacy_coordinate=CONVENTIONS[c],
                         device=dev)
    assert np.array_equal(got, z[f'recalls_{c}'])


# ------------------------------------------------------------------------------------------------ the detector
def test_rpn_detector_is_the_first_stage_of_the_faster_rcnn(dev):
    from oadg_amd import Config, build_detector
    from oadg_amd.apis import set_random_seed
    from oadg_amd.pipelines import DevicePipeline, SyntheticCityscapes
    set_random_seed(0)
    models = []
    for path in ('oadg/faster_rcnn_r50_fpn_1x_cityscapes.py', 'rpn/rpn_r50_fpn_1x_cityscapes.py'):
        cfg = Config.fromfile(os.path.join(ROOT, 'configs', path))
        m = build_detector(cfg.model, test_cfg=cfg.get('test_cfg'))
        m.init_weights(allow_missing_pretrained=True)
        models.append(m)
    det, rpn = models
    rep = rpn.load_state_dict(det.state_dict(), strict=False)                  # a Faster R-CNN checkpoint loads into it
    assert not rep.missing_keys and rep.unexpected_keys and all(k.startswith('roi_head.') for k in rep.unexpected_keys)
    det, rpn = (m.to(dev).to(memory_format=torch.channels_last).eval() for m in (det, rpn))
    norm = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
    inner = [dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **norm),
             dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']), dict(type='Collect', keys=['img'])]
    pipe = DevicePipeline([dict(type='LoadImageFromFile'),
                           dict(type='MultiScaleFlipAug', img_scale=(640, 320), flip=False, transforms=inner)],
                          dtype=torch.float32)
    ds = SyntheticCityscapes(img_shape=(256, 512), num_boxes=6, box_size=(24, 160), device=dev)
    imgs, _, _ = ds.batch([0, 1])
    data = pipe.test_batch(imgs)
    img, metas = data['img'][0], data['img_metas'][0]
    assert all(float(m['scale_factor'][0]) == 1.25 for m in metas)
    with torch.no_grad():
        want = det.rpn_head.simple_test_rpn(det.extract_feat(img), metas)
        want = [torch.cat([p[:, :4] / p.new_tensor(m['scale_factor']), p[:, 4:]], dim=1).cpu().numpy()
                for p, m in zip(want, metas)]
        got = rpn(return_loss=False, rescale=True, **data)
        plain = rpn.simple_test(img, metas)
    assert len(got) == 2 and all(isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape[1] == 5 for g in got)
    assert all(len(g) > 0 and g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert all(np.array_equal(p[:, :4] / 1.25, g[:, :4]) for p, g in zip(plain, got))
    # test-time augmentation: the merged proposals of aug_test_rpn, in the original frame with rescale, else in imgs[0]'s
    aug = DevicePipeline([dict(type='LoadImageFromFile'),
                          dict(type='MultiScaleFlipAug', img_scale=[(640, 320), (512, 256)], flip=True, transforms=inner)],
                         dtype=torch.float32).test_batch(imgs[:1])
    assert len(aug['img']) == 4 and float(aug['img_metas'][0][0]['scale_factor'][0]) == 1.25
    with torch.no_grad():
        merged = rpn.rpn_head.aug_test_rpn([rpn.extract_feat(i) for i in aug['img']], aug['img_metas'])
        res = rpn(return_loss=False, rescale=True, **aug)
        res0 = rpn.aug_test(aug['img'], aug['img_metas'], rescale=False)
    assert len(res) == 1 and len(res[0]) > 0 and res[0].tobytes() == merged[0].cpu().numpy().tobytes()
    assert np.array_equal(res0[0][:, :4], res[0][:, :4] * np.float32(1.25)) and np.array_equal(res0[0][:, 4], res[0][:, 4])
    # a result draws as twenty proposals of one class
    pic = rpn.show_result(imgs[0].cpu().numpy(), got[0])
    assert pic.shape == (256, 512, 3) and (pic != imgs[0].cpu().numpy()).any()
    # and scores through proposal_evaluate on the device as on the host
    ds.length = 2
    assert E.proposal_evaluate(ds, got, 'proposal_fast', logger='silent', device=dev) == \
        E.proposal_evaluate(ds, got, 'proposal_fast', logger='silent', device=None)


# ------------------------------------------------------------------------------------------------ the command lines
SMALL_PIPELINE = (
    "img_norm_cfg = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)\n"
    "test_pipeline = [dict(type='LoadImageFromFile'), dict(type='MultiScaleFlipAug', img_scale=({w}, {h}), flip=False,\n"
    "    transforms=[dict(type='Resize', keep_ratio=True), dict(type='RandomFlip'), dict(type='Normalize', **img_norm_cfg),\n"
    "                dict(type='Pad', size_divisor=32), dict(type='ImageToTensor', keys=['img']),\n"
    "                dict(type='Collect', keys=['img'])])]\n")


def test_test_cli_proposal_fast_on_a_synthetic_split(tmp_path):
    from oadg_amd.pipelines import SyntheticCityscapes
    cfg = tmp_path / 'rpn_tiny.py'
    cfg.write_text(f"_base_ = ['{ROOT}/configs/rpn/rpn_r50_fpn_1x_cityscapes.py']\n" + SMALL_PIPELINE.format(w=512, h=256) +
                   "data = dict(test=dict(type='SyntheticCityscapes', img_shape=(256, 512), num_boxes=6, num_classes=8, length=4,\n"
                   "                      box_size=(24, 160), pipeline=test_pipeline))\n")
    wd, out = tmp_path / 'eval', tmp_path / 'r.pkl'
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), str(cfg), 'none', '--eval', 'proposal_fast',
                        '--work-dir', str(wd), '--out', str(out), '--eval-options', 'proposal_nums=(10, 100, 1000)'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out, 'rb') as f:
        results = pickle.load(f)
    assert len(results) == 4 and all(isinstance(p, np.ndarray) and p.shape[1] == 5 for p in results)
    assert '4 images in ' in r.stdout and f'{sum(len(p) for p in results)} proposals' in r.stdout
    ds = SyntheticCityscapes(img_shape=(256, 512), num_boxes=6, num_classes=8, length=4, box_size=(24, 160), seed=12345,
                             device='cpu')
    want = E.eval_recalls([ds.boxes(i)[0] for i in range(4)], results, [10, 100, 1000], E.IOU_THRS, logger='silent').mean(axis=1)
    line, = [ln for ln in r.stdout.splitlines() if ln.startswith('proposal_fast: ')]
    printed = ast.literal_eval(line[len('proposal_fast: '):])
    assert list(printed) == ['AR@10', 'AR@100', 'AR@1000'] and list(printed.values()) == want.tolist()
    assert json.load(open(wd / 'eval.json')) == {'proposal_fast': printed}


def test_test_cli_recall_walks_two_tiny_voc_trees(tmp_path):
    from oadg_amd.datasets import SdgodDataset
    from test_sdgod_dataset import _obj, write_voc
    trees = []
    for k, names in enumerate((('a', 'b', 'c'), ('d', 'e', 'f'))):
        tree = {n: (96, 160, True, [_obj('car', (10 + 5 * k, 20, 90, 70)), _obj('person', (100, 10, 140, 80), 1)]) for n in names}
        trees.append(write_voc(str(tmp_path / f'dom{k}'), tree))
    cfg = tmp_path / 'rpn_dwd_tiny.py'
    cfg.write_text(f"_base_ = ['{ROOT}/configs/rpn/rpn_r101_dc5_1x_dwd_sdgod_test.py']\n" + SMALL_PIPELINE.format(w=320, h=192) +
                   "data = dict(test=[" + ', '.join(
                       f"dict(type='SdgodDataset', ann_file=['{t}ImageSets/Main/train.txt'], img_prefix=['{t}'], "
                       f"pipeline=test_pipeline)" for t in trees) + "])\n")
    wd = tmp_path / 'eval'
    env = dict(os.environ, OADG_ALLOW_RANDOM_INIT='1')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), str(cfg), 'none', '--eval', 'recall',
                        '--max-samples', '2', '--work-dir', str(wd), '--out', str(tmp_path / 'r.pkl'),
                        '--eval-options', 'iou_thr=[0.5, 0.75]', 'proposal_nums=(10, 1000)'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    dicts = [ast.literal_eval(ln[len('recall: '):]) for ln in r.stdout.splitlines() if ln.startswith("recall: {'recall@10@0.5'")]
    assert len(dicts) == 2, r.stdout[-2000:]
    keys = ['recall@10@0.5', 'recall@10@0.75', 'recall@1000@0.5', 'recall@1000@0.75', 'AR@10', 'AR@1000']
    for i, (d, t) in enumerate(zip(dicts, trees)):
        with open(tmp_path / f'r_{i}.pkl', 'rb') as f:
            results = pickle.load(f)
        assert len(results) == 2 and all(p.shape[1] == 5 for p in results)
        ds = SdgodDataset(ann_file=t + 'ImageSets/Main/train.txt', img_prefix=t, device='cpu', test_mode=True)
        boxes = [ds.get_ann_info(j)['bboxes'] for j in range(2)]              # the two TESTED images, legacy extents
        rec = E.eval_recalls(boxes, results, [10, 1000], [0.5, 0.75], logger='silent', use_legacy_coordinate=True)
        assert list(d) == keys and [d[k] for k in keys] == rec.reshape(-1).tolist() + rec.mean(axis=1).tolist()
    summary, = [ln for ln in r.stdout.splitlines() if ln.startswith('AR@1000 per split: ')]
    want = [d['AR@1000'] for d in dicts]
    assert summary == 'AR@1000 per split: ' + ' '.join(f'{v:.3f}' for v in want) + f'  mean {sum(want) / 2:.3f}'
    assert json.load(open(wd / 'eval.json')) == {'recall': dicts} and not (tmp_path / 'r.pkl').exists()
    assert all(f'split {i}: 2 images in ' in r.stdout for i in range(2))
    # a list of splits with a detection metric is the other tool's: refused by name, before any image is tested
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'test.py'), str(cfg), 'none', '--eval', 'mAP'],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and 'tools/test_dwd.py' in r.stderr and 'images in' not in r.stdout
