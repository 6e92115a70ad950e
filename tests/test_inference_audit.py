"""Elementwise fp64 audit of every launch of bf16 test-time inference (tools/test.py, tools/analysis_tools/test_robustness.py:
build_model, DevicePipeline.test_batch, ``model(return_loss=False, rescale=True)`` under no_grad and bf16 autocast), plus
CPU self-tests showing that the new checks of tests/infer_audit.py reject subtly wrong results.

GPU tests (``-m gpu``): two consecutive forwards of each workload under the three auditors (tests/conv_audit.py,
tests/head_audit.py, tests/infer_audit.py) - the first cold (the weight preparation launches), the second served from the
prepared-weight bank.  Each asserts that no audited value exceeds its bound, that the two forwards return bit-identical
results, that the carved-out borderline elements stay under their caps and that the audited kernel instantiations equal
the lists written here (a test-time launch routed to another kernel, or to a library call, fails the test).
"""
import os

import numpy as np
import pytest
import torch

import conv_audit as CA
import head_audit as HA
import infer_audit as IA
from audit_workload import DC5_CFG, R50_CFG, audited_inference, tta_pipeline
from test_head_audit import BORDERLINE_CAP as ROI_BORDERLINE_CAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------- CPU self-tests of the checks
def _proposals(seed=0, n_img=2, k=300):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand((n_img, k, 2), generator=g) * 500
    wh = 4 + torch.rand((n_img, k, 2), generator=g) * 100
    s = torch.rand((n_img, k, 1), generator=g)
    return list(torch.cat([xy, xy + wh, s], 2).unbind(0))


def test_proposal_check_accepts_equal_lists_and_rejects_one_ulp():
    ref = _proposals()
    A = IA.Auditor()
    A._check_proposals(['oadg_rpn_topk', 'oadg_rpn_decode', 'oadg_rpn_order', 'oadg_rpn_gather'], [p.clone() for p in ref], ref)
    assert not A.failures and {'rpn_decode_kernel', 'sel_sort_kernel'} <= A.kernels
    bad = [p.clone() for p in ref]
    bad[1][17, 2] = torch.nextafter(bad[1][17, 2], torch.tensor(float('inf')))        # one coordinate moved by one ulp
    A._check_proposals(['oadg_rpn_gather'], bad, ref)
    assert len(A.failures) == 1


def _sorted_boxes(seed=1, n_img=2, M=700):
    """class-offset boxes in descending-score order, clustered so that NMS suppresses many"""
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((n_img, M // 10, 1, 2), generator=g) * 400
    xy = (c + torch.randn((n_img, M // 10, 10, 2), generator=g) * 6).reshape(n_img, M, 2)
    wh = 20 + torch.rand((n_img, M, 2), generator=g) * 30
    return torch.cat([xy, xy + wh], 2).float()


@pytest.mark.parametrize('plant', [None, 'keeps a suppressed box', 'drops a kept box', 'count'])
def test_nms_check_against_the_oracle(plant):
    from oracle import nms as ONMS
    boxes = _sorted_boxes()
    counts = torch.tensor([700, 650], dtype=torch.int32)
    keep = torch.zeros((2, 700), dtype=torch.int32)
    cnt = torch.zeros(2, dtype=torch.int32)
    for i in range(2):
        k = ONMS.nms_sorted(boxes[i, :int(counts[i])].numpy(), 0.7, max_keep=1000)
        keep[i, :len(k)] = torch.as_tensor(k, dtype=torch.int32)
        cnt[i] = len(k)
    kept = set(keep[1, :int(cnt[1])].tolist())
    assert len(kept) < 600                                  # (the clusters do suppress)
    if plant == 'keeps a suppressed box':
        extra = min(set(range(650)) - kept)
        k = sorted(kept | {extra})
        keep[1, :len(k)] = torch.as_tensor(k, dtype=torch.int32)
        cnt[1] = len(k)
    elif plant == 'drops a kept box':
        k = sorted(kept)[:5] + sorted(kept)[6:]
        keep[1, :len(k)] = torch.as_tensor(k, dtype=torch.int32)
        keep[1, len(k)] = 0
        cnt[1] = len(k)
    elif plant == 'count':
        cnt[0] -= 1
    A = IA.Auditor()
    A._check_nms(boxes, counts, 0.7, 1000, keep, cnt)
    assert A.kernels == {'nms_mask_kernel', 'nms_scan_kernel<3, 2>'}
    assert bool(A.failures) == (plant is not None), A.failures


# post-processing: a RoI head's outputs with boxes that leave the image (the clamp matters) and a non-unit scale factor
_IMG_SHAPE, _SF = (400, 800, 3), np.array([0.8, 0.75, 0.8, 0.75], np.float32)
_MEANS, _STDS = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)


def _head_outputs(seed=2, n=400, C=8):
    g = torch.Generator().manual_seed(seed)
    c = torch.rand((n, 2), generator=g) * torch.tensor([850.0, 450.0]) - 25
    wh = 8 + torch.rand((n, 2), generator=g) * 150
    rois = torch.cat([torch.zeros(n, 1), c - wh / 2, c + wh / 2], 1)
    cls = (torch.randn((n, C + 1), generator=g) * 1.5).to(torch.bfloat16).float()
    reg = (torch.randn((n, 4 * C), generator=g) * 0.8).to(torch.bfloat16).float()
    return rois, cls, reg


def _product_postproc(rois, cls, reg, img_shape=_IMG_SHAPE, sf=_SF, rescale=True, thr=0.05, iou=0.5, max_num=100):
    """ConvFCBBoxHead.get_bboxes + bbox2result on the host (oracle NMS): what the detector returns for these outputs"""
    from oracle.backend import oracle_ops
    from oadg_amd.core import bbox2result, multiclass_nms
    from oadg_amd.core.bbox import DeltaXYWHBBoxCoder
    coder = DeltaXYWHBBoxCoder(target_means=_MEANS, target_stds=_STDS)
    scores = torch.softmax(cls, -1)
    b = coder.decode(rois[:, 1:], reg, max_shape=img_shape)
    if rescale:
        b = (b.view(b.size(0), -1, 4) / torch.as_tensor(sf)).view(b.size(0), -1)
    with oracle_ops():
        dets, labels = multiclass_nms(b, scores, thr, dict(type='nms', iou_threshold=iou), max_num)
    return bbox2result(dets, labels, cls.shape[1] - 1)


def _compare(result, rois, cls, reg, thr=0.05, max_num=100):
    b, bt, s, st = IA.decode_expect(rois, cls, reg, _IMG_SHAPE, _SF, _MEANS, _STDS)
    return IA.compare_detections(result, b, bt, s, st, thr, 0.5, max_num)


def test_postproc_reference_accepts_the_product_path():
    rois, cls, reg = _head_outputs()
    res = _product_postproc(rois, cls, reg)
    assert sum(len(r) for r in res) == 100                  # (max_per_img is reached: the cut is exercised)
    fails, border, total = _compare(res, rois, cls, reg)
    assert not fails and total > 500 and IA.within_cap(border, total), (fails[:3], border, total)
    res = _product_postproc(rois, cls, reg, max_num=-1)     # every survivor of the NMS
    fails, border, total = _compare(res, rois, cls, reg, max_num=-1)
    assert not fails and sum(len(r) for r in res) > 150, fails[:3]


def test_postproc_rejects_an_unrescaled_detection():
    rois, cls, reg = _head_outputs()
    fails, _, _ = _compare(_product_postproc(rois, cls, reg, rescale=False), rois, cls, reg)
    assert fails and fails[0][0] == 'detection matches no candidate of its class'


def test_postproc_rejects_a_detection_under_the_neighbouring_class():
    rois, cls, reg = _head_outputs()
    res = _product_postproc(rois, cls, reg)
    c = next(i for i in range(7) if len(res[i]))
    res[c + 1] = np.concatenate([res[c][:1], res[c + 1]])
    res[c] = res[c][1:]
    fails, _, _ = _compare(res, rois, cls, reg)
    assert fails and fails[0][0] == 'detection matches no candidate of its class'


@pytest.mark.parametrize('shape', [(399, 800, 3), (800, 400, 3)])
def test_postproc_rejects_a_wrong_img_shape_clamp(shape):
    rois, cls, reg = _head_outputs()
    fails, _, _ = _compare(_product_postproc(rois, cls, reg, img_shape=shape), rois, cls, reg)
    assert fails


def test_postproc_rejects_a_dropped_detection_and_caps_the_borderline_count():
    rois, cls, reg = _head_outputs()
    res = _product_postproc(rois, cls, reg)
    c = next(i for i in range(8) if len(res[i]))
    bad = list(res)
    bad[c] = res[c][1:]                                     # the best detection of a class lost
    fails, _, _ = _compare(bad, rois, cls, reg)
    assert fails and fails[0][0] == 'kept set differs from the fp64 selection'
    # candidates whose fp64 score lies within fp32 rounding above the threshold: fp32 drops them, fp64 keeps them -
    # borderline, not failures, and over the cap when they are many
    from oracle.backend import oracle_ops
    from oadg_amd.core import bbox2result, multiclass_nms
    b, bt, s, st = IA.decode_expect(rois, cls, reg, _IMG_SHAPE, _SF, _MEANS, _STDS)
    s[torch.arange(0, 400, 5), 0] = 0.05 + 1e-12
    with oracle_ops():
        dets, labels = multiclass_nms(b.float().view(400, -1), s.float(), 0.05, dict(type='nms', iou_threshold=0.5), -1)
    fails, border, total = IA.compare_detections(bbox2result(dets, labels, 8), b, bt, s, st, 0.05, 0.5, -1)
    assert not fails and border >= 10, (fails[:3], border)
    assert not IA.within_cap(border, total) and IA.within_cap(0, total)


def _one_class(boxes, scores):
    """fp64 candidates of one class (boxes [n, 1, 4], scores [n, 2] with a background column) and tight tolerances"""
    b = torch.tensor(boxes, dtype=torch.float64).view(-1, 1, 4)
    s = torch.tensor([[v, 1.0 - v] for v in scores], dtype=torch.float64)
    return b, torch.full_like(b, 1e-4), s, torch.full_like(s, 1e-6)


def _dets(b, s, rows):
    return [np.array([b[i, 0].tolist() + [float(s[i, 0])] for i in rows], np.float32).reshape(-1, 5)]


@pytest.mark.parametrize('far', [False, True])
def test_postproc_borderline_iou_its_suppression_cascade_and_the_max_per_img_tail(far):
    """B overlaps A at IoU 0.5 + 1e-12: fp64 suppresses it, an fp32 NMS may keep it - borderline.  Kept, B suppresses D
    (IoU 0.8 with B, far from A): the cascade of that borderline decision.  With ``far``, D does not overlap B and instead
    is pushed past max_per_img = 3 by B: the tail of the cut.  A detection dropped for no such reason still fails."""
    x = 10.0 / 3.0 - 1e-11                                 # IoU([0,0,10,10], [x,0,x+10,10]) just above 0.5
    d = [30.0, 0.0, 40.0, 10.0] if far else [x + 2.0, 0.0, x + 12.0, 10.0]
    boxes = [[0, 0, 10, 10], [x, 0, x + 10, 10], [100, 100, 120, 120], d, [200, 200, 230, 230]]
    b, bt, s, st = _one_class(boxes, [0.9, 0.8, 0.75, 0.7, 0.6])       # A, B, E, D, F
    ref = IA.multiclass_expect(b, s, 0.05, 0.5, 3).tolist()
    assert ref == [0, 2, 3]                                # A, E, D: B suppressed by A in fp64
    fails, border, total = IA.compare_detections(_dets(b, s, [0, 1, 2]), b, bt, s, st, 0.05, 0.5, 3)
    assert not fails and border == 2 and total == 5, (fails, border)
    # the same sets without a borderline root: B clearly overlapping A (IoU 0.6) - a failure
    boxes[1] = [2.5, 0, 12.5, 10]
    b, bt, s, st = _one_class(boxes, [0.9, 0.8, 0.75, 0.7, 0.6])
    fails, _, _ = IA.compare_detections(_dets(b, s, [0, 1, 2]), b, bt, s, st, 0.05, 0.5, 3)
    assert fails and fails[0][0] == 'kept set differs from the fp64 selection'


def test_postproc_tail_rule_moves_the_cut_by_the_explained_differences_only():
    """a borderline root (B in class 0) pushes one detection past max_per_img = 4 - the last of the fp64 selection in score
    order, here R of class 1.  A suppressed duplicate kept instead (Q of P) displaces a detection before the cut, E, which
    is not excused"""
    x = 10.0 / 3.0 - 1e-11
    b = torch.tensor([[[0, 0, 10, 10], [500, 500, 510, 510]], [[x, 0, x + 10, 10], [500, 500, 510, 510]],
                      [[100, 100, 120, 120], [600, 600, 610, 610]], [[300, 300, 320, 320], [200, 0, 210, 10]]],
                     dtype=torch.float64)
    # class 0: A .9, B .8 (borderline vs A), E .7; class 1: P .85 (row 0), Q .6 (row 1, duplicate of P), R .5
    s = torch.tensor([[0.9, 0.85, 0.0], [0.8, 0.6, 0.0], [0.7, 0.04, 0.0], [0.04, 0.5, 0.0]], dtype=torch.float64)
    bt, st = torch.full_like(b, 1e-4), torch.full_like(s, 1e-6)
    ref = IA.multiclass_expect(b, s, 0.05, 0.5, 4).tolist()
    assert ref == [0, 1, 4, 7]                             # A, P, E, R (B suppressed by A, Q by P)
    ok = [np.array([[0, 0, 10, 10, 0.9], [x, 0, x + 10, 10, 0.8], [100, 100, 120, 120, 0.7]], np.float32),
          np.array([[500, 500, 510, 510, 0.85]], np.float32)]
    fails, border, _ = IA.compare_detections(ok, b, bt, s, st, 0.05, 0.5, 4)
    assert not fails and border == 2, fails                # B (root) and R (past the cut)
    bad = [ok[0][:2], np.array([[500, 500, 510, 510, 0.85], [500, 500, 510, 510, 0.6]], np.float32)]
    fails, _, _ = IA.compare_detections(bad, b, bt, s, st, 0.05, 0.5, 4)
    assert fails and fails[0][0] == 'kept set differs from the fp64 selection'
    assert (2, 0) in {f[2:4] for f in fails}, fails          # E dropped


def test_postproc_selection_matches_the_oracle_on_the_reference_fixture(golden_dir):
    """multiclass_expect on tests/golden/postproc_reference.npz (multiclass_nms + bbox2result of the reference)"""
    from inputs import postproc_inputs
    from test_inference_path import CASES
    g = np.load(os.path.join(golden_dir, 'postproc_reference.npz'))
    for seed, n, C, per_class, thr, iou, max_num in CASES:
        boxes, scores = postproc_inputs(seed, n, C, per_class)
        b = torch.as_tensor(boxes, dtype=torch.float64).view(n, -1, 4).expand(n, C, 4)
        s = torch.as_tensor(scores, dtype=torch.float64)
        keep = IA.multiclass_expect(b, s, thr, iou, max_num)
        dets = torch.cat([b.reshape(-1, 4)[keep], s[:, :C].reshape(-1)[keep, None]], 1).to(torch.float32).numpy()
        for c in range(C):
            assert np.array_equal(dets[(keep % C).numpy() == c], g[f's{seed}_res{c}']), (seed, c)
        # and the host comparison accepts the reference's own arrays with no borderline detection
        z = torch.zeros_like(b) + IA.ALPHA
        fails, border, _ = IA.compare_detections([g[f's{seed}_res{c}'] for c in range(C)], b, z, s, torch.zeros_like(s) + IA.ALPHA,
                                                 thr, iou, max_num)
        assert not fails and border == 0, (seed, fails[:3])


def test_linear_reference_rejects_an_unpermuted_weight():
    g = torch.Generator().manual_seed(4)
    O, C, P, K = 64, 32, 9, 50
    x = torch.randn((K, P * C), generator=g).to(torch.bfloat16)
    w = torch.randn((O, C * P), generator=g) * 0.05
    b = torch.randn(O, generator=g) * 0.1
    wp = w.view(O, C, P).permute(0, 2, 1).reshape(O, P * C)         # the (p, c) column order RoIAlign's output has
    r, bd = IA.linear_expect(x, wp, b, torch.bfloat16)
    good = (x.double() @ wp.to(torch.bfloat16).double().t() + b.to(torch.bfloat16).double()).to(torch.bfloat16)
    assert CA.ratio(good, r, bd)[0] <= 1.0
    bad = (x.double() @ w.to(torch.bfloat16).double().t() + b.to(torch.bfloat16).double()).to(torch.bfloat16)
    assert CA.ratio(bad, r, bd)[0] > 1.0


# ------------------------------------------------------------------------------------------------- GPU audited inference
# the kernel instantiations (and library calls) each forward of a workload launches - the cold one and the warm one alike:
# the bank serves the trainable layers' prepared weights on the second forward (rows "(served from the bank)"), and the
# weights it does not hold (the frozen stem, the RPN head's zero-padded [rpn_cls; rpn_reg] built each forward) are prepared
# by prep_weights_kernel on every forward.  Launched at test time and by no audited training step: conv_pw_stream_kernel<512,
# false, false, false> (layer4's 512 -> 2048 conv3 without ReLU bits); the RPN head's padded 1x1 convolution takes
# instantiations listed there.  The proposal and NMS kernels run in every training step too (its RoI proposals), audited
# here first.
# No test-time convolution reaches F.conv2d: a 'F.conv2d (library) C->K RxS' row in the set fails the test.
# (the tile width of conv_igemm_kernel by conv_launch's rule, conv_audit.tile_width: 64-wide tiles on the small maps;
#  the two instantiations below run in every workload but the two-image R101-DC5 one)
_EXCEPT_DC5_B2 = {'conv_igemm_kernel<128, false, 2, false>', 'conv_igemm_kernel<64, true, 1, true>'}
_COMMON = {
    'F.linear (library GEMM)', 'bias_relu_maxpool_kernel', 'bottleneck_frozen_first_kernel',
    'bottleneck_frozen_kernel', 'conv_igemm_kernel<128, false, 1, false>', 'conv_igemm_kernel<128, false, 1, true>',
    'conv_igemm_kernel<128, true, 1, true>', 'conv_igemm_kernel<64, false, 1, false>',
    'conv_igemm_kernel<64, false, 1, true>', 'conv_igemm_kernel<64, false, 2, false>', 'fc_weight_permute_kernel',
    'nms_mask_kernel', 'nms_scan_kernel<3, 2>', 'prep_weights_kernel', 'roi_align_fwd_rows_kernel<unsigned short>',
    'rpn_decode_kernel', 'rpn_gather_kernel', 'rpn_order_kernel', 'sel_count_kernel2', 'sel_refine_kernel<1>',
    'sel_refine_kernel<2>', 'sel_scatter_kernel', 'sel_score_kernel', 'sel_sort_kernel', 'stem_conv7x7s2_kernel',
}
EXPECTED = {
    'r50_fpn': _COMMON | _EXCEPT_DC5_B2 | {'conv_igemm256_kernel<false, 2>', 'conv_pw_stream_kernel<256, true, false, false>',
                                           'conv_pw_stream_kernel<512, false, false, false>',
                                           'conv_pw_stream_kernel<512, true, false, false>', 'fpn_topdown_fwd_kernel'},
    'r101_dc5_b1': _COMMON | _EXCEPT_DC5_B2,
    # (two images: M = N Ho Wo of the 512 -> 2048 conv3 layers of layer4 reaches the streaming kernel, and no launch is
    #  left on the two-stage 128-wide tile or on the 64-wide pointwise tile with a residual)
    'r101_dc5_b2': _COMMON | {'conv_pw_stream_kernel<512, true, false, false>'},
}
# the ragged 800 x 1600 augmentations take no instantiation the 1024 x 2048 ones do not
EXPECTED['r50_fpn_aug'] = EXPECTED['r50_fpn']
WRAPPERS = {'conv_forward', '_PrepWeights.forward', 'frozen_bottleneck', 'stem_conv', 'bias_relu_maxpool',
            '_RoIAlignFPN.forward', '_FcWeightPermute.forward', 'nms_sorted_batched', 'RPNHead.get_bboxes', 'F.linear'}


def _infer(dev, monkeypatch, tmp_path, cfg, batch, H, W, key, pipeline=None):
    auditors = (CA.Auditor(), HA.Auditor(), IA.Auditor())
    per = []

    def install(mp, model):
        auditors[0].install(mp)
        auditors[1].install(mp, model, sgd=False)
        auditors[2].install(mp, model)

    def on_forward(k, model, res, data):
        auditors[2].check_results(model, k, res)
        per.append(set().union(*(a.kernels for a in auditors)))
        for a in auditors:
            a.kernels.clear()
    outs, model, walls = audited_inference(dev, monkeypatch, tmp_path, cfg, batch, H, W, install, pipeline, on_forward)
    for a, fam in zip(auditors, ('conv', 'head', 'inference')):
        a.print_table('%s %s (forwards %.1f s, %.1f s)' % (key, fam, *walls))
        print('worst err / bound: %.4f' % a.worst())
    print('cold instantiations:', sorted(per[0]))
    print('warm instantiations:', sorted(per[1]))
    print('detections per image:', auditors[2].info.get('detections'))
    fails = [f for a in auditors for f in a.failures]
    assert not fails, fails[:10]
    hit = set().union(*(a.wrappers for a in auditors))
    assert not WRAPPERS - hit, WRAPPERS - hit
    assert len(outs[0]) == len(outs[1]) == batch
    for r0, r1 in zip(*outs):
        assert all(np.array_equal(a, b) for a, b in zip(r0, r1)), 'the warm forward differs from the cold one'
    assert sum(len(c) for r in outs[0] for c in r) > 0
    for a in auditors[1:]:
        for fam, (carved, total) in a.borderline.items():
            cap = IA.within_cap(carved, total) if fam == 'post-processing' else carved <= ROI_BORDERLINE_CAP * max(total, 1)
            assert cap, (fam, carved, total)
    exp = EXPECTED[key]
    for k in range(2):
        assert per[k] == exp, (k, sorted(per[k] - exp), sorted(exp - per[k]))
    return auditors


@pytest.mark.gpu
def test_inference_audit_config1_r50_fpn(dev, monkeypatch, tmp_path):
    """configs[1] as tools/test.py runs it: R50-FPN OA-DG Cityscapes, batch 1 at 1024 x 2048, bf16"""
    _infer(dev, monkeypatch, tmp_path, R50_CFG, 1, 1024, 2048, 'r50_fpn')


@pytest.mark.gpu
@pytest.mark.parametrize('batch', [1, 2])
def test_inference_audit_config3_r101_dc5(dev, monkeypatch, tmp_path, batch):
    """configs[3]: R101-DC5 on 720 x 1280 images (padded to 736 x 1280), batch 1 and the config's samples_per_gpu (2);
    one RPN level with nms_pre 6000"""
    _infer(dev, monkeypatch, tmp_path, DC5_CFG, batch, 720, 1280, 'r101_dc5_b%d' % batch, tta_pipeline((1280, 720)))


@pytest.mark.gpu
def test_inference_audit_aug_test_two_scales_and_flip(dev, monkeypatch, tmp_path):
    """aug_test in bf16: MultiScaleFlipAug(img_scale=[(2048, 800), (2048, 1024)], flip=True) on a 1024 x 2048 image - the
    ragged 800 x 1600 pyramid, resize_bilinear_u8, flip_u8 and the merge of four augmentations"""
    _infer(dev, monkeypatch, tmp_path, R50_CFG, 1, 1024, 2048, 'r50_fpn_aug',
           tta_pipeline([(2048, 800), (2048, 1024)], flip=True))
