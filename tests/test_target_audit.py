"""The assignment / sampling / target auditor (tests/target_audit.py).

CPU: every reference function against tests/golden/core_reference.npz (the reference's own outputs) bit for bit - the
encoded deltas, CPU float32 there, within the GAMMA_T bound of the float64 recomputation -, one planted error per test that
the checker must reject, and the closure over the C-ABI call sites of oa-dg_amd/: every ``.oadg_*`` symbol called anywhere
belongs to exactly one named set, so a new call fails here until someone says which suite checks it.

GPU: the three audited steps of tests/test_head_audit.py (same arguments) and a fourth with the RoI sampler on the host,
under target_audit.Auditor; then the wrapped entry points called directly on constructed operands (stress launches),
judged by the same reference functions.
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import conv_audit as CA  # noqa: E402
import f32_audit as FA  # noqa: E402
import head_audit as HA  # noqa: E402
import infer_audit as IA  # noqa: E402
import target_audit as TA  # noqa: E402
from audit_workload import DC5_CFG, R50_CFG, ROOT, audited_step  # noqa: E402
from test_core_reference import _inputs  # noqa: E402


@pytest.fixture(scope='module')
def g(golden_dir):
    return np.load(os.path.join(golden_dir, 'core_reference.npz'))


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs the MI355X')
    return torch.device('cuda:0')


ASSIGN_CFGS = [dict(pos=0.7, neg_lo=0.0, neg_hi=0.3, min_pos=0.3, match_low_quality=True),
               dict(pos=0.5, neg_lo=0.0, neg_hi=0.5, min_pos=0.5, match_low_quality=False)]
SAMPLE_CFGS = [dict(num=64, pos_fraction=0.5, neg_pos_ub=-1, add_gt=False),
               dict(num=128, pos_fraction=0.25, neg_pos_ub=-1, add_gt=True)]


# ----------------------------------------------------------------------------------------------------- golden ties (CPU)
@pytest.mark.parametrize('seed', range(3))
def test_iou_assign_sample_references_match_the_golden(g, seed):
    props, gts, labels = _inputs(seed)
    assert np.array_equal(TA.iou_expect(gts, props), g[f'iou{seed}'])
    for c, (acfg, scfg) in enumerate(zip(ASSIGN_CFGS, SAMPLE_CFGS)):
        gi, mo, lab, (n_pos, n_neg) = TA.assign_expect(props, None, gts, labels, **acfg)
        assert np.array_equal(gi, g[f'assign{seed}_{c}_gt_inds'])
        assert np.array_equal(mo, g[f'assign{seed}_{c}_max_overlaps'])
        assert np.array_equal(lab, g[f'assign{seed}_{c}_labels'])
        assert (n_pos, n_neg) == (int((gi > 0).sum()), int((gi == 0).sum()))
        if scfg['add_gt']:
            _, gi, lab, mo, flags = TA.add_gt_expect(props, gts, labels, gi, mo, lab)
            assert flags[:len(gts)].all() and not flags[len(gts):].any()
        torch.manual_seed(seed)
        (s,), state = TA.sample_expect([gi], scfg['num'], scfg['pos_fraction'], scfg['neg_pos_ub'], torch.get_rng_state())
        assert np.array_equal(s[0], g[f'sample{seed}_{c}_pos'])
        assert np.array_equal(s[1], g[f'sample{seed}_{c}_neg'])
        after = torch.Generator()
        after.set_state(state)
        assert np.array_equal(torch.rand(1, generator=after).numpy(), g[f'sample{seed}_{c}_rng'])


@pytest.mark.parametrize('seed', range(3))
def test_delta_reference_matches_the_golden_within_the_bound(g, seed):
    """the golden deltas are the reference's CPU float32 results: the float64 recomputation meets them within GAMMA_T S +
    ALPHA, the three zero-size rows (3: width, 5: height, 7: both) included; the row-wise rule misses row 3"""
    p, gt, d = g[f'delta{seed}_p'], g[f'delta{seed}_g'], g[f'delta{seed}_d']
    means, stds = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)
    r, S, one_sided = TA.delta_expect(p, gt, means, stds)
    assert one_sided == 2 and np.isfinite(r).all()
    worst = TA.delta_ratio(d, r, S)
    print('golden deltas, seed %d: worst err / bound %.4f' % (seed, worst))
    assert worst <= 1.0
    assert TA.delta_ratio(d[[3, 5, 7]], r[[3, 5, 7]], S[[3, 5, 7]]) <= 1.0
    rw, Sw, _ = TA.delta_expect(p, gt, means, stds, rule='rowwise')
    assert TA.delta_ratio(d[3], rw[3], Sw[3]) > 1.0                      # KNOWN_DEVIATION_ENCODE_DELTA is visible here
    keep = np.ones(len(p), bool)
    keep[3] = False
    assert TA.delta_ratio(d[keep], rw[keep], Sw[keep]) <= 1.0
    # the tensor path of core/bbox.py is the golden rule (bit for bit: tests/test_core_reference.py)
    from oadg_amd.core.bbox import bbox2delta
    assert TA.delta_ratio(bbox2delta(torch.from_numpy(p), torch.from_numpy(gt), means, stds), r, S) <= 1.0


def test_delta_reference_raises_where_the_reference_does():
    p = np.array([[0, 0, 0, 10], [5, 5, 9, 9]], np.float32)            # one zero-width row, no zero-height row
    with pytest.raises(ValueError):
        TA.delta_expect(p, p, (0,) * 4, (1,) * 4)
    assert TA.delta_expect(p, p, (0,) * 4, (1,) * 4, rule='rowwise')[2] == 1


@pytest.mark.parametrize('seed', range(4))
def test_random_bboxes_reference_matches_the_golden(g, seed):
    np.random.seed(seed)
    state = np.random.get_state()
    np.random.seed(99)
    outside = np.random.get_state()
    b, after = TA.random_bboxes_expect(state, (256, 512), 10, g[f'rand_gts{seed}'], scales=(0.01, 0.3),
                                       ratios=(0.3, 1 / 0.3), iou_max=0.7, iou_min=0.0)
    assert TA.np_state_same(np.random.get_state(), outside)            # the caller's stream is left alone
    assert np.array_equal(np.asarray(b), g[f'rand_boxes{seed}'])
    np.random.set_state(after)
    assert np.random.uniform() == float(g[f'rand_rng{seed}'][0])


# ------------------------------------------------------------------------------------------------- planted errors (CPU)
def _assign_differs(boxes, valid, gts, labels, cfg, plant):
    good = TA.assign_expect(boxes, valid, gts, labels, **cfg)
    again = TA.assign_expect(boxes, valid, gts, labels, **cfg)
    bad = TA.assign_expect(boxes, valid, gts, labels, plant=plant, **cfg)
    assert TA.same(good[0], again[0]) and good[3] == again[3]
    return not TA.same(good[0], bad[0]) or (good[2] is not None and not TA.same(good[2], bad[2]))


def test_assign_rejects_a_strict_positive_threshold():
    gts = np.array([[0, 0, 10, 10]], np.float32)
    boxes = np.array([[0, 0, 10, 5], [20, 20, 30, 30]], np.float32)   # IoU exactly 0.5
    cfg = dict(pos=0.5, neg_lo=0.0, neg_hi=0.5, min_pos=0.5, match_low_quality=False)
    assert TA.iou_expect(gts, boxes)[0, 0] == np.float32(0.5)
    assert TA.assign_expect(boxes, None, gts, None, **cfg)[0].tolist() == [1, 0]
    assert _assign_differs(boxes, None, gts, None, cfg, '> for >=')


def test_assign_rejects_the_last_argmax_on_a_tie():
    gts = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60]], np.float32)   # two identical gts
    boxes = np.array([[0, 0, 10, 9], [50, 50, 60, 61]], np.float32)
    cfg = dict(pos=0.5, neg_lo=0.0, neg_hi=0.5, min_pos=0.5, match_low_quality=False)
    assert TA.assign_expect(boxes, None, gts, None, **cfg)[0].tolist() == [1, 3]
    assert _assign_differs(boxes, None, gts, None, cfg, 'last argmax')


def test_assign_rejects_a_low_quality_loop_that_keeps_the_first_gt():
    gts = np.array([[0, 0, 10, 10], [0, 0, 10, 10]], np.float32)
    boxes = np.array([[0, 0, 10, 4], [30, 30, 40, 40]], np.float32)   # IoU 0.4 with both: below pos, their maximum
    cfg = dict(pos=0.7, neg_lo=0.0, neg_hi=0.3, min_pos=0.3, match_low_quality=True)
    assert TA.assign_expect(boxes, None, gts, None, **cfg)[0].tolist() == [2, 0]      # the later gt overwrites
    assert _assign_differs(boxes, None, gts, None, cfg, 'low quality keeps the first gt')


def test_assign_rejects_a_padding_row_in_a_gt_maximum():
    gts = np.array([[0, 0, 10, 10]], np.float32)
    boxes = np.array([[0, 0, 10, 6], [0, 0, 10, 4], [40, 40, 50, 50]], np.float32)
    valid = np.array([False, True, True])                               # row 0 (IoU 0.6) is padding
    cfg = dict(pos=0.7, neg_lo=0.0, neg_hi=0.3, min_pos=0.3, match_low_quality=True)
    gi, mo, _, counts = TA.assign_expect(boxes, valid, gts, None, **cfg)
    assert gi.tolist() == [-1, 1, 0] and np.isnan(mo[0]) and counts == (1, 1)
    assert _assign_differs(boxes, valid, gts, None, cfg, 'padding row in a gt maximum')


def test_add_gt_rejects_gts_behind_the_proposals():
    props, gts, labels = _inputs(0, n_prop=50)
    gi, mo, lab, _ = TA.assign_expect(props, None, gts, labels, **ASSIGN_CFGS[1])
    good = TA.add_gt_expect(props, gts, labels, gi, mo, lab)
    assert good[1][:5].tolist() == [1, 2, 3, 4, 5] and (good[3][:5] == 1).all() and TA.same(good[0][:5], gts)
    bad = TA.add_gt_expect(props, gts, labels, gi, mo, lab, plant='gts behind the proposals')
    assert not TA.same(good[0], bad[0]) and not TA.same(good[1], bad[1]) and not TA.same(good[4], bad[4])


def _sample_case(seed=0):
    rs = np.random.RandomState(seed)
    gis = []
    for n, npos in ((5000, 300), (4200, 40), (700, 400)):
        gi = np.zeros(n, np.int64)
        idx = rs.permutation(n)
        gi[idx[:npos]] = rs.randint(1, 9, npos)
        gi[idx[npos:npos + 50]] = -1
        gis.append(gi)
    torch.manual_seed(7 + seed)
    return gis, torch.get_rng_state()


def test_sampling_rejects_negatives_drawn_before_positives():
    gis, st = _sample_case()
    good, gs = TA.sample_expect(gis, 512, 0.25, -1, st)
    again, as_ = TA.sample_expect(gis, 512, 0.25, -1, st)
    assert TA.sample_matches(again, as_, good, gs)
    assert good[0][2]['n_pos'] > good[0][2]['want_pos'] and good[0][2]['n_neg'] > good[0][2]['want_neg']   # both draws run
    bad, bs = TA.sample_expect(gis, 512, 0.25, -1, st, plant='negatives first')
    assert not TA.sample_matches(bad, bs, good, gs)
    assert TA.same(bs, gs)                                              # the same number of draws: only the indices tell


def test_sampling_rejects_one_draw_too_many_and_one_too_few():
    """the indices are right, the generator is left one draw off: only the end state tells"""
    gis, st = _sample_case(1)
    good, gs = TA.sample_expect(gis, 512, 0.25, -1, st)
    more, ms = TA.sample_expect(gis, 512, 0.25, -1, st, plant='one draw too many')
    assert all(TA.same(a[0], b[0]) and TA.same(a[1], b[1]) for a, b in zip(more, good))
    assert not TA.sample_matches(more, ms, good, gs)
    # too few: the end state of a batch whose first image has one negative candidate less (randperm(n) consumes n - 1 draws)
    fewer = [x.copy() for x in gis]
    fewer[0][np.nonzero(fewer[0] == 0)[0][-1]] = -1
    _, fs = TA.sample_expect(fewer, 512, 0.25, -1, st)
    assert not TA.same(fs, gs) and not TA.sample_matches(good, fs, good, gs)


def test_sampling_rejects_unsorted_indices_and_a_float32_negative_bound():
    gis, st = _sample_case(2)
    good, gs = TA.sample_expect(gis, 512, 0.25, -1, st)
    bad, bs = TA.sample_expect(gis, 512, 0.25, -1, st, plant='unsorted')
    assert TA.same(bs, gs) and not TA.sample_matches(bad, bs, good, gs)
    assert all(TA.same(np.sort(a[0]), b[0]) for a, b in zip(bad, good))
    # int(neg_pos_ub * max(1, k_pos)) is a double product: 0.29 * 100 -> 28 (float32: 29)
    gi = np.zeros(3000, np.int64)
    gi[:100] = 1
    (s,), _ = TA.sample_expect([gi], 512, 0.25, 0.29, st)
    assert s[0].size == 100 and s[1].size == 28 and int(np.float32(0.29) * np.float32(100)) == 29


def _roi_case(seed=0, n_img=2, cap=None):
    rs = np.random.RandomState(40 + seed)
    entries = []
    for i in range(n_img):
        props, gts, labels = _inputs(seed + i, n_prop=300)
        gi, mo, lab, _ = TA.assign_expect(props, None, gts, labels, **ASSIGN_CFGS[1])
        bx, gi, lab, mo, _ = TA.add_gt_expect(props, gts, labels, gi, mo, lab)
        pos = np.sort(rs.permutation(np.nonzero(gi > 0)[0])[:12])
        neg = np.sort(rs.permutation(np.nonzero(gi == 0)[0])[:36 - 5 * i])
        entries.append(dict(bboxes=bx, gts=gts, gt_inds=gi, labels=lab, pos_inds=pos, neg_inds=neg, cap=cap))
    extra = [rs.uniform(0, 100, (7, 4)).astype(np.float32), rs.uniform(0, 100, (4, 4)).astype(np.float32)]
    return entries, extra


MEANS, STDS = (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)


def _roi_got(exp):
    return dict(rois=exp['rois'], K=exp['K'], labels=exp['labels'], label_weights=exp['label_weights'],
                bbox_targets=exp['deltas'].astype(np.float32), bbox_weights=exp['bbox_weights'], absolute=exp['absolute'])


def _roi_plant(plant, pos_weight=-1.0, field=None):
    entries, extra = _roi_case()
    exp = TA.roi_targets_expect(entries, 8, pos_weight, MEANS, STDS, extra)
    ok, worst = TA.roi_targets_match(_roi_got(exp), exp)
    assert all(ok.values()) and worst <= 1.0, (ok, worst)               # its own float32 rounding is within the bound
    bad = TA.roi_targets_expect(entries, 8, pos_weight, MEANS, STDS, extra, plant=plant)
    ok, worst = TA.roi_targets_match(_roi_got(bad), exp)
    return ok, worst


def test_roi_targets_reference_by_hand():
    """two positives, one negative, one extra box: every field written out"""
    bx = np.array([[0, 0, 10, 10], [2, 2, 12, 12], [50, 50, 60, 60], [0, 0, 20, 20]], np.float32)
    gts = np.array([[0, 0, 10, 10]], np.float32)
    e = dict(bboxes=bx, gts=gts, gt_inds=np.array([1, 1, 0, 0]), labels=np.array([3, 3, -1, -1]),
             pos_inds=np.array([0, 1]), neg_inds=np.array([2]))
    exp = TA.roi_targets_expect([e, e], 8, 2.0, (0,) * 4, (1,) * 4, extra=[bx[3:]])
    assert exp['K'] == 6 and exp['rois'].shape == (7, 5)
    assert exp['rois'][:, 0].tolist() == [0, 0, 0, 1, 1, 1, 0]          # the extra list restarts at its own position 0
    assert exp['rois'][1, 1:].tolist() == [2, 2, 12, 12] and exp['rois'][6, 1:].tolist() == [0, 0, 20, 20]
    assert exp['labels'].tolist() == [3, 3, 8, 3, 3, 8] and exp['label_weights'].tolist() == [2, 2, 1, 2, 2, 1]
    assert exp['bbox_weights'][:, 0].tolist() == [1, 1, 0, 1, 1, 0]
    assert exp['absolute'][1].tolist() == [0, 0, 10, 10] and not exp['absolute'][2].any()
    assert np.allclose(exp['deltas'][1], [-0.2, -0.2, 0, 0]) and not exp['deltas'][0].any() and exp['one_sided'] == 0


def test_targets_reject_label_fill_0_for_num_classes():
    ok, _ = _roi_plant('label fill 0')
    assert not ok['labels'] and ok['rois'] and ok['absolute']
    an = np.array([[0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]], np.float32)
    im = dict(gts=an[:1], gt_inds=np.array([1, 0, 0]), pos_inds=np.array([0]), neg_inds=np.array([1]))
    good = TA.anchor_targets_expect(an, [im], 1, -1, MEANS, STDS)
    assert good['labels'].tolist() == [[0, 1, 1]] and good['label_weights'].tolist() == [[1, 1, 0]]
    got = dict(labels=good['labels'], label_weights=good['label_weights'], bbox_weights=good['bbox_weights'],
               bbox_targets=np.zeros((1, 3, 4), np.float32))
    assert all(TA.anchor_targets_match(got, good)[0].values())
    bad = TA.anchor_targets_expect(an, [im], 1, -1, MEANS, STDS, plant='label fill 0')
    got['labels'] = bad['labels']
    assert not TA.anchor_targets_match(got, good)[0]['labels']
    got['labels'] = good['labels']
    got['bbox_targets'][0, 2, 1] = 1e-3                                 # a stale value on an unsampled row
    assert not TA.anchor_targets_match(got, good)[0]['bbox_targets of unsampled rows are 0']


def test_targets_reject_an_ignored_pos_weight():
    ok, _ = _roi_plant('pos_weight ignored', pos_weight=2.0)
    assert not ok['label_weights'] and ok['labels']


def test_targets_reject_the_statistics_of_dw_applied_to_dx():
    ok, worst = _roi_plant('dw statistics on dx')
    assert all(ok.values()) and worst > 1.0


def test_targets_reject_absolute_boxes_taken_from_the_proposal():
    ok, worst = _roi_plant('absolute from the proposal')
    assert not ok['absolute'] and ok['rois'] and worst <= 1.0


def test_targets_reject_extra_rois_that_continue_the_batch_index():
    ok, _ = _roi_plant('extra rois continue the batch index')
    assert not ok['rois'] and ok['labels'] and ok['K']


def test_targets_compare_live_rows_only_when_an_image_is_short():
    entries, extra = _roi_case(cap=64)
    exp = TA.roi_targets_expect(entries, 8, -1, MEANS, STDS, extra)
    assert exp['K'] == 128 and int(exp['live'].sum()) == sum(len(e['pos_inds']) + len(e['neg_inds']) for e in entries) < 128
    got = _roi_got(exp)
    got['rois'] = got['rois'].copy()
    got['rois'][~exp['live_all']] = 77.0                                # padding rows are not the reference's business
    assert all(TA.roi_targets_match(got, exp)[0].values())
    got['rois'][0, 1] += 1
    assert not TA.roi_targets_match(got, exp)[0]['rois']


# -------------------------------------------------------------------------------------------- closure on the source (CPU)
# size / plan / capability queries: host arithmetic, nothing is launched
LAUNCHES_NOTHING = {
    'oadg_cls_loss_workspace_bytes', 'oadg_conv2d_auto_variant', 'oadg_conv2d_pixel_tiles', 'oadg_conv2d_wgrad_f32_splits',
    'oadg_conv2d_wgrad_multi_plan', 'oadg_conv2d_wgrad_variant', 'oadg_conv2d_wgrad_workspace_bytes',
    'oadg_conv1x1_n16_dgrad_rows', 'oadg_conv1x1_n16_wgrad_rows', 'oadg_jpeg_coef_capacity',
    'oadg_max_iou_assign_workspace_bytes', 'oadg_nms_workspace_bytes', 'oadg_oamix_bbox_plan_bytes',
    'oadg_oamix_final_tiles_workspace_bytes', 'oadg_oamix_saliency_workspace_bytes', 'oadg_prep_conv_weights_multi_blocks',
    'oadg_relu_bias_bwd_workspace_bytes', 'oadg_roi_sample_max_rows', 'oadg_rpn_loss_workspace_bytes',
    'oadg_rpn_topk_workspace_bytes', 'oadg_sample_select_workspace_bytes', 'oadg_sgd_blocks', 'oadg_supcon_workspace_bytes',
}
# the data pipeline, OA-Mix, the decoders and the corruptions: they run before an audited step installs anything (or not
# in it at all) and have byte-exact suites of their own (tests/test_hip_oamix.py, test_oracle_oamix.py,
# test_oamix_buffers.py, test_oamix_ops.py, test_geometric.py, test_jpeg_decode.py, test_decoder_robustness.py,
# test_sdgod_dataset.py, test_hip_corrupt.py, test_corrupt.py) - not part of the audited step.  (The fp32 parity convolutions are audited launch by launch in the fp32
# step: tests/f32_audit.py)
OWN_SUITES = {
    'oadg_chamfer_l2_5x5', 'oadg_glass_shuffle_u8', 'oadg_corrupt_correlate1d', 'oadg_corrupt_defocus', 'oadg_corrupt_elastic',
    'oadg_corrupt_epilogue', 'oadg_corrupt_hsv', 'oadg_corrupt_motion_blur_f64', 'oadg_corrupt_motion_blur_u8',
    'oadg_corrupt_snow_blend', 'oadg_corrupt_snow_layer', 'oadg_corrupt_zoom_blur', 'oadg_flip_u8', 'oadg_resize_bilinear_u8',
    'oadg_jpeg_entropy_decode', 'oadg_jpeg_pixels_bgr', 'oadg_png_decode_bgr', 'oadg_oamix_bbox_chain',
    'oadg_oamix_bbox_chain_multi', 'oadg_oamix_bbox_levels', 'oadg_oamix_bbox_plan', 'oadg_oamix_bbox_step',
    'oadg_oamix_box_profiles', 'oadg_oamix_compose', 'oadg_oamix_fg_union', 'oadg_oamix_fg_union_rects', 'oadg_oamix_final',
    'oadg_oamix_final_tiles', 'oadg_oamix_gray_sum', 'oadg_oamix_hist', 'oadg_oamix_luts', 'oadg_oamix_normalize',
    'oadg_oamix_saliency', 'oadg_oamix_saliency_batch',
}
CLAIM_SETS = {'conv audit': CA.CLAIMS, 'head audit': HA.CLAIMS, 'infer audit': IA.CLAIMS, 'target audit': TA.CLAIMS,
              'f32 audit': FA.CLAIMS, 'launches nothing': LAUNCHES_NOTHING, 'own suites': OWN_SUITES}
# the ``what`` a call reports through _lib.check where it is not the symbol's name
LABEL_OF = {'oadg_conv2d_nhwc_bf16_ex': 'oadg_conv2d_nhwc_bf16'}


def called_symbols(root=os.path.join(ROOT, 'oa-dg_amd')):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith('.py'):
                with open(os.path.join(d, f)) as fh:
                    for m in re.finditer(r'\.(oadg_\w+)', fh.read()):
                        out.setdefault(m.group(1), set()).add(os.path.relpath(os.path.join(d, f), root))
    return out


def unclaimed(symbols, sets):
    """(symbols no set claims, symbols more than one set claims, claimed names nothing calls)"""
    owners = {s: [k for k, v in sets.items() if s in v] for s in symbols}
    stale = sorted(set().union(*sets.values()) - set(symbols))
    return sorted(s for s, o in owners.items() if not o), sorted(s for s, o in owners.items() if len(o) > 1), stale


def test_every_c_abi_call_site_is_claimed_by_exactly_one_suite():
    syms = called_symbols()
    assert len(syms) > 100 and 'oadg_np_random_bboxes' in syms and 'oadg_host_randperm_prefix' in syms
    none, many, stale = unclaimed(syms, CLAIM_SETS)
    assert not none, 'C-ABI calls no suite answers for: %s' % [(s, sorted(syms[s])) for s in none]
    assert not many, many
    assert not stale, 'claimed, but called nowhere: %s' % stale
    # the queries are recognisable by name; nothing that launches hides among them
    assert all(re.search(r'_(bytes|blocks|rows|splits|variant|plan|capacity|tiles)$', s) for s in LAUNCHES_NOTHING)


def test_closure_fails_when_a_name_leaves_its_claim_set():
    syms = called_symbols()
    for name, victim in (('target audit', 'oadg_roi_sample_device'), ('head audit', 'oadg_supcon_bwd'),
                         ('launches nothing', 'oadg_sgd_blocks')):
        sets = {k: set(v) - ({victim} if k == name else set()) for k, v in CLAIM_SETS.items()}
        assert unclaimed(syms, sets)[0] == [victim]
    sets = dict(CLAIM_SETS, extra={'oadg_nms_batched'})
    assert unclaimed(syms, sets)[1] == ['oadg_nms_batched']


# ------------------------------------------------------------------------------------------------- GPU audited steps
WRAPPERS = {'MaxIoUAssigner.assign_many', 'PendingSampling.finish', 'AnchorHead._fused_targets', 'BBoxHead.rois_and_targets',
            'roi_assign_sample_begin', 'RPNHead.get_bboxes', 'nms_sorted_batched', 'generate_random_bboxes_xy',
            'randperm_prefix (oadg_host_randperm_prefix)'}
_OTHERS = {LABEL_OF.get(s, s) for s in CA.CLAIMS | HA.CLAIMS}
_PROPOSALS = {'oadg_rpn_decode', 'oadg_rpn_order', 'oadg_rpn_gather', 'oadg_nms_batched'}
_RPN = {'oadg_max_iou_assign', 'oadg_sample_select', 'oadg_anchor_targets', 'oadg_host_randperm_prefix', 'oadg_np_random_bboxes',
        'oadg_roi_assign_add_gt'}
CHECKED = {'device': _PROPOSALS | _RPN | {'oadg_rpn_topk', 'oadg_roi_sample_device', 'oadg_roi_targets_dev'},
           'host': _PROPOSALS | _RPN | {'oadg_rpn_topk', 'oadg_roi_targets'}}


def _target_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size, key, speculative=True,
                 fused_anchor_targets=True):
    A = TA.Auditor()
    out, det, wall = audited_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size,
                                  lambda mp, det: A.install(mp, det),
                                  speculative_sampling=None if speculative else False)
    drew_on_device = A.check_end_state()                # engine.step has returned: sync_host is behind us
    A.print_table('%s (audited step %.1f s)' % (key, wall))
    assert not A.failures, A.failures[:10]
    missing = WRAPPERS - set(A.wrappers)
    assert not missing, missing
    assert not A.declined, A.declined
    assert drew_on_device == speculative
    # positives exist, and every generator check had something to check
    assert A.n_pos['rpn'] and min(A.n_pos['rpn']) > 0 and A.n_pos['roi'] and min(A.n_pos['roi']) > 0, A.n_pos
    rpn = [d for d in A.draws if d['kind'] == 'rpn']
    roi = [d for d in A.draws if d['kind'] == 'roi']
    assert rpn and roi and len(roi) == batch
    assert all(d['branch'] == 'host' and d['n_neg'] > d['want_neg'] and d['k_pos'] > 0 for d in rpn), rpn
    assert all(d['branch'] == ('device' if speculative else 'host') and d['n_neg'] > d['want_neg'] and d['k_pos'] > 0 and
               d['k_pos'] + d['k_neg'] == 512 for d in roi), roi
    assert all(k == 'oadg_roi_targets_dev' if speculative else k == 'oadg_roi_targets' for k in A.info['roi_targets_entry'])
    assert all(n > 0 for per in A.info['roi_sampled_pos'] for n in per)
    assert A.info['proposals'] == 'fused' and all(k > 0 for k in A.info['proposals_kept'])
    # closure at run time: every label a check() saw during the audited step is the other auditors' or verified here
    seen = set(A.labels) | ({'oadg_host_randperm_prefix', 'oadg_np_random_bboxes'} & A.checked)
    mine = seen - _OTHERS
    assert mine == A.checked, ('unclaimed', sorted(mine - A.checked), 'checked but not seen', sorted(A.checked - mine))
    want = CHECKED['device' if speculative else 'host'] - (set() if fused_anchor_targets else {'oadg_anchor_targets'})
    assert A.info['anchor_targets'] == ('fused' if fused_anchor_targets else 'tensor path')
    assert ('anchor targets (tensor path) labels' in A.table) != fused_anchor_targets
    assert A.checked == want, (sorted(A.checked - want), sorted(want - A.checked))
    assert A.one_sided == 0, A.one_sided                # KNOWN_DEVIATION_ENCODE_DELTA cannot matter in this step
    assert not A.borderline, A.borderline
    return A


@pytest.mark.gpu
def test_target_audit_config1_r50_fpn_bench_step(dev, monkeypatch):
    """configs[1] as bench.py builds it: 4 images x 2 views at 1024 x 2048 - 8 x 523,776 anchors, 4 x 1000 padded proposals"""
    _target_step(dev, monkeypatch, R50_CFG, 4, 1024, 2048, 20, 8, (24, 400), 'r50_fpn')


@pytest.mark.gpu
def test_target_audit_config3_r101_dc5(dev, monkeypatch):
    """configs[3]: R101-DC5 at 736 x 1280 - 15 anchors per pixel on one level.  Its RPN filters anchors at the border
    (allowed_border = 0): the assignment takes the validity mask and the anchor targets the tensor path - outside
    oadg_anchor_targets' domain -, whose outputs are judged by the same reference"""
    _target_step(dev, monkeypatch, DC5_CFG, 2, 736, 1280, 12, 7, (24, 300), 'r101_dc5', fused_anchor_targets=False)


@pytest.mark.gpu
def test_target_audit_multiscale_800x1600(dev, monkeypatch):
    _target_step(dev, monkeypatch, R50_CFG, 2, 800, 1600, 12, 8, (24, 300), 'r50_fpn_multiscale')


# 256 x 512: every image there still has more RoI candidates than the sampler's num (asserted: k_pos + k_neg == 512)
HOST_STEP_SHAPE = (256, 512)


@pytest.mark.gpu
def test_target_audit_host_sampler_step(dev, monkeypatch):
    """TrainEngine.speculative_sampling = False - what every multi-rank run on a backend other than RCCL takes: the RoI
    draws on the host, oadg_sample_select on RoI rows, oadg_roi_targets (the entry without device-side counts)"""
    _target_step(dev, monkeypatch, R50_CFG, 2, HOST_STEP_SHAPE[0], HOST_STEP_SHAPE[1], 12, 8, (24, 300), 'r50_fpn_host_sampler',
                 speculative=False)


# ----------------------------------------------------------------------------------------------- GPU stress launches
def _boxes(rs, n, W=640, H=480, lo=8, hi=200):
    x, y = rs.uniform(0, W - lo, n), rs.uniform(0, H - lo, n)
    w, h = rs.uniform(lo, hi, n), rs.uniform(lo, hi, n)
    return np.stack([x, y, np.minimum(x + w, W), np.minimum(y + h, H)], 1).astype(np.float32)


def _stress_images(rs, N, gt_counts, all_padding=()):
    """per image: proposals [N, 5] (jittered gts, exact copies of gts, zero-area boxes, random boxes, a tail of score -1
    padding rows), gts (the first two identical when there are at least two), labels"""
    props, gts, labels = [], [], []
    for b, G in enumerate(gt_counts):
        g = _boxes(rs, G)
        if G >= 2:
            g[1] = g[0]
        p = _boxes(rs, N, lo=4, hi=260)
        k = min(G, N // 8)
        if k:
            p[:k] = g[:k] + rs.uniform(-4, 4, (k, 4)).astype(np.float32)
            p[k:2 * k] = g[:k]                                          # proposals equal to a gt
            p[2 * k:3 * k] = g[:k] + np.float32(0.5)
        p[3 * k:3 * k + 5, 2] = p[3 * k:3 * k + 5, 0]                   # zero-area proposals
        p[3 * k + 5:3 * k + 8, 2:] = p[3 * k + 5:3 * k + 8, :2]
        s = np.sort(rs.uniform(0.01, 1, N).astype(np.float32))[::-1].copy()
        s[N - N // 7:] = -1                                             # padding rows ...
        p[N - N // 7:] = 0
        if b in all_padding:
            s[:], p[:] = -1, 0
        props.append(np.concatenate([p, s[:, None]], 1))
        gts.append(g)
        labels.append(rs.randint(0, 8, G).astype(np.int64))
    return props, gts, labels


def _to(dev, arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _finish_stress(A, title, want_declined=()):
    torch.cuda.synchronize()
    A.print_table(title)
    assert not A.failures, A.failures[:10]
    assert sorted(A.declined) == sorted(want_declined), A.declined
    assert not A.borderline
    return A


@pytest.mark.gpu
@pytest.mark.parametrize('form', ['roi', 'assign_many'])
def test_target_stress_assignment(dev, monkeypatch, form):
    """two identical gts, proposals equal to a gt, zero-area proposals, an image without gts beside images with gts, an
    image whose proposals are all padding, N not a multiple of 256, neg_iou_thr as a tuple, match_low_quality in the RoI
    form"""
    from oadg_amd.core import bbox as BB
    rs = np.random.RandomState(3)
    N = 1000
    props, gts, labels = _stress_images(rs, N, [7, 0, 3, 12], all_padding=(2,))
    P, G, L = _to(dev, props), _to(dev, gts), _to(dev, labels)
    asg = BB.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=(0.1, 0.5), min_pos_iou=0.3, match_low_quality=True,
                            ignore_iof_thr=-1)
    smp = BB.RandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    A = TA.Auditor().install(monkeypatch)
    if form == 'roi':
        pend = BB.roi_assign_sample_begin(asg, smp, P, G, L)
        assert pend is not None
        torch.manual_seed(5)
        res = pend.finish()                                             # (no speculation record: the host branch)
        assert [int(r.neg_inds.numel()) for r in res][2] == 0          # all padding: no negative candidate
        assert A.wrappers['roi_assign_sample_begin'] == 1 and A.wrappers['PendingSampling.finish'] == 1
        assert A.info['roi_padding_rows'][2] == N
    else:
        out = asg.assign_many([p[:, :4] for p in P], [p[:, 4] >= 0 for p in P], G, L)
        assert out is not None and A.wrappers['MaxIoUAssigner.assign_many'] == 1
        # shared boxes, no validity mask, no labels: the RPN's form
        out = asg.assign_many(P[0][:, :4].contiguous(), None, G, None)
        assert out is not None
    monkeypatch.undo()
    _finish_stress(A, 'assignment stress (%s)' % form)
    assert ('assign_kernel gt_inds (RoI form, padding rows -1)' if form == 'roi' else 'assign_kernel gt_inds') in A.table


@pytest.mark.gpu
def test_target_stress_assignment_1024_gts_run_and_1025_are_declined(dev, monkeypatch):
    """declined means the tensor path (the callers loop), not an error"""
    from oadg_amd.core import bbox as BB
    rs = np.random.RandomState(4)
    asg = BB.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1)
    smp = BB.RandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    A = TA.Auditor().install(monkeypatch)
    for G, runs in ((1024, True), (1025, False)):
        props, gts, labels = _stress_images(rs, 300, [G, 5])
        P, Gt, L = _to(dev, props), _to(dev, gts), _to(dev, labels)
        pend = BB.roi_assign_sample_begin(asg, smp, P, Gt, L)
        out = asg.assign_many([p[:, :4] for p in P], [p[:, 4] >= 0 for p in P], Gt, L)
        assert (pend is not None) == runs and (out is not None) == runs
    monkeypatch.undo()
    _finish_stress(A, 'assignment stress (Gmax 1024 / 1025)', want_declined=['roi_assign_sample_begin', 'assign_many'])
    assert A.table['assign_kernel gt_inds'].calls == 2 and A.table['assign_kernel gt_inds (RoI form, padding rows -1)'].calls == 2


def _pending(BB, dev, gis, sampler):
    """a PendingSampling as roi_assign_sample_begin leaves it, on constructed gt_inds (gts-as-proposals rows included)"""
    prepared = []
    for gi in gis:
        t = torch.from_numpy(gi).to(dev)
        ar = BB.AssignResult(0, t, torch.zeros(len(gi), device=dev), labels=torch.zeros(len(gi), dtype=torch.long, device=dev))
        prepared.append((ar, torch.zeros((len(gi), 4), device=dev), 0, (lambda a_=ar: a_.gt_inds > 0),
                         (lambda a_=ar: a_.gt_inds == 0)))
    counts = torch.tensor([[int((g > 0).sum()), int((g == 0).sum())] for g in gis], dtype=torch.int32, device=dev)
    pend = BB.PendingSampling(sampler, prepared, [torch.zeros((0, 4), device=dev)] * len(gis), counts, [0] * len(gis))
    pend._scratch = counts
    return pend


def _gt_inds(rs, n, npos, nneg=None):
    gi = np.full(n, -1, np.int64)
    idx = rs.permutation(n)
    gi[idx[:npos]] = rs.randint(1, 20, npos)
    nneg = n - npos if nneg is None else nneg
    gi[idx[npos:npos + nneg]] = 0
    return gi


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['4096 rows', '4097 rows', 'short image', 'neg_pos_ub 0.29', 'neg_pos_ub 3'])
def test_target_stress_device_sampler(dev, monkeypatch, case):
    """rows 4096 (runs) and 4097 (declined: the host branch draws), an image with fewer candidates than num (flag raised,
    live rows only), draws that cross MT19937 reloads inside an image and between images (thousands of candidates, a
    start a few draws before a reload), a fractional and an integral negative / positive bound"""
    from oadg_amd import device_rng
    from oadg_amd.core import bbox as BB
    rs = np.random.RandomState(6)
    ub = {'neg_pos_ub 0.29': 0.29, 'neg_pos_ub 3': 3}.get(case, -1)
    smp = BB.RandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=ub, add_gt_as_proposals=True)
    n = 4097 if case == '4097 rows' else 4096
    gis = [_gt_inds(rs, n, 300), _gt_inds(rs, 1100, 40), _gt_inds(rs, n, 100, 3000), _gt_inds(rs, 2000, 700)]
    if case == 'short image':
        gis[1] = _gt_inds(rs, 1100, 30, 200)
    torch.manual_seed(21)
    torch.randperm(624 * 2 - 37)                    # leaves the engine 37 draws before its next reload
    A = TA.Auditor().install(monkeypatch)
    BB.begin_speculation()
    try:
        res = _pending(BB, dev, gis, smp).finish()
        torch.cuda.synchronize()
    finally:
        recs = BB.end_speculation()
    device = case != '4097 rows'
    assert isinstance(res[0], BB.DeviceSamplingResult) == device
    if device:
        assert device_rng.sync_all() and A.check_end_state()
        flags = recs[-1]['meta'].numpy()[2 * len(gis):]
        assert bool(flags.any()) == (case in ('short image', 'neg_pos_ub 0.29', 'neg_pos_ub 3')), flags
    monkeypatch.undo()
    _finish_stress(A, 'device sampler stress (%s)' % case)
    d = A.draws
    assert all(x['branch'] == ('device' if device else 'host') for x in d)
    assert d[0]['n_pos'] > d[0]['want_pos'] and all(x['n_neg'] > x['want_neg'] for x in d if not (case == 'short image' and x['image'] == 1))
    if case == 'neg_pos_ub 0.29':
        assert (d[2]['k_pos'], d[2]['k_neg']) == (100, 28)             # int(0.29 * 100) in double; float32 gives 29
    if case == 'short image':
        assert d[1]['k_pos'] + d[1]['k_neg'] == 230


def _roi_launch(dev, monkeypatch, props, gts, labels, branch):
    """roi_assign_sample_begin -> finish (host or device branch) -> BBoxHead.rois_and_targets of the R50-FPN config's head
    on constructed proposals, under the auditor: (auditor, head, sampling results, rois_and_targets' output, device flags)"""
    from oadg_amd import Config, build_detector, device_rng
    from oadg_amd.core import bbox as BB
    P, G, L = _to(dev, props), _to(dev, gts), _to(dev, labels)
    asg = BB.MaxIoUAssigner(pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5, match_low_quality=False, ignore_iof_thr=-1)
    smp = BB.RandomSampler(num=512, pos_fraction=0.25, neg_pos_ub=-1, add_gt_as_proposals=True)
    cfg = Config.fromfile(R50_CFG)
    head = build_detector(cfg.model).roi_head.bbox_head
    A = TA.Auditor().install(monkeypatch)
    torch.manual_seed(3)
    flags = None
    if branch == 'device':
        BB.begin_speculation()
    try:
        res = BB.roi_assign_sample_begin(asg, smp, P, G, L).finish()
        out = head.rois_and_targets(res, cfg.model.train_cfg.rcnn)
        torch.cuda.synchronize()
    finally:
        if branch == 'device':
            recs = BB.end_speculation()
            assert device_rng.sync_all() and A.check_end_state()
            flags = recs[-1]['meta'].numpy()[2 * len(props):].tolist()
    monkeypatch.undo()
    assert isinstance(res[0], BB.DeviceSamplingResult) == (branch == 'device') and out is not None
    return A, head, res, out, flags


@pytest.mark.gpu
def test_target_stress_short_image_on_the_device_path(dev, monkeypatch):
    """an image with fewer candidates than the sampler's num on the device path: its flag is raised (the trainer repeats
    such a step on the host path), roi_targets_kernel fills the fixed capacity and only the live rows - the first
    k_pos + k_neg of the image - are compared; the image beside it is full"""
    rs = np.random.RandomState(9)
    props, gts, labels = _stress_images(rs, 700, [6, 6])
    props[0][100:, 4], props[0][100:, :4] = -1, 0                       # 100 valid proposals + 6 gts: 106 rows of 512
    A, head, res, out, flags = _roi_launch(dev, monkeypatch, props, gts, labels, 'device')
    _finish_stress(A, 'short image, device path')
    assert flags == [1, 0]
    d = A.draws
    assert d[0]['k_pos'] + d[0]['k_neg'] == d[0]['n_pos'] + d[0]['n_neg'] == 106 and d[1]['k_pos'] + d[1]['k_neg'] == 512
    assert out[1] == 1024 and A.info['roi_targets_entry'] == ['oadg_roi_targets_dev']
    assert A.table['roi_targets_kernel rois (oadg_roi_targets_dev)'].calls == 1


@pytest.mark.gpu
@pytest.mark.parametrize('branch', ['host', 'device'])
def test_target_stress_zero_size_positives(dev, monkeypatch, branch):
    """gts added as proposals make a positive with a zero side reachable: rows with zero width only, zero height only and
    both.  The tensor path (core/bbox.py bbox2delta) is the golden's positional rule.  The fused kernel is asserted to do
    what it DOES (KNOWN_DEVIATION_ENCODE_DELTA): equal to the reference where a row is degenerate in both dimensions or
    in none, the row-wise formula for a one-sided row - there the reference pairs by position (and raises when the counts
    of zero-width and zero-height rows differ; here they are equal, 2 and 2)."""
    from oadg_amd.core import bbox as BB
    rs = np.random.RandomState(8)
    gts = _boxes(rs, 6)
    gts[1, 2] = gts[1, 0]                           # zero width only
    gts[2, 3] = gts[2, 1]                           # zero height only
    gts[3, 2:] = gts[3, :2]                         # both
    props = _boxes(rs, 700, lo=4, hi=260)
    props[:6] = gts + rs.uniform(-3, 3, (6, 4)).astype(np.float32)
    props = np.concatenate([props, np.sort(rs.uniform(0.01, 1, 700).astype(np.float32))[::-1][:, None]], 1)
    labels = rs.randint(0, 8, 6).astype(np.int64)
    A, head, res, out, flags = _roi_launch(dev, monkeypatch, [props], [gts], [labels], branch)
    pos = TA._np(res[0].pos_inds)
    assert pos[:6].tolist() == [0, 1, 2, 3, 4, 5]   # the six gts lead the positives (fewer than 128 candidates: all taken)
    rois, K, (lab, lw, bt, bw, ab) = out
    bx = TA._np(res[0]._src[0])
    gi = TA._np(res[0]._src[2].gt_inds)
    pb, pg = bx[pos], gts[gi[pos] - 1]
    coder = head.bbox_coder
    kernel = TA._np(bt)[:len(pos)]
    # 1. the tensor path is the golden rule
    tensor = BB.bbox2delta(torch.from_numpy(pb).to(dev), torch.from_numpy(pg).to(dev), coder.means, coder.stds)
    r, S, one_sided = TA.delta_expect(pb, pg, coder.means, coder.stds, rule='positional')
    assert one_sided == 2
    print('tensor path vs positional rule: %.4f' % TA.delta_ratio(tensor, r, S))
    assert TA.delta_ratio(tensor, r, S) <= 1.0
    # 2. the kernel: the row-wise formula everywhere ...
    rw, Sw, _ = TA.delta_expect(pb, pg, coder.means, coder.stds, rule='rowwise')
    print('kernel vs row-wise rule: %.4f' % TA.delta_ratio(kernel, rw, Sw))
    assert TA.delta_ratio(kernel, rw, Sw) <= 1.0, TA.KNOWN_DEVIATION_ENCODE_DELTA
    # ... which is the reference's except on the zero-width-only row (row 1: dy = (py[2] - py[1]) / ph[1] there, 0 here)
    rest = np.ones(len(pos), bool)
    rest[1] = False
    assert TA.delta_ratio(kernel[rest], r[rest], S[rest]) <= 1.0
    assert kernel[1, 1] == 0.0 and abs(r[1, 1]) > 1.0 and TA.delta_ratio(kernel[1], r[1], S[1]) > 1.0, \
        TA.KNOWN_DEVIATION_ENCODE_DELTA
    # the auditor saw the same launch and judges by the reference's rule: every exact field right, the two one-sided rows
    # counted, and the deviation flagged - an audited step with such a positive would fail on exactly this row
    A.print_table('zero-size positives (%s)' % branch)
    assert A.one_sided == 2
    assert [f[0] for f in A.failures] == ['roi_targets_kernel deltas (err / bound, GAMMA_T)'], A.failures
