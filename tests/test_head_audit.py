"""Elementwise fp64 audit of the non-convolution launches of a real training step (tests/head_audit.py): RoIAlign and its
order, the RPN / RoI losses, supcon, _parse_losses, the RoI head's casts and permutation, the fused SGD step.

CPU self-tests tie each fp64 reference to oracle/ and show that the checker rejects planted errors.  GPU tests (``-m gpu``)
audit the workloads of tests/test_conv_audit.py plus one stress launch of RoIAlign.
"""
import pytest
import torch

import head_audit as HA
from audit_workload import DC5_CFG, R50_CFG, audited_step
from oracle import losses as OL
from oracle import roi_align as ORA


def _worst(o, ref, b):
    return HA.ratio(o, ref, b)[0]


# ------------------------------------------------------------------------------------------------ RoIAlign references
def _pyramid(seed=0, N=2, C=8, sizes=((32, 40), (16, 20), (8, 10)), dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((N, C) + s, generator=g).to(dtype) for s in sizes]


def _rois(K=40, seed=1, N=2, W=160, H=128, lo=4, hi=120):
    g = torch.Generator().manual_seed(seed)
    x1 = torch.rand(K, generator=g) * W * 0.8 - 4
    y1 = torch.rand(K, generator=g) * H * 0.8 - 4
    w = lo + torch.rand(K, generator=g) * (hi - lo)
    h = lo + torch.rand(K, generator=g) * (hi - lo)
    b = torch.randint(0, N, (K,), generator=g).float()
    return torch.stack([b, x1, y1, x1 + w, y1 + h], 1)


SCALES = (0.25, 0.125, 0.0625)


def _fwd(feats, rois, PH=7, PW=7, aligned=True, finest=8, **kw):
    shapes = [tuple(f.shape) for f in feats]
    lvl, geo, near = HA.roi_setup(rois, shapes, SCALES, finest, PH, PW, 0, aligned)
    for k, v in kw.items():
        if k == 'lvl':
            lvl = v
        else:
            geo[k] = v
    r, S, S4 = HA.roi_align_ref(feats, rois, lvl, geo, PH, PW)
    return r, HA.bound(r, S, 0.0, HA.GAMMA_ROI, HA.POS_ERR * S4), lvl, geo


def _oracle_fwd(feats, rois, aligned=True, finest=8):
    return ORA.roi_align_fpn(feats, rois, 7, [1 / s for s in SCALES], finest, 0, aligned).permute(0, 2, 3, 1).double()


def test_roi_align_reference_matches_the_oracle():
    feats, rois = _pyramid(), _rois()
    r, b, lvl, _ = _fwd(feats, rois)
    assert len(set(lvl.tolist())) == 3                      # all three levels reached
    assert _worst(_oracle_fwd(feats, rois), r, b) <= 0.25
    assert torch.equal(lvl, ORA.map_roi_levels(rois, 3, 8))


def test_roi_align_rejects_a_missing_half_pixel_offset():
    feats, rois = _pyramid(), _rois()
    r, b, _, _ = _fwd(feats, rois)
    assert _worst(_oracle_fwd(feats, rois, aligned=False), r, b) > 1.0


def test_roi_align_rejects_a_plain_clamp_at_the_edge():
    # samples between size - 1 and size: the edge rule reads the last row with weight 1; a plain clamp of both corners
    # to size - 1 keeps the fractional weight split and agrees, so plant the other plain form: high = low + 1 clamped,
    # low = floor(y) (the fractional part not reset to 0) - the last row then carries weight (1 - l) only
    feats = _pyramid(sizes=((16, 16),), N=1)
    rois = torch.tensor([[0, 40.0, 40.0, 66.0, 66.0]])                # ends past the map's last pixel at 1/4
    shapes = [tuple(feats[0].shape)]
    lvl, geo, _ = HA.roi_setup(rois, shapes, (0.25,), 8, 7, 7, 0, True)
    r, S, S4 = HA.roi_align_ref(feats, rois, lvl, geo, 7, 7)
    b = HA.bound(r, S, 0.0, HA.GAMMA_ROI, HA.POS_ERR * S4)
    orig = HA._axis

    def plain(start, binsz, grid, i, P, size, shift):
        low, high, hw, lw, inside = orig(start, binsz, grid, i, P, size, shift)
        p = torch.arange(P, dtype=torch.float64).view(1, P)
        c = (start.view(-1, 1) + p * binsz.view(-1, 1) + (i + 0.5) * binsz.view(-1, 1) /
             grid.clamp_min(1).double().view(-1, 1)).clamp_min(0)
        lo = c.floor().long().clamp_max(size.view(-1, 1) - 1)
        frac = c - c.floor()
        return lo, (lo + 1).clamp_max(size.view(-1, 1) - 1), 1 - frac, frac * (lo + 1 < size.view(-1, 1)), inside
    HA._axis = plain
    try:
        bad, _, _ = HA.roi_align_ref(feats, rois, lvl, geo, 7, 7)
    finally:
        HA._axis = orig
    assert _worst(bad, r, b) > 1.0
    assert _worst(ORA.roi_align(feats[0], rois, 7, 0.25).permute(0, 2, 3, 1).double(), r, b) <= 0.25


def test_roi_align_rejects_one_roi_on_the_neighbouring_level():
    feats, rois = _pyramid(), _rois()
    r, b, lvl, geo = _fwd(feats, rois)
    k = int((lvl == 1).nonzero()[0])
    l2 = lvl.clone()
    l2[k] = 0
    g2 = HA.roi_geometry(rois, l2, [tuple(f.shape) for f in feats], SCALES, 7, 7, 0, True)
    bad, _, _ = HA.roi_align_ref(feats, rois, l2, g2, 7, 7)
    assert _worst(bad, r, b) > 1.0


def test_roi_align_rejects_a_batch_index_off_by_one():
    feats, rois = _pyramid(), _rois()
    r, b, _, _ = _fwd(feats, rois)
    r2 = rois.clone()
    r2[5, 0] = 1 - r2[5, 0]
    assert _worst(_oracle_fwd(feats, r2), r, b) > 1.0


def _bwd(feats, rois, gout, finest=8):
    shapes = [tuple(f.shape) for f in feats]
    lvl, geo, _ = HA.roi_setup(rois, shapes, SCALES, finest, 7, 7, 0, True)
    return HA.roi_align_bwd_ref(shapes, rois, lvl, geo, gout, 7, 7)


def _oracle_bwd(feats, rois, gout, finest=8):
    fs = [f.clone().requires_grad_(True) for f in feats]
    out = ORA.roi_align_fpn(fs, rois, 7, [1 / s for s in SCALES], finest, 0, True)
    out.backward(gout)
    return [(f.grad if f.grad is not None else torch.zeros_like(f)).permute(0, 2, 3, 1).double() for f in fs]


def test_roi_align_backward_reference_matches_the_oracle_and_rejects_a_dropped_roi():
    # 600 RoIs of image 0 on level 0: one (level, image) group of more than 512 RoIs, the size the tile-by-tile backward
    # walks in pieces
    feats, rois = _pyramid(), _rois(K=600, N=1, lo=2, hi=14)
    g = torch.Generator().manual_seed(3)
    gout = torch.randn((rois.shape[0], 8, 7, 7), generator=g)
    refs = _bwd(feats, rois, gout)
    orc = _oracle_bwd(feats, rois, gout)
    lvl = ORA.map_roi_levels(rois, 3, 8)
    assert int(((lvl == 0) & (rois[:, 0] == 0)).sum()) > 512
    for (r, S, S4), o in zip(refs, orc):
        assert _worst(o, r, HA.bound(r, S, 0.0, HA.GAMMA_ROI, HA.POS_ERR * S4)) <= 0.25
        assert torch.equal(o == 0, r == 0)             # exact zeros where no sample lands
    # one RoI of a cold tile dropped from the level-0 gradient
    k = int(((lvl == 0)).nonzero()[-1])
    g2 = gout.clone()
    g2[k] = 0
    bad = _oracle_bwd(feats, rois, g2)[0]
    r, S, S4 = refs[0]
    assert _worst(bad, r, HA.bound(r, S, HA.RHO, HA.GAMMA_ROI, HA.POS_ERR * S4)) > 1.0


def test_roi_align_backward_rejects_a_contribution_in_the_next_channel_chunk():
    feats = _pyramid(C=512, sizes=((12, 12),), N=1)
    rois = _rois(K=6, N=1, W=40, H=40, lo=4, hi=20)
    g = torch.Generator().manual_seed(4)
    gout = torch.randn((6, 512, 7, 7), generator=g)
    (r, S, S4), = HA.roi_align_bwd_ref([tuple(feats[0].shape)], rois, *HA.roi_setup(
        rois, [tuple(feats[0].shape)], (0.25,), 8, 7, 7, 0, True)[:2], gout, 7, 7)
    b = HA.bound(r, S, HA.RHO, HA.GAMMA_ROI, HA.POS_ERR * S4)
    assert _worst(HA.bf16(r), r, b) <= 1.0
    g2 = gout.clone()
    g2[2, 256:] = gout[2, :256]          # RoI 2's first chunk added again into the second one
    (bad, _, _), = HA.roi_align_bwd_ref([tuple(feats[0].shape)], rois, *HA.roi_setup(
        rois, [tuple(feats[0].shape)], (0.25,), 8, 7, 7, 0, True)[:2], g2, 7, 7)
    assert _worst(HA.bf16(bad), r, b) > 1.0


def test_roi_align_backward_rejects_an_unwritten_ragged_edge_tile():
    feats, rois = _pyramid(sizes=((13, 21),), N=1), _rois(K=30, N=1, W=84, H=52, lo=8, hi=60)
    g = torch.Generator().manual_seed(5)
    gout = torch.randn((30, 8, 7, 7), generator=g)
    shapes = [tuple(feats[0].shape)]
    lvl, geo, _ = HA.roi_setup(rois, shapes, (0.25,), 8, 7, 7, 0, True)
    (r, S, S4), = HA.roi_align_bwd_ref(shapes, rois, lvl, geo, gout, 7, 7)
    b = HA.bound(r, S, HA.RHO, HA.GAMMA_ROI, HA.POS_ERR * S4)
    o = HA.bf16(r)
    assert _worst(o, r, b) <= 1.0
    bad = o.clone()
    bad[:, 8:, 16:] = 0                  # the last (partial) 8 x 8 tile never written (torch.empty: here zeros)
    assert bool((r[:, 8:, 16:] != 0).any())
    assert _worst(bad, r, b) > 1.0


def test_roi_order_check_accepts_a_stable_sort_and_rejects_a_swap():
    rois = _rois(K=300, N=2, W=1024, H=512, lo=8, hi=400)
    cands = HA.roi_order_expect(rois, 2, 4, 56)
    keys, grp = cands[0]
    order = torch.sort(keys * 4096 + torch.arange(300), stable=True)[1].int()
    rng = torch.searchsorted(grp[order.long()], torch.arange(9)).int()
    ok, lvl, _ = HA.check_order(rois, 2, 4, 56, order, rng)
    assert ok and torch.equal(lvl, ORA.map_roi_levels(rois, 4, 56))
    bad = order.clone()
    i = int((keys[order.long()][1:] != keys[order.long()][:-1]).nonzero()[0])
    bad[i], bad[i + 1] = order[i + 1], order[i]
    assert not HA.check_order(rois, 2, 4, 56, bad, rng)[0]
    rng2 = rng.clone()
    rng2[1] += 1
    assert not HA.check_order(rois, 2, 4, 56, order, rng2)[0]


# ---------------------------------------------------------------------------------------------------- loss references
def _rpn_case(seed=0, B=4, A=3, Cy=16, sizes=((8, 12), (4, 6))):
    g = torch.Generator().manual_seed(seed)
    ys = [torch.randn((B, Cy) + s, generator=g).to(torch.bfloat16) for s in sizes]
    At = sum(h * w for h, w in sizes) * A
    labels = torch.randint(-1, 2, (B, At), generator=g)
    labels[0, :5] = HA.IGNORE_INDEX
    label_w = torch.rand((B, At), generator=g) + 0.5
    bbox_t = torch.randn((B, At, 4), generator=g)
    bbox_w = (torch.rand((B, At, 4), generator=g) > 0.7).float()
    return ys, A, (labels, label_w, bbox_t, bbox_w)


def _rpn_oracle(ys, A, targets, avg, lam, w_box=1.0):
    labels, label_w, bbox_t, bbox_w = targets
    X, D = HA.rpn_flatten(ys, A)
    total, ce, js = OL.ce_jsd(X.float().reshape(-1, 1), labels.reshape(-1).long(), label_w.reshape(-1), avg, True, 1.0, lam)
    # oracle rows: view 1 first (images [0, B/2)), then view 2 in the same order
    l1 = OL.l1_view1(D.float().reshape(-1, 4), bbox_t.reshape(-1, 4), bbox_w.reshape(-1, 4), avg, loss_weight=w_box)
    return torch.stack([total, ce, js, l1]).double()


def test_rpn_loss_reference_matches_the_oracle():
    ys, A, tg = _rpn_case()
    vals, S, named = HA.rpn_loss_expect(ys, A, tg, 37.0, 1.0, 0.1, 1.0)
    o = _rpn_oracle(ys, A, tg, 37.0, 0.1)
    assert _worst(o, vals, HA.bound(vals, S, 0.0, 2.0 ** -12, named)) <= 1.0


def test_rpn_loss_rejects_a_missing_view2_jsd_term_and_avg_factor_on_jsd():
    ys, A, tg = _rpn_case()
    avg, lam = 37.0, 10.0
    vals, S, named = HA.rpn_loss_expect(ys, A, tg, avg, 1.0, lam, 1.0)
    b = HA.bound(vals, S, 0.0, HA.GAMMA_LOSS, named)
    X, _ = HA.rpn_flatten(ys, A)
    B2 = X.shape[0] // 2
    p1, p2 = torch.sigmoid(X[:B2]), torch.sigmoid(X[B2:])
    m = (p1 + p2) / 2
    kl1 = p1 * torch.log(p1 / m) + (1 - p1) * torch.log((1 - p1) / (1 - m))
    bad = vals.clone()
    bad[2] = lam / avg * (kl1 / 2).sum()            # the view-2 KL term missing
    bad[0] = bad[1] + bad[2]
    assert _worst(bad, vals, b) > 1.0
    bad2 = vals.clone()
    bad2[2] = vals[2] / avg                         # avg_factor applied twice to the JSD
    bad2[0] = bad2[1] + bad2[2]
    assert _worst(bad2, vals, b) > 1.0


def test_rpn_grad_rejects_a_weighted_ignore_label_and_a_nonzero_pad_channel():
    ys, A, tg = _rpn_case()
    labels, label_w, bbox_t, bbox_w = tg
    refs = HA.rpn_grad_expect(ys, A, tg, 37.0, 1.0, 10.0, 1.0, 1.0, 1.0)
    (r, S, E) = refs[0]
    b = HA.bound(r, S, HA.RHO, HA.GAMMA_LOSS, E)
    assert _worst(HA.bf16(r), r, b) <= 1.0
    # the ignore label of image 0, anchors 0..4 (pixel 0 / 1) given its weight as if it were background
    lab2 = labels.clone()
    lab2[0, :5] = 1
    bad = HA.rpn_grad_expect(ys, A, (lab2, label_w, bbox_t, bbox_w), 37.0, 1.0, 10.0, 1.0, 1.0, 1.0)[0][0]
    assert _worst(HA.bf16(bad), r, b) > 1.0
    pad = HA.bf16(r).clone()
    pad[1, 2, 3, 15] = 1e-3
    assert _worst(pad, r, b) > 1.0


def test_ce_jsd_reference_matches_the_oracle_both_modes():
    g = torch.Generator().manual_seed(6)
    for mode, C in ((1, 9), (0, 1)):
        x = torch.randn((64, C), generator=g) * 3
        lab = torch.randint(0, max(C, 2), (64,), generator=g)
        lab[3] = HA.IGNORE_INDEX
        w = torch.rand(64, generator=g)
        vals, S, named, (r, Sg, E) = HA.ce_jsd_expect(x, lab, w, mode, 13.0, 1.0, 10.0, 1.0)
        xo = x.double().requires_grad_(True)
        tot, ce, js = OL.ce_jsd(xo, lab, w.double(), 13.0, mode == 0, 1.0, 10.0)
        tot.backward()
        o = torch.stack([tot, ce, js]).detach()
        # (the oracle's BCE runs in fp32: its weights and one-hot targets are cast with .float())
        assert _worst(o, vals, HA.bound(vals, S, 0.0, 2.0 ** -20, named)) <= 1.0
        assert _worst(xo.grad, r, HA.bound(r, Sg, 0.0, 2.0 ** -20, E)) <= 1.0


def test_supcon_reference_matches_the_oracle_and_rejects_self_in_the_positive_mask():
    g = torch.Generator().manual_seed(7)
    B, ori, rp = 40, 16, 4
    feats = torch.randn((B, 16), generator=g)
    labels = torch.randint(0, 4, (B - 3,), generator=g)
    loss, S = HA.supcon_expect(feats, labels, ori, rp, 0.07, 2, 0.5)
    x = feats.double().requires_grad_(True)
    ref = OL.supcon(x, labels, ori, rp, temper=0.07, min_samples=2, loss_weight=0.5)
    ref.backward()
    assert _worst(ref.detach().view(1), loss.view(1), HA.bound(loss.view(1), S.view(1), 0.0, 2.0 ** -30)) <= 1.0
    _, _, r, Sx = HA.supcon_expect(feats, labels, ori, rp, 0.07, 2, 0.5, 1.0)
    b = HA.bound(r, Sx, 0.0, HA.GAMMA_LOSS)
    assert _worst(x.grad, r, b) <= 1e-2                 # (two fp64 evaluations)
    # the positive mask including self: a different loss and gradient
    xs = feats.double().requires_grad_(True)
    f = torch.nn.functional.normalize(xs, dim=1)
    lab = torch.cat([labels, labels[-1:].repeat(3)])
    L = f @ f.t() / 0.07
    L = L - L.max(1, keepdim=True)[0].detach()
    eye = torch.eye(B, dtype=torch.bool)
    fg = lab != lab.max()
    P = ((lab.view(-1, 1) == lab.view(1, -1)) & fg.view(-1, 1) & fg.view(1, -1)).double()   # (no ~eye)
    tw = OL.twin_index(B, ori, rp)
    twin = torch.zeros(B, B, dtype=torch.bool)
    twin[torch.arange(B)[tw >= 0], tw[tw >= 0]] = True
    P = torch.maximum(P, (twin & (~fg).view(-1, 1) & (~fg).view(1, -1)).double())
    lp = L - torch.log((torch.exp(L) * (~eye).double()).sum(1, keepdim=True))
    bad = 0.5 * (-((P * lp).sum(1) / (P.sum(1) + 1e-8))).mean()
    bad.backward()
    assert _worst(xs.grad, r, b) > 1.0
    assert _worst(bad.detach().view(1), loss.view(1), HA.bound(loss.view(1), S.view(1), 0.0, HA.GAMMA_LOSS)) > 1.0
    # min_samples: at most that many foreground rows give 0
    z, _ = HA.supcon_expect(feats, torch.full((B,), 3), ori, rp, 0.07, 2, 0.5)
    assert float(z) == 0.0


def test_roi_reg_rejects_the_neighbouring_class_columns():
    g = torch.Generator().manual_seed(8)
    K, C = 32, 8
    pred = torch.randn((K, 4 * C), generator=g).to(torch.bfloat16)
    lab = torch.randint(0, C + 1, (K,), generator=g)
    t, w = torch.randn((K, 4), generator=g), torch.rand((K, 4), generator=g)
    for beta in (1.0, 0.0):
        r, S = HA.roi_reg_grad_expect(pred, lab, t, w, C, 20, beta, 11.0, 1.0, 1.0)
        b = HA.bound(r, S, HA.RHO, HA.GAMMA_LOSS)
        p = pred.double().requires_grad_(True)
        pos = (torch.arange(K) < 20) & (lab < C)
        cols = lab.clamp_max(C - 1).view(-1, 1) * 4 + torch.arange(4)
        loss_fn = OL.smooth_l1_view1 if beta > 0 else OL.l1_view1
        kw = dict(beta=beta) if beta > 0 else {}
        loss = loss_fn(p.gather(1, cols)[pos], t.double()[pos], w.double()[pos], 11.0, num_views=1, **kw)
        loss.backward()
        ref_loss, S_l = HA.roi_reg_expect(pred, lab, t, w, C, 20, beta, 11.0, 1.0)
        assert _worst(loss.detach().view(1), ref_loss.view(1), HA.bound(ref_loss.view(1), S_l.view(1), 0.0, 2 ** -30)) <= 1
        assert _worst(HA.bf16(p.grad), r, b) <= 1.0
        lab2 = torch.where(pos, (lab + 1) % C, lab)        # the gradient taken from (and written to) the next class
        bad, _ = HA.roi_reg_grad_expect(pred, lab2, t, w, C, 20, beta, 11.0, 1.0, 1.0)
        assert _worst(HA.bf16(bad), r, b) > 1.0


@pytest.mark.parametrize('plant', [None, 'permutation not undone', 'second call dropped'])
def test_linear_param_check_follows_the_permutation_and_sums_the_calls(plant):
    """check_linear_params: a permuted first FC (hip_ops._FcWeightPermute, columns p C + c) and a linear called twice"""
    g = torch.Generator().manual_seed(10)
    K, O, C, P = 24, 8, 16, 4
    fc, fc2 = torch.nn.Linear(C * P, O), torch.nn.Linear(O, O)
    x = torch.randn((K, P * C), generator=g).to(torch.bfloat16)          # features in (p, c) order
    gy = torch.randn((K, O), generator=g).to(torch.bfloat16)
    y = torch.randn((K, O), generator=g).to(torch.bfloat16)
    x2a, x2b = (torch.randn((K, O), generator=g).to(torch.bfloat16) for _ in range(2))
    A = HA.Auditor()
    A._linear_ref((fc.weight, (C, P)), (fc.bias, None), x, y, gy)
    A._linear_ref((fc2.weight, None), None, x2a, None, gy)
    A._linear_ref((fc2.weight, None), None, x2b, None, gy)
    gm = gy.double() * (y > 0)
    dperm = (gm.t() @ x.double()).float().to(torch.bfloat16)           # the GEMM's bf16 gradient in the permuted layout
    fc.weight.grad = dperm.float().view(O, P, C).permute(0, 2, 1).reshape(O, C * P).contiguous()
    fc.bias.grad = gm.sum(0).float().to(torch.bfloat16).float()
    parts = [(gy.double().t() @ xx.double()).to(torch.bfloat16) for xx in (x2a, x2b)]
    fc2.weight.grad = (parts[0] + parts[1]).float()
    if plant == 'permutation not undone':
        fc.weight.grad = dperm.float()
    elif plant == 'second call dropped':
        fc2.weight.grad = parts[0].float()
    named = [('roi_head.fc.weight', fc.weight), ('roi_head.fc.bias', fc.bias), ('roi_head.fc2.weight', fc2.weight)]
    assert A.check_linear_params(named) == {n for n, _ in named}
    assert (not A.failures) == (plant is None), A.failures
    B = HA.Auditor()                    # a trainable parameter no captured call produced: reported
    B.check_linear_params([('roi_head.fc2.bias', fc2.bias)])
    assert B.failures


def test_top1_takes_the_first_maximum_of_tied_logits():
    s = torch.tensor([[1.0, 3.0, 3.0], [5.0, 1.0, 0.0], [0.0, 0.0, 2.0], [1.0, 3.0, 3.0]])
    assert HA.top1_first(s, torch.tensor([1, 0, 1, 2])) == (2, 2)


def test_parse_losses_rejects_a_loss_missing_from_the_total():
    A = HA.Auditor()
    vals = [torch.tensor([v]) for v in (0.7, 0.2, 0.05, 1.3, 55.0)]
    name_of, mask = (0, 0, 1, 2, 3), 0b0111       # name 3 (an accuracy) not in the total
    s = [0.7 + 0.2, 0.05, 1.3, 55.0]
    good = torch.tensor(s + [sum(s[:3])])
    A._check_parse(name_of, 4, mask, vals, (good[-1], good))
    assert not A.failures
    bad = torch.tensor(s + [s[0] + s[2]])           # the second loss left out
    A._check_parse(name_of, 4, mask, vals, (bad[-1], bad))
    assert A.failures


def test_sgd_check_rejects_a_tensor_without_weight_decay():
    g = torch.Generator().manual_seed(9)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 17)]
    frozen = torch.nn.Parameter(torch.randn(3, generator=g), requires_grad=False)
    model = torch.nn.Module()
    for i, p in enumerate(ps + [frozen]):
        model.register_parameter('p%d' % i, p)
    for step in range(2):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        for drop_wd in (False, True):
            opt = torch.optim.SGD(ps, lr=0.02, momentum=0.9, weight_decay=1e-2)
            if step:
                for p in ps:
                    opt.state[p]['momentum_buffer'] = torch.randn(p.shape, generator=g)
            A = HA.Auditor()
            snap = A._sgd_snapshot(opt, model)
            if drop_wd:                 # one tensor updated without weight decay
                ref = torch.optim.SGD([ps[1]], lr=0.02, momentum=0.9, weight_decay=0.0)
                ref.state[ps[1]] = opt.state[ps[1]]
                with torch.no_grad():
                    opt2 = torch.optim.SGD([ps[0]], lr=0.02, momentum=0.9, weight_decay=1e-2)
                    opt2.state[ps[0]] = opt.state[ps[0]]
                    opt2.step()
                    ref.step()
                opt.state[ps[0]], opt.state[ps[1]] = opt2.state[ps[0]], ref.state[ps[1]]
            else:
                opt.step()
            A._check_sgd(opt, snap, model)
            assert bool(A.failures) == drop_wd, A.failures
            with torch.no_grad():
                for p, (_, p0, _, _, _) in zip(ps, snap[0]):
                    p.copy_(p0)



def test_sgd_fall_back_to_torch_is_not_recorded_as_the_kernel():
    p = torch.nn.Parameter(torch.ones(4))
    p.grad = torch.ones(4)
    opt = torch.optim.SGD([p], lr=0.1, momentum=0.9)
    A = HA.Auditor()
    snap = A._sgd_snapshot(opt, None)
    opt.step()
    A._check_sgd(opt, snap, None, fused=False)
    assert not A.failures and 'sgd_multi_kernel' not in A.kernels
    assert A.info['sgd_steps'] == [('first step', 1, 'fall-back')]

# ------------------------------------------------------------------------------------------------- GPU audited steps
# carved-out RoIAlign elements per element checked: the elements of RoIs whose launch matched only the other side of a
# choice within fp32 rounding of its threshold (level, adaptive sample count, out-of-map drop), where the two sides differ
BORDERLINE_CAP = 1e-4

# the launches every workload's audited step reaches
_COMMON = {
    'roi_align_bwd_tiles_kernel', 'roi_tile_box_kernel', 'roi_order_rank_kernel', 'roi_align_fwd_rows_kernel<unsigned short>',
    'sm_kernel<false>', 'sm_kernel<true>', 'cls_fin_kernel', 'roi_reg_acc_fwd_kernel', 'roi_reg_bwd_kernel',
    'parse_losses_kernel', 'fc_weight_permute_kernel', 'sgd_multi_kernel', 'rpn_loss_fin_kernel',
    'supcon_prep_kernel', 'supcon_tile_kernel<false>', 'supcon_tile_kernel<true>', 'supcon_fin_kernel',
    'supcon_bwd_fin_kernel', 'rpn_loss_fwd_kernel<3>', 'rpn_loss_bwd_kernel<true, 3>',
}
EXPECTED = {'r50_fpn': set(_COMMON), 'r50_fpn_multiscale': set(_COMMON),
            # (15 anchors per pixel on one level: the RPN loss takes the per-level CE + JSD launches, sigmoid rows)
            'r101_dc5': _COMMON - {'rpn_loss_fwd_kernel<3>', 'rpn_loss_bwd_kernel<true, 3>', 'rpn_loss_fin_kernel'} |
            {'sig_kernel<false>', 'sig_kernel<true>'}}
WRAPPERS = {'linear_bias_grad', '_RoIAlignFPN.forward', '_RoIAlignFPN.backward', '_RpnLoss.forward', '_RpnLoss.backward', '_CeJsd.forward',
            '_CeJsd.backward', '_RoiRegAcc.forward', '_RoiRegAcc.backward', '_SupCon.forward', '_SupCon.backward',
            '_ParseLosses.forward', '_CastAll.forward', '_CastAll.backward', '_FcWeightPermute.forward',
            '_FcWeightPermute.backward', 'FusedSGD.step'}
WRAPPERS_OF = {'r50_fpn': WRAPPERS, 'r50_fpn_multiscale': WRAPPERS,
               'r101_dc5': WRAPPERS - {'_RpnLoss.forward', '_RpnLoss.backward'}}


def _head_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size, key):
    A = HA.Auditor()
    checked = []

    def on_end_backward(det):
        checked.append(A.check_linear_params(list(det.named_parameters())))

    out, det, wall = audited_step(dev, monkeypatch, cfg_path, batch, H, W, boxes, classes, box_size,
                                  lambda mp, det: A.install(mp, det), on_end_backward=on_end_backward,
                                  before_step1=lambda mp, det: A.install_sgd(mp, det))
    A.print_table('%s (audited step %.1f s)' % (key, wall))
    print('worst err / bound: %.4f' % A.worst())
    print('audited instantiations:', sorted(A.kernels))
    print('roi head parameters checked: %d' % len(checked[-1] if checked else ()))
    assert not A.failures, A.failures[:10]
    missing = WRAPPERS_OF[key] - set(A.wrappers)
    assert not missing, missing
    assert [s[0::2] for s in A.info['sgd_steps']] == [('first step', 'fused'), ('later step', 'fused')], A.info['sgd_steps']
    # every trainable parameter: its gradient checked here (the RoI head) or by tests/test_conv_audit.py
    trainable = {n for n, p in det.named_parameters() if p.requires_grad}
    roi = {n for n in trainable if n.startswith('roi_head.')}
    assert roi and checked and checked[-1] == roi, sorted(roi ^ set(checked[-1] if checked else ()))[:10]
    rest = {n for n in trainable - roi if not n.startswith(('backbone.', 'neck.', 'rpn_head.'))}
    assert not rest, sorted(rest)[:10]
    assert not A.info['sgd_missed'], A.info['sgd_missed'][:10]
    for fam, (carved, total) in A.borderline.items():
        assert carved <= BORDERLINE_CAP * max(total, 1), (fam, carved, total)
    assert A.kernels == EXPECTED[key], (sorted(A.kernels - EXPECTED[key]), sorted(EXPECTED[key] - A.kernels))
    return A


@pytest.mark.gpu
def test_head_audit_config1_r50_fpn_bench_step(dev, monkeypatch):
    """configs[1] as bench.py builds it: 4 images x 2 views at 1024 x 2048, bf16, the second step audited"""
    _head_step(dev, monkeypatch, R50_CFG, 4, 1024, 2048, 20, 8, (24, 400), 'r50_fpn')


@pytest.mark.gpu
def test_head_audit_config3_r101_dc5(dev, monkeypatch):
    """configs[3]: R101-DC5 at 736 x 1280 - one 2048-channel map: eight channel chunks per RoI"""
    _head_step(dev, monkeypatch, DC5_CFG, 2, 736, 1280, 12, 7, (24, 300), 'r101_dc5')


@pytest.mark.gpu
def test_head_audit_multiscale_800x1600(dev, monkeypatch):
    """the ragged multi-scale shape of tests/test_conv_audit.py: partial tiles of every level"""
    _head_step(dev, monkeypatch, R50_CFG, 2, 800, 1600, 12, 8, (24, 300), 'r50_fpn_multiscale')


@pytest.mark.gpu
@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float32])
def test_head_audit_roi_align_stress(dev, monkeypatch, dt):
    """the bench pyramid (P2 256 x 512 ... P5, 8 images, 256 channels) with clustered RoIs: a (level, image) group of more than
    512 RoIs (the tile-by-tile backward walks it in pieces) and bins wider than 32 pixels (the rows forward's per-sample
    fallback); fp32 maps take roi_align_fwd_rows_kernel<float> and the atomic backward"""
    from oadg_amd import hip_ops
    g = torch.Generator(device='cpu').manual_seed(11)
    N, C = 8, 256
    feats = [(torch.randn((N, C, 256 // 2 ** l, 512 // 2 ** l), generator=g)).to(dev, dt)
             .contiguous(memory_format=torch.channels_last).requires_grad_(True) for l in range(4)]
    K = 4096
    small = 700                                       # image 0, level 0: centred on one object
    cx = 300 + torch.randn(small, generator=g) * 20
    cy = 200 + torch.randn(small, generator=g) * 20
    sz = 16 + torch.rand(small, generator=g) * 60
    big = 8                                           # level 3 with bins > 32 px at 1/32: boxes wider than 7 * 32 * 32 px
    bx = torch.rand(big, generator=g) * 200
    bs = torch.full((big,), 7500.0)
    rest = K - small - big
    rx, ry = torch.rand(rest, generator=g) * 1900, torch.rand(rest, generator=g) * 900
    rs = 8 + torch.rand(rest, generator=g) * 500
    rois = torch.cat([
        torch.stack([torch.zeros(small), cx - sz / 2, cy - sz / 2, cx + sz / 2, cy + sz / 2], 1),
        torch.stack([torch.full((big,), 3.0), bx - 3000, bx * 0.2, bx - 3000 + bs, bx * 0.2 + bs * 0.3], 1),
        torch.stack([torch.randint(0, N, (rest,), generator=g).float(), rx, ry, rx + rs, ry + rs * 0.7], 1)]).to(dev)
    A = HA.Auditor().install(monkeypatch, sgd=False)
    out = hip_ops.roi_align_fpn(feats, rois, 7, [0.25, 0.125, 0.0625, 0.03125], 56, 0, True)
    out.backward(torch.randn(out.shape, generator=g).to(dev, dt))
    torch.cuda.synchronize()
    monkeypatch.undo()
    A.print_table('RoIAlign stress %s' % dt)
    assert not A.failures, A.failures[:10]
    assert A.info['max_group'] > 512 and A.info['max_bin'] > 32, A.info
    for fam, (carved, total) in A.borderline.items():
        assert carved <= BORDERLINE_CAP * max(total, 1), (fam, carved, total)
    want = {'roi_align_fwd_rows_kernel<unsigned short>', 'roi_align_bwd_tiles_kernel', 'roi_tile_box_kernel',
            'roi_order_rank_kernel'} if dt == torch.bfloat16 else {'roi_align_fwd_rows_kernel<float>', 'roi_align_bwd_kernel',
                                                                  'roi_order_rank_kernel'}
    assert A.kernels == want, sorted(A.kernels)
