"""Stress launches of the loss kernels (csrc/cls_loss.hip, csrc/supcon.hip) at saturated operands: the regime of a trained
or briefly diverging detector, which the audited steps (step 2 of a freshly initialised model) and the N(0, 3) logits of
tests/test_hip_losses.py never reach.

The GPU tests drive the Python entry points that tests/head_audit.py wraps (hip_ops.ce_jsd_loss, rpn_loss, roi_reg_acc,
supcon_loss, BaseDetector._parse_losses) with the auditor installed: every launch is recomputed in float64 from the operands
it received and compared element by element under the auditor's own bound

    |o - r| <= RHO |r| + GAMMA_LOSS S + ALPHA + named

and every test prints the auditor's table (worst err / bound per kernel).  On top of that: every output is finite wherever
the float64 reference is, and for the softmax rows the cross-entropy of the rows with the largest gap between the row
maximum and the label's logit is checked ONE ROW AT A TIME (a weight vector that is zero except for that row, lambda = 0), so
that the sum over the rows cannot cover a wrong row.

The CPU self-tests (not ``gpu``) feed float32 restatements of the softmax forward and of the gradient through the same
checks: they show what the checks reject and what they accept.
"""
import numpy as np
import pytest
import torch

import head_audit as HA

GAPS = (20, 60, 86, 88, 95, 103, 104, 120, 300)
SM_HALF = 133                         # 4 k + 1: the last block of four waves holds one pair
SM_C = (2, 9, 64, 65, 81, 256)        # the 64-lane chunk edges and the kernel's maximum
SIG_SCALES = (1, 5, 10, 17, 30, 60, 90, 200)
SIG_EXACT = (0.0, 16.6, -16.6, 17.4, -17.4, 88.0, -88.0, 104.0, -104.0)
SIG_LABELS = (0, 1, -1, HA.IGNORE_INDEX)


# ------------------------------------------------------------------------------------------------------------ inputs
def softmax_case(C, gaps=GAPS, seed=0):
    """(logits [2 half, C] fp32, labels [half], weights [half], {row: gap}) on the CPU: N(0, 3) background plus the rows
    the module docstring names.  The gap rows hold their label in the first 64-lane chunk and the winning class in the last
    one (C > 64); every planted value is a small integer or half-integer, so the gap is exact in fp32."""
    g = torch.Generator().manual_seed(1000 * seed + C)
    half = SM_HALF
    x = torch.randn((2 * half, C), generator=g) * 3
    lab = torch.randint(0, C, (half,), generator=g)
    w = torch.rand(half, generator=g) + 0.5
    lo, hi = (3 if C > 64 else 0), C - 1
    planted = {}

    def gap_row(r, gp, both):
        for v in ((r, r + half) if both else (r,)):
            top = float(x[v].max().ceil()) + 2.0
            x[v, hi] = top
            x[v, lo] = top - gp
        lab[r] = lo
        planted[r] = gp

    r = 0
    for gp in gaps:                                  # view 2: background / the same gap
        gap_row(r, gp, False)
        gap_row(r + 1, gp, True)
        r += 2
    gap_row(half - 1, 95, False)                     # the lone pair of the last block
    for s in (50.0, 200.0):                          # both views saturated towards the label
        for _ in range(2):
            x[r, lab[r]] += s
            x[r + half, lab[r]] += s
            r += 1
    for s in (60.0, 200.0):                          # the views saturated towards different classes: JSD near ln 2
        for _ in range(2):
            a = int(lab[r])
            b = (a + 64) % C if C > 64 else (a + 1) % C
            x[r, a] += s
            x[r + half, b] += s
            r += 1
    x[r] = 1.5                                       # all logits equal, in both views / in view 1
    x[r + half] = -2.0
    x[r + 1] = 0.0
    r += 2
    for bad in (HA.IGNORE_INDEX, -1, C):             # invalid labels
        lab[r] = bad
        lab[r + 1] = bad
        x[r + 1, hi] += 90.0
        r += 2
    w[r:r + 4] = 0.0                                 # valid rows without weight, one of them saturated
    x[r, (int(lab[r]) + 1) % C] += 100.0
    w[half - 2] = 0.0
    return x, lab, w, planted


def sigmoid_case(n, seed=0):
    """(x1 [n], x2 [n], labels [n]) on the CPU: the exact values paired across the views in all sign combinations, under
    every label kind, then blocks of N(0, s) logits"""
    g = torch.Generator().manual_seed(77 + seed)
    pairs = [(a, b, l) for a in SIG_EXACT for b in SIG_EXACT for l in SIG_LABELS]
    assert n >= len(pairs) + 8 * len(SIG_SCALES)
    x1, x2 = torch.empty(n), torch.empty(n)
    blk = -(-n // len(SIG_SCALES))
    for i, s in enumerate(SIG_SCALES):
        m = min(blk, n - i * blk)
        if m > 0:
            x1[i * blk:i * blk + m] = torch.randn(m, generator=g) * s
            x2[i * blk:i * blk + m] = torch.randn(m, generator=g) * s
    lab = torch.tensor(SIG_LABELS)[torch.randint(0, 4, (n,), generator=g)]
    # (half of the random pairs correlated: both views saturated to the same side)
    same = torch.rand(n, generator=g) < 0.5
    x2 = torch.where(same, x1 + torch.randn(n, generator=g), x2)
    k = len(pairs)
    x1[:k] = torch.tensor([p[0] for p in pairs])
    x2[:k] = torch.tensor([p[1] for p in pairs])
    lab[:k] = torch.tensor([p[2] for p in pairs])
    return x1, x2, lab.long()


# ------------------------------------------------------------------------------------------------------------ checks
def check_finite(A, kernel, o, ref):
    """every output finite wherever the float64 reference is"""
    ok = bool(torch.isfinite(o.double())[torch.isfinite(ref)].all())
    A.exact(kernel, tuple(o.shape), ok, check='finite where the reference is', launched=False)


def check_softmax_forward(A, run, x, lab, w, avg, lw, lam, kernel='sm_kernel<false>'):
    """``run(x, labels, weights, lam) -> parts [3]`` (total, ce, lambda jsd) of the forward under test: the whole launch, then
    each of the up-to-16 rows with the largest gap on its own - in the same launch under a weight vector that is zero except
    for that row (lambda = 0), and as a launch of that one pair.  Returns {gap: [(ce under the one-row weights, fp64 ce, its
    err / bound, ce of the pair alone, its err / bound)]}."""
    vals, S, named = HA.ce_jsd_expect(x, lab, w, 1, avg, lw, lam)
    o = run(x, lab, w, lam).double().cpu()
    A.record(kernel, tuple(x.shape), o, vals.cpu(), HA.bound(vals, S, 0.0, HA.GAMMA_LOSS, named).cpu(), check='parts',
             launched=False)
    check_finite(A, kernel, o, vals.cpu())
    h, C = x.shape[0] // 2, x.shape[1]
    valid = (lab >= 0) & (lab < C)
    x1 = x[:h].double()
    gap = x1.max(1)[0] - x1.gather(1, lab.clamp(0, C - 1).view(-1, 1)).view(-1)
    gap = torch.where(valid, gap, torch.full_like(gap, -1.0))
    rows = torch.argsort(gap, descending=True, stable=True)[:16]
    rows = [int(r) for r in rows if bool(valid[r])]
    seen = {}
    for r in rows:
        one = torch.zeros_like(w)
        one[r] = 1.0
        v1, S1, n1 = HA.ce_jsd_expect(x, lab, one, 1, avg, lw, 0.0)
        o1 = run(x, lab, one, 0.0).double().cpu()
        b1 = HA.bound(v1, S1, 0.0, HA.GAMMA_LOSS, n1).cpu()
        rt = A.record(kernel, tuple(x.shape), o1, v1.cpu(), b1, check='one row: parts', launched=False)
        check_finite(A, kernel, o1, v1.cpu())
        xa, la, wa = x[[r, r + h]].contiguous(), lab[r:r + 1].contiguous(), one[r:r + 1].contiguous()
        v2, S2, n2 = HA.ce_jsd_expect(xa, la, wa, 1, avg, lw, lam)
        o2 = run(xa, la, wa, lam).double().cpu()
        rt2 = A.record(kernel, (2, C), o2, v2.cpu(), HA.bound(v2, S2, 0.0, HA.GAMMA_LOSS, n2).cpu(), check='one pair: parts',
                       launched=False)
        check_finite(A, kernel, o2, v2.cpu())
        seen.setdefault(round(float(gap[r]), 3), []).append((float(o1[1]), float(v1[1]), rt, float(o2[1]), rt2))
    return seen


def print_gaps(gaps):
    print('rows on their own, gap: (ce under one-row weights, fp64 ce, err / bound; ce of the pair alone, err / bound)')
    for gp in sorted(gaps):
        print('  %8.3f: %s' % (gp, ', '.join('(%.7g, %.7g, %.3g; %.7g, %.3g)' % t for t in gaps[gp])))


def finish(A, title, gaps=None):
    A.print_table(title)
    if gaps:
        print_gaps(gaps)
    assert not A.failures, A.failures


# ------------------------------------------------------------------------------------ float32 restatements (CPU self-tests)
def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def softmax_forward_f32(x, lab, w, avg, lw, lam, through_probability):
    """sm_kernel<false> + cls_fin_kernel in torch float32 (per-row terms summed in float64 like the kernel's partials):
    ``through_probability`` = the CE as -log(exp(x - m) / s), else (m - x) + log s"""
    x = x.float()
    h, C = x.shape[0] // 2, x.shape[1]
    P, D, Ssum = [], [], []
    for v in (x[:h], x[h:]):
        d = v - v.max(1, keepdim=True)[0]
        a = torch.exp(d)
        s = a.sum(1, keepdim=True)
        P.append(a / s)
        D.append(d)
        Ssum.append(s)
    valid = (lab != HA.IGNORE_INDEX) & (lab >= 0) & (lab < C)
    li = lab.clamp(0, C - 1).view(-1, 1)
    wv = torch.where(valid, w.float(), torch.zeros(h))
    if through_probability:
        nll = -torch.log(P[0].gather(1, li).view(-1))
    else:
        nll = torch.log(Ssum[0].view(-1)) - D[0].gather(1, li).view(-1)
    ce = (wv * nll)[valid].double().sum()
    m = ((P[0] + P[1]) / 2.0).clamp(1e-7, 1.0)
    lm = torch.log(m)
    t = [torch.where(p > 0, p * (torch.log(p.clamp_min(1e-45)) - lm), torch.zeros_like(p)) for p in P]
    js = ((t[0] + t[1]) / 2.0).sum(1).double().sum()
    k_ce, k_jsd = _f32(lw) / _f32(avg), _f32(lam) / _f32(avg)
    cev, jsv = ce.float() * k_ce, js.float() * k_jsd
    return torch.stack([cev + jsv, cev, jsv])


def sigmoid_grad_f32(x1, x2, lab, w, avg, lw, lam, g0, always_subtract):
    """sig_kernel<true> in torch float32; ``always_subtract`` = jsd_dterm without its ``live`` test: the -1/2 (t1 + t2) / (2 M)
    term also where M is clamped"""
    x1, x2 = x1.float(), x2.float()
    valid = (lab >= 0) & (lab != HA.IGNORE_INDEX)
    t = (valid & (lab == 0)).float()
    wv = torch.where(valid, w.float() if w is not None else torch.ones_like(t), torch.zeros_like(t))
    p1, p2 = 1.0 / (1.0 + torch.exp(-x1)), 1.0 / (1.0 + torch.exp(-x2))
    q1, q2 = 1.0 - p1, 1.0 - p2

    def dterm(t1, t2):
        mraw = (t1 + t2) / 2.0
        m = mraw.clamp(1e-7, 1.0)
        gq = 0.5 * (torch.log(t1.clamp_min(1e-45)) + 1.0 - torch.log(m))
        live = (mraw >= 1e-7) & (mraw <= 1.0)
        if always_subtract:
            live = torch.ones_like(live)
        gq = torch.where(live, gq - 0.5 * (t1 + t2) * 0.5 / m, gq)
        return torch.where(t1 > 0, gq, torch.zeros_like(gq))
    d1 = dterm(p1, p2) - dterm(q1, q2)
    d2 = dterm(p2, p1) - dterm(q2, q1)
    k_ce, k_jsd = _f32(lw) / _f32(avg), _f32(lam) / _f32(avg)
    g1 = k_ce * wv * (p1 - t) + k_jsd * p1 * (1.0 - p1) * d1
    g2 = k_jsd * p2 * (1.0 - p2) * d2
    return _f32(g0) * torch.cat([g1, g2]).view(-1, 1)


def softmax_grad_f32(x, lab, w, avg, lw, lam, g0, always_subtract):
    """sm_kernel<true> in torch float32, ``always_subtract`` as in sigmoid_grad_f32 (the two kernels share jsd_dterm)"""
    x = x.float()
    h, C = x.shape[0] // 2, x.shape[1]
    p1, p2 = (torch.exp(v - v.max(1, keepdim=True)[0]) for v in (x[:h], x[h:]))
    p1, p2 = p1 / p1.sum(1, keepdim=True), p2 / p2.sum(1, keepdim=True)
    valid = (lab != HA.IGNORE_INDEX) & (lab >= 0) & (lab < C)
    wv = torch.where(valid, w.float(), torch.zeros(h)).view(-1, 1)
    onehot = torch.zeros_like(p1).scatter_(1, lab.clamp(0, C - 1).view(-1, 1), 1.0) * valid.view(-1, 1)
    mraw = (p1 + p2) / 2.0
    m = mraw.clamp(1e-7, 1.0)
    lm = torch.log(m)
    live = (mraw >= 1e-7) & (mraw <= 1.0)
    if always_subtract:
        live = torch.ones_like(live)

    def dterm(t1, t2):
        gq = 0.5 * (torch.log(t1.clamp_min(1e-45)) + 1.0 - lm)
        gq = torch.where(live, gq - 0.5 * (t1 + t2) * 0.5 / m, gq)
        return torch.where(t1 > 0, gq, torch.zeros_like(gq))
    gd1, gd2 = dterm(p1, p2), dterm(p2, p1)
    dot1, dot2 = (p1 * gd1).sum(1, keepdim=True), (p2 * gd2).sum(1, keepdim=True)
    k_ce, k_jsd = _f32(lw) / _f32(avg), _f32(lam) / _f32(avg)
    g1 = k_ce * wv * (p1 - onehot) + k_jsd * p1 * (gd1 - dot1)
    g2 = k_jsd * p2 * (gd2 - dot2)
    return _f32(g0) * torch.cat([g1, g2])


# -------------------------------------------------------------------------------------------------------- CPU self-tests
SELF_GAPS = GAPS + (110,)


@pytest.mark.parametrize('C', [9, 81])
def test_isolated_ce_rejects_the_log_of_an_underflowing_probability(C):
    """The CE through the label's probability, -log(exp(x - m) / s), in host float32: the probability is a denormal from a
    gap of 87.3 and 0 from 104.
    * Under one-row weights EVERY isolated launch is rejected (gaps 95 and 110 among them): the rows with a gap of 104 and
      more contribute 0 * inf = NaN although their weight is 0.
    * The pair alone is rejected from a gap of 103: 1.3 denormal units, then +inf.  At 88 and 95 the denormal still holds 22 /
      12 bits; its logarithm is off by at most 1e-7 / 1.3e-4, that is 0.0001 / 0.09 of the row's bound GAMMA_LOSS * gap, and
      no check at this bound tells it from the stable form there.  (The printed table has the measured figures.)"""
    x, lab, w, planted = softmax_case(C, gaps=SELF_GAPS)
    A = HA.Auditor()
    seen = check_softmax_forward(A, lambda xx, ll, wt, lam: softmax_forward_f32(xx, ll, wt, 13.0, 1.0, lam, True), x, lab, w,
                                 13.0, 1.0, 10.0, kernel='float32 restatement, CE = -log p')
    A.print_table('planted: CE through the probability, C = %d' % C)
    print_gaps(seen)
    for gp in (88.0, 95.0, 103.0, 104.0, 110.0, 120.0, 300.0):
        assert all(not t[2] <= 1.0 for t in seen[gp]), (gp, seen[gp])
    for gp in (103.0, 104.0, 110.0, 120.0, 300.0):
        assert all(not t[4] <= 1.0 for t in seen[gp]), (gp, seen[gp])
    for gp in (104.0, 110.0, 120.0, 300.0):
        assert all(t[3] == float('inf') for t in seen[gp]), (gp, seen[gp])
    assert A.failures


@pytest.mark.parametrize('C', SM_C)
def test_isolated_ce_accepts_the_stable_form_at_every_gap(C):
    x, lab, w, planted = softmax_case(C, gaps=SELF_GAPS)
    A = HA.Auditor()
    seen = check_softmax_forward(A, lambda xx, ll, wt, lam: softmax_forward_f32(xx, ll, wt, 13.0, 1.0, lam, False), x, lab, w,
                                 13.0, 1.0, 10.0, kernel='float32 restatement, CE = (m - x) + log s')
    assert {float(g) for g in SELF_GAPS if g >= 88} <= set(seen)
    finish(A, 'stable CE, C = %d' % C, seen)


def test_gradient_check_rejects_a_jsd_term_subtracted_inside_the_clamp():
    """jsd_dterm without its ``live`` test (the -1/2 (t1 + t2) / (2 M) term applied where M = 1e-7 is the clamp).  The softmax
    rows' bound scales with the element's own probability and rejects it on every saturated row.  On the sigmoid rows the
    defect moves an element by at most lambda / avg * 1e-7 (q1 <= 2e-7 under the clamp, the term <= 1/2), while the
    expectation's named term PROB_ERR * max(p, q) * lambda / avg * (|d| + 2) is at least 4.8e-7 of the same unit: the
    auditor's bound cannot see it there, whatever the operands - the defect moves no element by more than 0.06 of its bound (printed
    below)."""
    x, lab, w, _ = softmax_case(81)
    avg, lw, lam, g0 = 13.0, 1.0, 10.0, 0.75
    _, _, _, (r, S, E) = HA.ce_jsd_expect(x, lab, w, 1, avg, lw, lam, g0)
    b = HA.bound(r, S, 0.0, HA.GAMMA_LOSS, E)
    good = HA.ratio(softmax_grad_f32(x, lab, w, avg, lw, lam, g0, False), r, b)[0]
    bad = HA.ratio(softmax_grad_f32(x, lab, w, avg, lw, lam, g0, True), r, b)[0]
    print('softmax rows: float32 restatement %.4f, live test dropped %.4g' % (good, bad))
    assert good <= 1.0 and bad > 1.0
    x1, x2, sl = sigmoid_case(4097)
    ws = torch.rand(4097, generator=torch.Generator().manual_seed(5)) + 0.5
    xs = torch.cat([x1, x2]).view(-1, 1)
    _, _, _, (r, S, E) = HA.ce_jsd_expect(xs, sl, ws, 0, 37.0, 1.0, 0.1, g0)
    b = HA.bound(r, S, 0.0, HA.GAMMA_LOSS, E)
    og = sigmoid_grad_f32(x1, x2, sl, ws, 37.0, 1.0, 0.1, g0, False)
    ob = sigmoid_grad_f32(x1, x2, sl, ws, 37.0, 1.0, 0.1, g0, True)
    good, bad = HA.ratio(og, r, b)[0], HA.ratio(ob, r, b)[0]
    moved = float(((ob - og).abs().double() / b).max())
    print('sigmoid rows: float32 restatement %.4f, live test dropped %.4g; the defect moves an element by at most %.4g of '
          'its bound' % (good, bad, moved))
    assert good <= 1.0
    assert 0.0 < moved < 1.0                      # it changes the output, by less than the bound admits (see the docstring)


# -------------------------------------------------------------------------------------------------------------- GPU tests
def _auditor(monkeypatch):
    return HA.Auditor().install(monkeypatch, sgd=False)


@pytest.mark.gpu
@pytest.mark.parametrize('C', SM_C)
def test_softmax_ce_jsd_at_saturated_rows(dev, monkeypatch, C):
    """sm_kernel<false> / <true>.  While the CE was -logf of the label's probability this test failed at every C, and only in
    the forward's checks (measured on the MI355X, whose expf keeps denormals: the figures equal the host restatement's):
    * the pair alone: gaps 86, 88, 95 finite and within 0.11 of the bound (22- to 12-bit denormals); 103 finite and wrong
      (7.944533 for 7.933519, 91 to 131 bounds: a one-unit denormal); 104, 120, 300 +inf;
    * under one-row weights every launch NaN, and the whole launch +inf: a valid row with weight 0 and a gap of 104 adds
      0 * inf.
    With the CE as log s - (x_label - m) the worst one-row / one-pair err / bound is 0.007 / 0.019; the backward kernel was
    and is within 0.04."""
    from oadg_amd import hip_ops
    x, lab, w, planted = softmax_case(C)
    avg, lw, lam = 13.0, 1.0, 10.0
    xd, labd = x.to(dev), lab.to(dev)
    A = _auditor(monkeypatch)

    def run(xx, ll, wt, lm):
        with torch.no_grad():
            return hip_ops.ce_jsd_loss(xx, ll, wt, False, avg, lw, lm)[1]
    seen = check_softmax_forward(A, run, xd, labd, w.to(dev), avg, lw, lam)
    assert {float(g) for g in GAPS if g >= 88} <= set(seen)
    xg = xd.clone().requires_grad_(True)
    tot, parts = hip_ops.ce_jsd_loss(xg, labd, w.to(dev), False, avg, lw, lam)
    (tot * 0.75).backward()
    torch.cuda.synchronize()
    _, _, _, (r, _, _) = HA.ce_jsd_expect(xd, labd, w.to(dev), 1, avg, lw, lam, 0.75)
    check_finite(A, 'sm_kernel<true>', xg.grad, r)
    # rows without a valid label or without weight carry the JSD's gradient only: the CE term exactly absent
    assert {'sm_kernel<false> parts', 'sm_kernel<false> total', 'sm_kernel<true>'} <= set(A.table)
    finish(A, 'softmax rows, C = %d' % C, seen)


@pytest.mark.gpu
@pytest.mark.parametrize('weighted', [True, False])
def test_sigmoid_ce_jsd_at_saturated_rows(dev, monkeypatch, weighted):
    """sig_kernel<false> / <true>: N(0, s) logits up to s = 200 and the exact values around the 1e-7 clamp of (q1 + q2) / 2
    (sigmoid(-16.6) = 6.2e-8, sigmoid(-17.4) = 2.8e-8) and around expf's underflow"""
    from oadg_amd import hip_ops
    half = 4097
    x1, x2, lab = sigmoid_case(half)
    w = None
    if weighted:
        g = torch.Generator().manual_seed(5)
        w = torch.rand(half, generator=g) + 0.5
        w[torch.rand(half, generator=g) < 0.1] = 0.0
        w = w.to(dev)
    A = _auditor(monkeypatch)
    xg = torch.cat([x1, x2]).view(-1, 1).to(dev).requires_grad_(True)
    labd = lab.to(dev)
    tot, parts = hip_ops.ce_jsd_loss(xg, labd, w, True, 37.0, 1.3, 0.1)
    (tot * 0.75).backward()
    torch.cuda.synchronize()
    vals, _, _, (r, _, _) = HA.ce_jsd_expect(xg.detach(), labd, w, 0, 37.0, 1.3, 0.1, 0.75)
    check_finite(A, 'sig_kernel<false>', parts, vals)
    check_finite(A, 'sig_kernel<true>', xg.grad, r)
    assert {'sig_kernel<false> parts', 'sig_kernel<false> total', 'sig_kernel<true>'} <= set(A.table)
    finish(A, 'sigmoid rows, %s' % ('weights' if weighted else 'no weight tensor'))


RPN_FORMS = [
    # (A, dtype, Cy per level, channels-last, forward kernel, backward kernel)
    (3, torch.bfloat16, (16, 16), True, 'rpn_loss_fwd_kernel<3>', 'rpn_loss_bwd_kernel<true, 3>'),
    (2, torch.bfloat16, (16, 16), True, 'rpn_loss_fwd_kernel<0>', 'rpn_loss_bwd_kernel<true, 0>'),
    (3, torch.float32, (16, 16), False, 'rpn_loss_fwd_kernel<0>', 'rpn_loss_bwd_kernel<true, 0>'),
    (3, torch.bfloat16, (16, 24), True, 'rpn_loss_fwd_kernel<3>', 'rpn_loss_bwd_kernel<false, 0>'),
    (2, torch.float32, (16, 24), True, 'rpn_loss_fwd_kernel<0>', 'rpn_loss_bwd_kernel<false, 0>'),
]


@pytest.mark.gpu
@pytest.mark.parametrize('A_,dt,Cys,nhwc,fwd_name,bwd_name', RPN_FORMS)
def test_fused_rpn_loss_at_saturated_logits_every_kernel_form(dev, monkeypatch, A_, dt, Cys, nhwc, fwd_name, bwd_name):
    """oadg_rpn_loss_fwd / _bwd on a two-level pyramid (two blocks forward, five backward, the last one ragged) in every form
    the launcher selects; the objectness channels carry the recipe of the sigmoid rows, the delta channels values up to
    1e4, deltas equal to their target and weightless targets of 3e38"""
    from oadg_amd import hip_ops
    B, sizes = 4, ((13, 19), (3, 4))
    B2 = B // 2
    At = sum(h * w for h, w in sizes) * A_
    g = torch.Generator().manual_seed(31 + A_)
    x1, x2, lab = sigmoid_case(B2 * At, seed=A_)
    X = torch.cat([x1.view(B2, At), x2.view(B2, At)])
    labels = torch.cat([lab.view(B2, At), lab.view(B2, At).flip(1)])              # (view 2's labels are never read)
    label_w = torch.rand((B, At), generator=g) + 0.5
    label_w[torch.rand((B, At), generator=g) < 0.1] = 0.0
    scale = torch.tensor([1.0, 30.0, 1e3, 1e4])[torch.randint(0, 4, (B, At, 1), generator=g)]
    D = (torch.randn((B, At, 4), generator=g) * scale).clamp(-1e4, 1e4)
    ys, a0 = [], 0
    for (h, w), Cy in zip(sizes, Cys):
        n = h * w * A_
        y = torch.randn((B, h, w, Cy), generator=g)
        y[..., :A_] = X[:, a0:a0 + n].view(B, h, w, A_)
        y[..., A_:5 * A_] = D[:, a0:a0 + n].reshape(B, h, w, 4 * A_)
        y = y.to(dt).permute(0, 3, 1, 2)                                           # logical [B, Cy, H, W], NHWC memory
        ys.append((y if nhwc else y.contiguous()).to(dev))
        a0 += n
    _, Dm = HA.rpn_flatten(ys, A_)                                                 # the deltas as the maps hold them
    bbox_t = torch.randn((B, At, 4), generator=g).to(dev) * 2
    bbox_w = torch.rand((B, At, 4), generator=g).to(dev)
    kind = torch.randint(0, 4, (B, At, 4), generator=g).to(dev)
    bbox_t = torch.where(kind == 1, Dm.float(), bbox_t)                            # a delta equal to its target
    bbox_w = torch.where(kind == 2, torch.zeros_like(bbox_w), bbox_w)              # no weight: the target means nothing
    bbox_t = torch.where(kind == 2, torch.full_like(bbox_t, 3e38), bbox_t)
    bbox_w[:, 5::7] = 0.0                                                          # whole anchors without box weight
    assert bool(((Dm[:B2].float() == bbox_t[:B2]) & (bbox_w[:B2] > 0)).any())
    targets = (labels.to(dev), label_w.to(dev), bbox_t.contiguous(), bbox_w.contiguous())
    ys = [y.requires_grad_(True) for y in ys]
    assert HA.Auditor._rpn_kernel(A_, ys, targets[2], targets[3], False) == fwd_name
    assert HA.Auditor._rpn_kernel(A_, ys, targets[2], targets[3], True) == bwd_name
    A = _auditor(monkeypatch)
    lc, lb, parts = hip_ops.rpn_loss(ys, A_, targets, 37.0, 1.3, 0.1, 0.9)
    (lc * 1.5 + lb * 0.5).backward()
    torch.cuda.synchronize()
    vals, _, _ = HA.rpn_loss_expect([y.detach() for y in ys], A_, targets, 37.0, 1.3, 0.1, 0.9)
    check_finite(A, fwd_name, parts, vals)
    for y in ys:
        assert y.grad is not None and bool(torch.isfinite(y.grad).all())
    want = {fwd_name + ' parts', fwd_name + ' returned losses'}
    for l in range(len(sizes)):
        want |= {'%s (level %d)' % (bwd_name, l), '%s zero channels' % bwd_name}
    assert want <= set(A.table), sorted(A.table)
    finish(A, 'fused RPN loss, A = %d, %s, Cy %s' % (A_, dt, Cys))


@pytest.mark.gpu
@pytest.mark.parametrize('beta', [0.0, 0.7, 1.0])
@pytest.mark.parametrize('dt', [torch.float32, torch.bfloat16])
@pytest.mark.parametrize('agnostic', [False, True])
def test_roi_box_loss_and_accuracy_at_the_kinks_and_large_deltas(dev, monkeypatch, beta, dt, agnostic):
    """roi_reg_acc_fwd_kernel / roi_reg_bwd_kernel: |d| exactly beta and exactly 0 (predictions 0 / small integers: exact in
    bf16), |d| up to 1e4, background and negative labels, reg_limit inside the positives, tied maxima in the scores"""
    from oadg_amd import hip_ops
    K, C, reg_limit = 130, 8, 70
    g = torch.Generator().manual_seed(17)
    labels = torch.randint(0, C + 1, (K,), generator=g)                 # C = background
    labels[5::11] = -1
    labels[0:4] = torch.tensor([2, 0, C - 1, 3])
    labels[reg_limit - 1] = 1
    labels[reg_limit] = 1                                               # a positive just outside the limit
    n_reg = 4 if agnostic else 4 * C
    scale = torch.tensor([1.0, 30.0, 1e4])[torch.randint(0, 3, (K, 1), generator=g)]
    pred = (torch.randn((K, n_reg), generator=g) * scale).clamp(-1e4, 1e4).to(dt)
    tg = torch.randn((K, 4), generator=g) * 2
    bw = torch.rand((K, 4), generator=g) + 0.25
    bw[torch.rand((K, 4), generator=g) < 0.15] = 0.0
    col = lambda r: 0 if agnostic else int(labels[r]) * 4   # noqa: E731
    b32 = float(np.float32(beta))
    pred[0, col(0):col(0) + 4] = torch.tensor([0.0, 0.0, 2.0, -3.0]).to(dt)
    tg[0] = torch.tensor([-b32, b32, 2.0, -3.0])                        # |d| = beta twice (both signs), d = 0 twice
    pred[1, col(1):col(1) + 4] = torch.tensor([1e4, -1e4, 0.0, 0.5]).to(dt)
    tg[1] = torch.tensor([-3.0, 7.0, 0.0, 0.5 + b32])
    bw[0] = 1.0
    bw[1] = torch.tensor([0.5, 2.0, 1.0, 1.0])
    cs = torch.randn((K, C + 1), generator=g).to(torch.bfloat16)
    for r in range(0, K, 3):                                            # tied maxima: the first one counts
        a, b = sorted(torch.randperm(C + 1, generator=g)[:2].tolist())
        cs[r, a] = cs[r, b] = 8.0
        if r % 2 and labels[r] >= 0:
            labels[r] = a if r % 4 == 1 else b
    cs[1::6, :] = -2.5                                                  # a whole row tied: class 0
    labels[1] = 0
    pred, cs, labels, tg, bw = (t.to(dev) for t in (pred, cs, labels, tg, bw))
    hits, ties = HA.top1_first(cs, labels)
    assert ties >= K // 3 and 0 < hits < K
    A = _auditor(monkeypatch)
    p = pred.clone().requires_grad_(True)
    loss, acc = hip_ops.roi_reg_acc(p, cs, labels, tg, bw, C, reg_limit, beta, 37.0, 1.5)
    (loss * 2.0).backward()
    torch.cuda.synchronize()
    assert float(acc) == float(np.float32(hits) * (np.float32(100.0) / np.float32(K)))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(p.grad.float()).all()) and p.grad.dtype == dt
    c0 = col(0)
    if beta > 0:       # at |d| = beta the linear branch: sign(d) exactly; at d = 0 exactly 0
        k = np.float32(2.0) * np.float32(1.5) / np.float32(37.0)
        assert p.grad[0, c0:c0 + 2].float().tolist() == torch.tensor([k, -k]).to(dt).float().tolist()
    assert p.grad[0, c0 + 2:c0 + 4].float().abs().sum() == 0
    assert bool((p.grad[reg_limit:] == 0).all())
    assert {'roi_reg_acc_fwd_kernel loss', 'roi_reg_acc_fwd_kernel accuracy', 'roi_reg_bwd_kernel',
            'roi_reg_bwd_kernel zeros'} <= set(A.table)
    assert A.info['accuracy_ties'] == ties
    finish(A, 'RoI box loss, beta %.1f, %s, %s' % (beta, dt, 'class-agnostic' if agnostic else 'per class'))


def supcon_case(D, seed=0):
    """(feats [B, D], labels [2 ori], ori, rp, number of foreground rows) on the CPU; B = 153 = 4 * 32 + 25: two workgroups
    of row tiles, a ragged last tile"""
    g = torch.Generator().manual_seed(200 + D + seed)
    ori, rp, extra = 70, 5, 3
    B = 2 * ori + 2 * rp + extra
    bg = 6
    lab1 = torch.full((ori,), bg, dtype=torch.long)
    lab1[:30] = torch.randint(0, 3, (30,), generator=g)               # foreground classes 0, 1, 2
    lab2 = lab1.clone()
    lab1[30] = 4                                                      # a class with a single member (its twin is background)
    labels = torch.cat([lab1, lab2])
    f = torch.randn((B, D), generator=g)
    f[ori:2 * ori] = f[:ori] + 0.3 * torch.randn((ori, D), generator=g)          # view 2 near view 1
    f[2 * ori + rp:2 * ori + 2 * rp] = f[2 * ori:2 * ori + rp] + 0.3 * torch.randn((rp, D), generator=g)
    f = f * 10.0 ** (torch.rand((B, 1), generator=g) * 6 - 3)         # row norms over 1e-3 .. 1e3 (times sqrt D)
    for r in (0, 1, 40, 41):                                          # exact duplicates across the views (fg and bg rows)
        f[ori + r] = f[r]
    f[2 * ori + rp] = f[2 * ori]                                      # ... and of a random proposal and its twin
    for r in (2, 3, 42, 43):                                          # antipodal pairs
        f[ori + r] = -f[r]
    for r in (4, ori + 5, 44, ori + 45):                              # rows that are exactly zero (fg and bg, either view)
        f[r] = 0.0
    nfg = int((torch.cat([labels, labels[-1:].repeat(B - 2 * ori)]) != bg).sum())
    return f, labels, ori, rp, nfg


@pytest.mark.gpu
@pytest.mark.parametrize('D', [64, 256])
@pytest.mark.parametrize('active', [True, False])
def test_supcon_at_duplicates_antipodes_zero_rows_and_spread_norms(dev, monkeypatch, D, active):
    """supcon_*_kernel; ``active``: the foreground count is min_samples + 1 (the loss runs) / exactly min_samples (loss and
    gradient exactly 0).  A feature row that is exactly zero has an unbounded derivative of normalize(): the expectation's
    S is infinite there, so such a row's own gradient is only required to be finite."""
    from oadg_amd import _lib, hip_ops
    f, labels, ori, rp, nfg = supcon_case(D)
    min_samples = nfg - 1 if active else nfg
    spaces = []
    ws_orig = hip_ops._ws

    def ws(nbytes, device):
        spaces.append(ws_orig(nbytes, device))
        return spaces[-1]
    monkeypatch.setattr(hip_ops, '_ws', ws)
    A = _auditor(monkeypatch)
    x = f.to(dev).requires_grad_(True)
    loss = hip_ops.supcon_loss(x, labels.to(dev), ori, rp, 0.06, min_samples, 0.5)
    (loss * 3.0).backward()
    torch.cuda.synchronize()
    head = spaces[0][:8192].cpu().numpy()
    assert _lib.lib().oadg_supcon_status(head.ctypes.data) == 0
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(x.grad).all())
    if active:
        assert float(loss) > 0 and float(x.grad.abs().sum()) > 0
    else:
        assert float(loss) == 0.0 and float(x.grad.abs().sum()) == 0.0
    assert {'supcon_fin_kernel', 'supcon_bwd_fin_kernel'} <= set(A.table)
    finish(A, 'supcon, D = %d, %d foreground rows, min_samples %d' % (D, nfg, min_samples))


def _detector():
    from oadg_amd.detectors import BaseDetector
    det = BaseDetector.__new__(BaseDetector)
    torch.nn.Module.__init__(det)
    det.log_vars_on_host = False
    return det


@pytest.mark.gpu
def test_parse_losses_over_twelve_decades_and_with_an_infinite_entry(dev, monkeypatch):
    """parse_losses_kernel: ``packed`` and ``total`` bit-equal to the float32 left-to-right sums; one +inf entry gives +inf,
    not NaN, in its variable and in the total"""
    f32 = np.float32
    level = [3.7e-8, 2.5e3, 1.1e-3, 0.93, 7.7e-6]
    single = dict(loss_rpn_bbox=9.9e3, acc=87.5, loss_cls=1.0e4, loss_bbox=1.3e-8, loss_cont=4.2e-2)
    det = _detector()

    def run(first):
        losses = dict(loss_rpn_cls=[torch.tensor(v, device=dev).view(()) for v in [first] + level[1:]])
        losses.update({k: torch.tensor([v], device=dev) for k, v in single.items()})
        loss, log_vars = det._parse_losses(losses)
        torch.cuda.synchronize()
        s = f32(0.0)
        for v in [first] + level[1:]:
            s = f32(s + f32(v))
        want = [s] + [f32(0.0) + f32(v) for v in single.values()]
        tot = f32(0.0)
        for k, v in zip(['loss_rpn_cls'] + list(single), want):
            if 'loss' in k:
                tot = f32(tot + v)
        return loss, log_vars, want + [tot]
    with np.errstate(over='ignore'):
        loss, lv, want = run(float('inf'))
    assert list(lv) == ['loss_rpn_cls'] + list(single) + ['loss']
    assert float(lv['loss_rpn_cls']) == float('inf') and float(loss) == float('inf') and float(lv['loss']) == float('inf')
    assert [float(lv[k]) for k in single] == [float(v) for v in want[1:-1]]
    A = _auditor(monkeypatch)
    loss, lv, want = run(level[0])
    got = torch.stack([lv[k].reshape(()) for k in lv]).cpu().numpy()
    assert got.dtype == np.float32 and got.tobytes() == np.array(want, dtype=np.float32).tobytes(), (got, want)
    assert float(loss) == float(want[-1])
    assert {'parse_losses_kernel packed', 'parse_losses_kernel total'} <= set(A.table)
    finish(A, '_parse_losses')
