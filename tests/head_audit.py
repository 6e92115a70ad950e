"""Launch auditor of the non-convolution half of a training step: RoIAlign forward / backward and its processing order, the
fused RPN loss, the RoI head's CE + JSD and box loss, supcon, _parse_losses, the bf16 casts / column permutation of the RoI
head's linears and the fused SGD step.  Each launch is checked elementwise against a float64 recomputation from the exact
operands it received (teacher forcing), in the form of tests/conv_audit.py::

    |o - r| <= RHO * |r| + GAMMA * S + ALPHA + (named terms)          (RHO = 0 for fp32 outputs)

``S`` is the same computation over absolute values.  The named terms are the fp32 rounding of quantities the kernel computes
before a smooth function of them (RoIAlign's sample coordinates, the sigmoid / softmax probabilities).  Exact operations
(casts, permutations, the SGD step) are compared bit for bit.

Discrete choices (RoIAlign's pyramid level, adaptive sample counts, the out-of-map sample drop) that sit within fp32 rounding of their threshold accept either outcome.  The elements this carve-out covers are
counted in ``Auditor.borderline`` and the GPU tests cap that count.

``Auditor.install(monkeypatch)`` wraps the Python entry points of hip_ops and apis.FusedSGD.step.  The pure fp64 reference
functions below are what tests/test_head_audit.py's CPU self-tests tie to oracle/ and plant errors into.
"""
import torch
import torch.nn.functional as F

RHO = 2.0 ** -8          # one bf16 rounding
# fp32 arithmetic of RoIAlign (bilinear weights, sums of up to ~10^3 weighted samples, the division by the count) and of the
# backward's sums.  Set from measurement: the worst err / bound of the fp32 outputs (the stress launch of
# tests/test_head_audit.py with fp32 maps: roi_align_bwd_kernel and roi_align_fwd_rows_kernel<float>) is 0.061, a margin of
# 16x.  (The bf16 outputs of the audited steps reach 0.87 - 0.98: one bf16 rounding of a value just above a power of two,
# the RHO term, not this one.)
# Away from 7 x 7 / adaptive / aligned (tests/test_roi_align_stress.py: pooled sides 1 .. 14, sampling ratios 1 - 3, unaligned
# RoIs, bins of 31 - 97 pixels on both sides of the table overflows, 4 - 516 channels, maps down to 1 x 1, 2 - 8 tiles per
# workgroup, degenerate boxes, more than 8192 RoIs) the same constants hold on the MI355X with no RoI taking the other side of
# a borderline choice - worst err / bound of the fp32 outputs:
#   roi_align_bwd_kernel 0.089 (97-pixel bins, 194 samples per bin through roi_bwd_scatter; 0.065 for two-sample bins 70
#   pixels wide, at most 0.004 in every other family), roi_align_fwd_rows_kernel<float> 0.040 (two-sample bins of 20 - 70
#   pixels; 0.007 elsewhere); with 33 x 33 samples per bin both stay below 0.025.
# (bf16 outputs: roi_align_fwd_rows_kernel<unsigned short> 0.84, roi_align_bwd_tiles_kernel 0.79, roi_align_bwd_kernel with
# bf16 maps - a pooled side above 8 - 0.57: RHO.)
GAMMA_ROI = 2.0 ** -16
# fp32 arithmetic of the loss kernels (logf / expf, per-element terms summed in fp64, the final fp32 scalings).  Set from
# measurement: the worst err / bound of the fp32 outputs over the three audited steps is 0.072 (supcon's feature gradient,
# configs[1]), a margin of 14x; the loss values stay below 0.006, sig_kernel<true> / sm_kernel<true> below 0.008.
# At saturated operands (tests/test_loss_stress.py: softmax gaps up to 300, sigmoid logits N(0, 200) and the values around
# the 1e-7 clamp and expf's underflow, deltas up to 1e4, supcon duplicates / antipodes / zero rows / norms over six decades)
# the same constants hold on the MI355X with no named term added - worst err / bound of the fp32 outputs:
#   sig_kernel<true> 0.093, rpn_loss_bwd_kernel fp32 maps 0.096 (<true, 0> 0.091, <false, 0> 0.096), sm_kernel<true> 0.039,
#   supcon_bwd_fin_kernel 0.039, roi_reg_bwd_kernel 0.008; the loss values: sm_kernel<false> 0.019 (one pair alone; 0.007
#   for the whole launch and under one-row weights), sig_kernel<false> 0.002, rpn_loss_fwd_kernel 0.001,
#   roi_reg_acc_fwd_kernel 0.004, supcon_fin_kernel 0.003, parse_losses_kernel 0.004.
# (bf16 outputs - the RPN gradient maps, the bf16 box gradient - reach 0.82 - 0.97 there as in the audited steps: RHO.)
# sm_kernel<false> computed the CE as -logf(p_label) until that suite: +inf from a gap of 104 between the row maximum and the
# label's logit, a one-unit denormal at 103 (91 - 131 bounds of that row), NaN as soon as such a row had weight 0.
GAMMA_LOSS = 2.0 ** -16
ALPHA = 1e-30
# the RoI head's weight gradients: the library GEMM (g^T x, K = up to 4096 bf16 products summed in fp32) - not this
# project's kernel; the check is of the gradient's path through the permutation, the casts and autograd.  The same constant
# as tests/conv_audit.py's fp32 accumulation.
GAMMA_GEMM = 2.0 ** -14
# absolute fp32 error of a RoIAlign sample coordinate (in feature pixels): start + ph * bin + (iy + 0.5) * bin / grid, four
# roundings of values below 2^11 (2^-13 each, 2^-11 in all); it moves each bilinear weight by at most that much
POS_ERR = 2.0 ** -11
# relative fp32 error of a sigmoid / softmax probability (expf, the division; and 1 - p for the complementary one)
PROB_ERR = 2.0 ** -21
# thresholds of the discrete choices: how close (in the unit of the compared quantity) counts as "within fp32 rounding"
TOL_LVL = 1e-5           # log2(sqrt(wh) / finest + 1e-6)
GRID_ERR = 2.0 ** -21    # rh / PH (an adaptive sample count is ceil of it): see roi_geometry
TOL_POS = 4 * POS_ERR    # a sample coordinate against -1 and the map size
IGNORE_INDEX = -100
# the C-ABI calls this auditor answers for (tests/test_target_audit.py's closure over the call sites of oa-dg_amd/)
CLAIMS = {
    'oadg_roi_align_fwd', 'oadg_roi_align_bwd', 'oadg_roi_align_bwd_tiles', 'oadg_roi_order', 'oadg_roi_order_keys',
    'oadg_rpn_loss_fwd', 'oadg_rpn_loss_bwd', 'oadg_ce_jsd_fwd', 'oadg_ce_jsd_bwd', 'oadg_roi_reg_acc_fwd', 'oadg_roi_reg_bwd',
    'oadg_supcon_fwd', 'oadg_supcon_bwd', 'oadg_parse_losses', 'oadg_fc_weight_permute', 'oadg_sgd_step_multi',
}


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def ratio(o, ref, b):
    """(worst err / bound, flat index of the worst element)"""
    e = (o.to(torch.float64) - ref).abs() / b
    e = torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e)
    if e.numel() == 0:
        return 0.0, 0
    i = int(e.reshape(-1).argmax())
    return float(e.reshape(-1)[i]), i


def bound(r, S, rho, gamma, *extra):
    b = rho * r.abs() + gamma * S + ALPHA
    for e in extra:
        b = b + e
    return b


# ------------------------------------------------------------------------------------------------------ RoIAlign (fp64)
def roi_levels(rois, n_levels, finest_scale, shift=0):
    """single_level_roi_extractor.py:50-54 in fp64; ``shift`` -1 / +1 moves the floor's threshold by TOL_LVL (the other side of
    a borderline choice); a NaN scale (negative area) takes level 0 like the kernel's fminf / fmaxf"""
    r = rois.to(torch.float64)
    if n_levels == 1:
        return torch.zeros(r.shape[0], dtype=torch.long, device=r.device), torch.zeros(r.shape[0], dtype=torch.bool,
                                                                                         device=r.device)
    v = torch.log2(torch.sqrt((r[:, 3] - r[:, 1]) * (r[:, 4] - r[:, 2])) / finest_scale + 1e-6)
    v = torch.where(torch.isnan(v), torch.full_like(v, -1.0), v)
    lvl = torch.floor(v + shift * TOL_LVL).clamp(0, n_levels - 1).long()
    near = ((v - v.round()).abs() < TOL_LVL) & (v.round() >= 1) & (v.round() <= n_levels - 1)
    return lvl, near


def roi_geometry(rois, lvl, shapes, scales, PH, PW, sampling_ratio, aligned, shift=0):
    """per-RoI fp64 geometry of mmcv's RoIAlign on the given levels: start, bin size, sample counts (``shift``: the other
    side of a borderline ceil), count = max(gh * gw, 1), batch index, map size"""
    r = rois.to(torch.float64)
    dev = r.device
    sc = torch.tensor([float(s) for s in scales], dtype=torch.float64, device=dev)[lvl]
    Hs = torch.tensor([s[2] for s in shapes], dtype=torch.long, device=dev)[lvl]
    Ws = torch.tensor([s[3] for s in shapes], dtype=torch.long, device=dev)[lvl]
    off = 0.5 if aligned else 0.0
    sw, sh = r[:, 1] * sc - off, r[:, 2] * sc - off
    rw, rh = r[:, 3] * sc - off - sw, r[:, 4] * sc - off - sh
    if not aligned:
        rw, rh = rw.clamp_min(1.0), rh.clamp_min(1.0)
    if sampling_ratio > 0:
        gh = torch.full_like(lvl, sampling_ratio)
        gw = torch.full_like(lvl, sampling_ratio)
        near = torch.zeros_like(lvl, dtype=torch.bool)
    else:
        th, tw = rh / PH, rw / PW
        # fp32: start / end = roi * scale - off (one rounding each, the scales are powers of two), rh = end - start and
        # rh / PH one more each - under 2^-23 (|start| + |end| + |rh|) / PH + 2^-24 rh / PH; tolerance: twice that
        eh = GRID_ERR * ((sh.abs() + (sh + rh).abs() + rh.abs()) / PH + th.abs())
        ew = GRID_ERR * ((sw.abs() + (sw + rw).abs() + rw.abs()) / PW + tw.abs())
        gh = torch.ceil(th + shift * eh).long()
        gw = torch.ceil(tw + shift * ew).long()
        near = ((th - th.round()).abs() < eh) | ((tw - tw.round()).abs() < ew)
    return dict(sh=sh, sw=sw, bh=rh / PH, bw=rw / PW, gh=gh, gw=gw, count=(gh * gw).clamp_min(1).to(torch.float64),
                batch=r[:, 0].trunc().long(), H=Hs, W=Ws, near=near)


def _drop_near(start, binsz, grid, P, size):
    """whether a sample coordinate start + (j + 0.5) bin / grid, j < P grid, lies within TOL_POS of -1 or ``size``"""
    g = grid.clamp_min(1).to(torch.float64)
    step = binsz / g
    n = (P * grid).clamp_min(1)
    near = torch.zeros_like(grid, dtype=torch.bool)
    for T in (-1.0, None):
        Tv = size.to(torch.float64) if T is None else torch.full_like(start, T)
        j = torch.where(step != 0, (Tv - start) / step.where(step != 0, torch.ones_like(step)) - 0.5, torch.zeros_like(start))
        j = torch.minimum(torch.maximum(j.round(), torch.zeros_like(j)), (n - 1).to(torch.float64))
        near |= ((start + (j + 0.5) * step - Tv).abs() < TOL_POS) & (grid > 0)
    return near


def _axis(start, binsz, grid, i, P, size, shift):
    """[n, P] sample coordinate of sample ``i`` of every bin along one axis: (low, high, w_low, w_high, inside)"""
    p = torch.arange(P, dtype=torch.float64, device=start.device).view(1, P)
    g = grid.clamp_min(1).to(torch.float64).view(-1, 1)
    c = start.view(-1, 1) + p * binsz.view(-1, 1) + (i + 0.5) * binsz.view(-1, 1) / g
    S = size.view(-1, 1).to(torch.float64)
    inside = ~((c < -1.0 - shift * TOL_POS) | (c > S + shift * TOL_POS)) & (i < grid).view(-1, 1)
    c = c.clamp_min(0.0)
    low = c.floor().long()
    edge = low >= size.view(-1, 1) - 1
    low = torch.where(edge, size.view(-1, 1) - 1, low)
    high = torch.where(edge, low, low + 1)
    c = torch.where(edge, low.to(torch.float64), c)
    lw = c - low.to(torch.float64)
    return low, high, 1.0 - lw, lw, inside


def _chunks(idx, per_roi, limit=1 << 24):
    n = max(1, limit // max(per_roi, 1))
    for s in range(0, idx.numel(), n):
        yield idx[s:s + n]


def _pow2(t):
    """sample-count bucket: powers of two up to 8, exact above (wide bins: one loop per count)"""
    t = max(int(t), 1)
    return t if t > 8 or not t & (t - 1) else 1 << t.bit_length()


def _groups(lvl, geo, sel):
    """RoI subsets sharing a level and a power-of-two bound on the sample counts (the loops below run to that bound with
    a mask)"""
    out = {}
    ok = sel & (geo['gh'] > 0) & (geo['gw'] > 0) & (geo['batch'] >= 0)
    if not bool(ok.any()):
        return out
    idx = torch.nonzero(ok).view(-1)
    key = torch.stack([lvl[idx], geo['gh'][idx], geo['gw'][idx]], 1).cpu()
    for (l, gh, gw), i in zip(key.tolist(), idx.tolist()):
        out.setdefault((l, _pow2(gh), _pow2(gw)), []).append(i)
    return {k: torch.tensor(v, dtype=torch.long, device=lvl.device) for k, v in out.items()}


def roi_align_ref(feats, rois, lvl, geo, PH, PW, sel=None):
    """(r, S, S4) [K, PH, PW, C] fp64 of RoIAlign over maps ``feats`` (logical [N, C, H, W], any dtype / layout) with the
    per-RoI level ``lvl`` and geometry ``geo``: r = sum of the four-corner bilinear samples / count, S = the same over |w| |f|,
    S4 = sum of the four corners' |f| / count (what a POS_ERR shift of the weights can move).  RoIs with a bad batch index or
    no samples give 0.  ``sel``: only these RoIs (others stay 0)."""
    K = rois.shape[0]
    N, C = feats[0].shape[:2]
    dev = rois.device
    r = torch.zeros((K, PH, PW, C), dtype=torch.float64, device=dev)
    S, S4 = torch.zeros_like(r), torch.zeros_like(r)
    sel = torch.ones(K, dtype=torch.bool, device=dev) if sel is None else sel
    sel = sel & (geo['batch'] < N)
    for (l, GH, GW), idx_all in _groups(lvl, geo, sel).items():
        fm = feats[l]
        H, W = fm.shape[2], fm.shape[3]
        flat = fm.detach().permute(0, 2, 3, 1).reshape(N * H * W, C)
        for idx in _chunks(idx_all, PH * PW * C):
            n = idx.numel()
            acc, sa, s4 = (torch.zeros((n, PH, PW, C), dtype=torch.float64, device=dev) for _ in range(3))
            base = (geo['batch'][idx] * H * W).view(n, 1, 1)
            for iy in range(GH):
                yl, yh, hy, ly, iny = _axis(geo['sh'][idx], geo['bh'][idx], geo['gh'][idx], iy, PH, geo['H'][idx],
                                            geo.get('shift', 0))
                for ix in range(GW):
                    xl, xh, hx, lx, inx = _axis(geo['sw'][idx], geo['bw'][idx], geo['gw'][idx], ix, PW, geo['W'][idx],
                                                geo.get('shift', 0))
                    m = (iny.view(n, PH, 1) & inx.view(n, 1, PW)).to(torch.float64)
                    if not bool(m.any()):
                        continue
                    for (yy, wy), (xx, wx) in (((yl, hy), (xl, hx)), ((yl, hy), (xh, lx)), ((yh, ly), (xl, hx)),
                                               ((yh, ly), (xh, lx))):
                        rows = base + yy.view(n, PH, 1) * W + xx.view(n, 1, PW)
                        f = flat[rows.view(-1)].to(torch.float64).view(n, PH, PW, C)
                        w = (wy.view(n, PH, 1) * wx.view(n, 1, PW) * m).unsqueeze(-1)
                        acc += w * f
                        sa += w.abs() * f.abs()
                        s4 += m.unsqueeze(-1) * f.abs()
            cnt = geo['count'][idx].view(n, 1, 1, 1)
            r[idx], S[idx], S4[idx] = acc / cnt, sa / cnt, s4 / cnt
    return r, S, S4


def roi_align_bwd_ref(shapes, rois, lvl, geo, gout, PH, PW):
    """per level (r, S, S4) [N, H, W, C] fp64 of the scatter of gout [K, C, PH, PW] with RoIAlign's weights: the gradient
    of every map element (exact zeros where no sample lands)"""
    N, C = shapes[0][:2]
    dev = rois.device
    outs = [[torch.zeros((N * s[2] * s[3], C), dtype=torch.float64, device=dev) for _ in range(3)] for s in shapes]
    g_all = gout.detach().permute(0, 2, 3, 1)
    sel = geo['batch'] < N
    for (l, GH, GW), idx_all in _groups(lvl, geo, sel).items():
        H, W = shapes[l][2], shapes[l][3]
        dr, dS, d4 = outs[l]
        for idx in _chunks(idx_all, PH * PW * C):
            n = idx.numel()
            g = g_all[idx].to(torch.float64) / geo['count'][idx].view(n, 1, 1, 1)
            ga = g.abs()
            base = (geo['batch'][idx] * H * W).view(n, 1, 1)
            for iy in range(GH):
                yl, yh, hy, ly, iny = _axis(geo['sh'][idx], geo['bh'][idx], geo['gh'][idx], iy, PH, geo['H'][idx],
                                            geo.get('shift', 0))
                for ix in range(GW):
                    xl, xh, hx, lx, inx = _axis(geo['sw'][idx], geo['bw'][idx], geo['gw'][idx], ix, PW, geo['W'][idx],
                                                geo.get('shift', 0))
                    m = (iny.view(n, PH, 1) & inx.view(n, 1, PW)).to(torch.float64)
                    if not bool(m.any()):
                        continue
                    for (yy, wy), (xx, wx) in (((yl, hy), (xl, hx)), ((yl, hy), (xh, lx)), ((yh, ly), (xl, hx)),
                                               ((yh, ly), (xh, lx))):
                        rows = (base + yy.view(n, PH, 1) * W + xx.view(n, 1, PW)).view(-1)
                        w = (wy.view(n, PH, 1) * wx.view(n, 1, PW) * m).unsqueeze(-1)
                        dr.index_add_(0, rows, (w * g).reshape(-1, C))
                        dS.index_add_(0, rows, (w.abs() * ga).reshape(-1, C))
                        d4.index_add_(0, rows, (m.unsqueeze(-1) * ga).reshape(-1, C))
    return [[t.view(N, s[2], s[3], C) for t in o] for o, s in zip(outs, shapes)]


def roi_setup(rois, shapes, scales, finest_scale, PH, PW, sampling_ratio, aligned, shift=0):
    """(levels, geometry, borderline RoIs) of one variant: ``shift`` 0 = the fp64 choices, -1 / +1 = the other side of every
    choice that lies within its tolerance"""
    lvl, near_l = roi_levels(rois, len(shapes), finest_scale, shift)
    geo = roi_geometry(rois, lvl, shapes, scales, PH, PW, sampling_ratio, aligned, shift)
    geo['shift'] = shift
    near = near_l | geo['near'] | _drop_near(geo['sh'], geo['bh'], geo['gh'], PH, geo['H']) | \
        _drop_near(geo['sw'], geo['bw'], geo['gw'], PW, geo['W'])
    return lvl, geo, near


def roi_order_expect(rois, n_img, levels, finest_scale):
    """fp64 / fp32 restatement of csrc roi_order_key: (candidate keys [K, 2] - the second differs from the first only where
    the level is borderline -, group of every candidate)"""
    r32 = rois.to(torch.float32)
    r = rois.to(torch.float64)
    # (a NaN coordinate: fmaxf(NaN, 0) is 0 - level 0 - and the conversion of a NaN cell coordinate to int gives 0)
    w, h = torch.nan_to_num(r[:, 3] - r[:, 1], nan=0.0).clamp_min(0), torch.nan_to_num(r[:, 4] - r[:, 2], nan=0.0).clamp_min(0)
    v = torch.log2(torch.sqrt(w * h) / finest_scale + 1e-6)
    cands = []
    for shift in (0, 1, -1):
        lvl = torch.floor(v + shift * TOL_LVL).clamp(0, levels - 1).long()
        cell = (64.0 * (1 << lvl).to(torch.float32))
        qx = torch.nan_to_num((((r32[:, 1] + r32[:, 3]) * 0.5) / cell).trunc(), nan=0.0).long().clamp(0, 1023)
        qy = torch.nan_to_num((((r32[:, 2] + r32[:, 4]) * 0.5) / cell).trunc(), nan=0.0).long().clamp(0, 1023)
        b = r32[:, 0].trunc().long().clamp(0, n_img - 1)
        cands.append((((lvl * n_img + b) * 1024 + qy) * 1024 + qx, lvl * n_img + b))
    return cands


def check_order(rois, n_img, levels, finest_scale, order, rng):
    """(ok, chosen level per RoI or None, borderline RoIs): ``order`` must be a stable sort of the keys and ``rng`` the first
    position of every (level, image) group; a RoI whose level is borderline may sort with either level"""
    K = rois.shape[0]
    cands = roi_order_expect(rois, n_img, levels, finest_scale)
    o = order.long().cpu()
    if sorted(o.tolist()) != list(range(K)):
        return False, None, 0
    keys = torch.stack([c[0] for c in cands], 1).cpu()[o]          # [K, 3] in the launch's order
    grp = torch.stack([c[1] for c in cands], 1).cpu()[o]
    ol = o.tolist()
    prev, chosen_g = None, []
    border = 0
    for j in range(K):
        opts = sorted(set(zip(keys[j].tolist(), grp[j].tolist())))
        border += len(opts) > 1
        pick = None
        for kv, g in opts:
            if prev is None or (kv, ol[j]) > prev:
                pick = (kv, g)
                break
        if pick is None:
            return False, None, border
        prev = (pick[0], ol[j])
        chosen_g.append(pick[1])
    cg = torch.tensor(chosen_g, dtype=torch.long)
    lvl = torch.empty(K, dtype=torch.long)
    lvl[o] = cg // n_img
    if rng is not None:
        want = torch.searchsorted(cg, torch.arange(levels * n_img + 1, dtype=torch.long)).int()
        if not torch.equal(rng.cpu().int(), want):
            return False, None, border
    return True, lvl.to(rois.device), border


# ------------------------------------------------------------------------------------------------------ losses (fp64)
def _xlogy_abs(t, logm):
    """(t (ln t - ln m), |t ln t| + |t ln m|) with 0 at t == 0"""
    lt = torch.where(t > 0, torch.log(t.clamp_min(1e-300)), torch.zeros_like(t))
    return t * (lt - logm), t * (lt.abs() + logm.abs())


def _dterm(t1, t2, mraw, m, logm):
    """d/dt1 of 1/2 [t1 (ln t1 - ln M) + t2 (ln t2 - ln M)], M = clamp((t1 + t2) / 2, 1e-7, 1), and its magnitude"""
    lt = torch.log(t1.clamp_min(1e-300))
    live = ((mraw >= 1e-7) & (mraw <= 1.0)).to(t1.dtype)
    g = 0.5 * (lt + 1.0 - logm) - live * 0.5 * (t1 + t2) * 0.5 / m
    a = 0.5 * (lt.abs() + 1.0 + logm.abs()) + live * 0.5 * (t1 + t2) * 0.5 / m
    z = t1 > 0
    return torch.where(z, g, torch.zeros_like(g)), torch.where(z, a, torch.zeros_like(a))


def sigmoid_jsd(x1, x2):
    """per pair (JSD, S_JSD, named sigmoid term of the value) of 1-logit rows and the gradient pieces
    (d1, d2, S_d1, S_d2, p1, q1, p2, q2)"""
    p1, q1, p2, q2 = torch.sigmoid(x1), torch.sigmoid(-x1), torch.sigmoid(x2), torch.sigmoid(-x2)
    mpr, mqr = (p1 + p2) / 2, (q1 + q2) / 2
    mp, mq = mpr.clamp(1e-7, 1.0), mqr.clamp(1e-7, 1.0)
    lmp, lmq = torch.log(mp), torch.log(mq)
    terms = [_xlogy_abs(p1, lmp), _xlogy_abs(q1, lmq), _xlogy_abs(p2, lmp), _xlogy_abs(q2, lmq)]
    js = sum(t[0] for t in terms) / 2
    Sj = sum(t[1] for t in terms) / 2
    # each probability off by PROB_ERR max(p, q) (q = 1 - p in fp32): moves t ln(t / m) by that times |ln t| + |ln m| + 2
    e = lambda t, lm, big: PROB_ERR * big * (torch.log(t.clamp_min(1e-300)).abs() + lm.abs() + 2.0)  # noqa: E731
    b1, b2 = torch.maximum(p1, q1), torch.maximum(p2, q2)
    sig = (e(p1, lmp, b1) + e(q1, lmq, b1) + e(p2, lmp, b2) + e(q2, lmq, b2)) / 2
    a1, sa1 = _dterm(p1, p2, mpr, mp, lmp)
    a2, sa2 = _dterm(q1, q2, mqr, mq, lmq)
    c1, sc1 = _dterm(p2, p1, mpr, mp, lmp)
    c2, sc2 = _dterm(q2, q1, mqr, mq, lmq)
    return js, Sj, sig, dict(d1=a1 - a2, d2=c1 - c2, S1=sa1 + sa2, S2=sc1 + sc2, p1=p1, q1=q1, p2=p2, q2=q2, b1=b1, b2=b2)


def bce_logits(x, t):
    """(value, S) of torch's binary_cross_entropy_with_logits"""
    v = torch.clamp_min(x, 0) - x * t + torch.log1p(torch.exp(-x.abs()))
    return v, (1 - t) * x.abs() + torch.clamp_min(-x, 0) + torch.log1p(torch.exp(-x.abs()))


def rpn_targets_view1(labels, label_w):
    valid = (labels >= 0) & (labels != IGNORE_INDEX)
    t = (valid & (labels == 0)).to(torch.float64)
    w = torch.where(valid, label_w.to(torch.float64), torch.zeros_like(label_w, dtype=torch.float64))
    return t, w


def rpn_flatten(ys, A):
    """([B, At] logits, [B, At, 4] deltas) fp64 of the head's channel-padded maps, anchor = level offset + (h W + w) A + a"""
    xs, ds = [], []
    for y in ys:
        B, Cy, H, W = y.shape
        t = y.detach().permute(0, 2, 3, 1).to(torch.float64)
        xs.append(t[..., :A].reshape(B, H * W * A))
        ds.append(t[..., A:5 * A].reshape(B, H * W * A, 4))
    return torch.cat(xs, 1), torch.cat(ds, 1)


def rpn_loss_expect(ys, A, targets, avg, w_cls, lam, w_box):
    """fp64 (values [ce + jsd, ce, jsd, l1], S [4], named sigmoid term [4]) of the fused RPN loss"""
    labels, label_w, bbox_t, bbox_w = targets
    X, D = rpn_flatten(ys, A)
    B2 = X.shape[0] // 2
    t, w = rpn_targets_view1(labels[:B2], label_w[:B2])
    bce, Sb = bce_logits(X[:B2], t)
    js, Sj, sig, _ = sigmoid_jsd(X[:B2], X[B2:])
    bw, bt = bbox_w[:B2].to(torch.float64), bbox_t[:B2].to(torch.float64)
    l1 = ((D[:B2] - bt).abs() * bw).sum()
    Sl1 = ((D[:B2].abs() + bt.abs()) * bw.abs()).sum()
    kc, kj, kb = w_cls / avg, lam / avg, w_box / avg
    ce, Sce = kc * (w * bce).sum(), abs(kc) * (w.abs() * Sb).sum()
    # the BCE's own sigmoid: |d bce / d x| <= 1, fp32 expf / logf relative error on its terms
    jv, Sjv, sg = kj * js.sum(), abs(kj) * Sj.sum(), abs(kj) * sig.sum()
    vals = torch.stack([ce + jv, ce, jv, kb * l1])
    S = torch.stack([Sce + Sjv, Sce, Sjv, abs(kb) * Sl1])
    named = torch.stack([sg, torch.zeros_like(sg), sg, torch.zeros_like(sg)])
    return vals, S, named


def rpn_grad_expect(ys, A, targets, avg, w_cls, lam, w_box, gc, gb):
    """per level (r, S, named) [B, H, W, Cy] fp64 of the fused RPN loss's gradient maps: view 1 = BCE + JSD on the logit
    channels and the L1 sign on the delta channels; view 2 = JSD only; every other channel 0"""
    labels, label_w, bbox_t, bbox_w = targets
    X, D = rpn_flatten(ys, A)
    B = X.shape[0]
    B2 = B // 2
    t, w = rpn_targets_view1(labels[:B2], label_w[:B2])
    _, _, _, P = sigmoid_jsd(X[:B2], X[B2:])
    kc, kj, kb = w_cls / avg, lam / avg, w_box / avg
    p1, q1, p2, q2 = P['p1'], P['q1'], P['p2'], P['q2']
    g1 = gc * (kc * w * (p1 - t) + kj * p1 * q1 * P['d1'])
    S1 = abs(gc) * (abs(kc) * w.abs() * (p1 + t) + abs(kj) * p1 * q1 * P['S1'])
    e1 = abs(gc) * PROB_ERR * P['b1'] * (abs(kc) * w.abs() + abs(kj) * (P['d1'].abs() + 2.0))
    g2 = gc * kj * p2 * q2 * P['d2']
    S2 = abs(gc) * abs(kj) * p2 * q2 * P['S2']
    e2 = abs(gc) * PROB_ERR * P['b2'] * abs(kj) * (P['d2'].abs() + 2.0)
    bw, bt = bbox_w[:B2].to(torch.float64), bbox_t[:B2].to(torch.float64)
    gd = gb * kb * bw * torch.sign(D[:B2] - bt)
    Sd = gd.abs()
    out = []
    a0 = 0
    for y in ys:
        _, Cy, H, W = y.shape
        n = H * W * A
        r = torch.zeros((B, H, W, Cy), dtype=torch.float64, device=X.device)
        S, E = torch.zeros_like(r), torch.zeros_like(r)
        for dst, v1, v2 in ((r, g1, g2), (S, S1, S2), (E, e1, e2)):
            dst[:B2, ..., :A] = v1[:, a0:a0 + n].view(B2, H, W, A)
            dst[B2:, ..., :A] = v2[:, a0:a0 + n].view(B2, H, W, A)
        r[:B2, ..., A:5 * A] = gd[:, a0:a0 + n].reshape(B2, H, W, 4 * A)
        S[:B2, ..., A:5 * A] = Sd[:, a0:a0 + n].reshape(B2, H, W, 4 * A)
        out.append((r, S, E))
        a0 += n
    return out


def ce_jsd_expect(logits, labels, weights, mode, avg, lw, lam, g0=None):
    """fp64 CrossEntropyLossPlus (jsdv1_3_2aug): ((total, ce, lambda jsd), S [3], named [3]) and, with ``g0``, the
    gradient (r, S, named) [R, C].  mode 0: 1-logit sigmoid rows, 1: softmax rows"""
    x = logits.detach().to(torch.float64).view(logits.shape[0], -1)
    R, C = x.shape
    h = R // 2
    lab = labels.view(-1)[:h]
    wsrc = weights.view(-1)[:h].to(torch.float64) if weights is not None else None
    kc, kj = lw / avg, lam / avg
    if mode == 0:
        valid = (lab >= 0) & (lab != IGNORE_INDEX)
        t = (valid & (lab == 0)).to(torch.float64)
        w = torch.where(valid, wsrc if wsrc is not None else torch.ones_like(t), torch.zeros_like(t))
        bce, Sb = bce_logits(x[:h, 0], t)
        js, Sj, sig, P = sigmoid_jsd(x[:h, 0], x[h:, 0])
        ce, Sce = kc * (w * bce).sum(), abs(kc) * (w.abs() * Sb).sum()
        jv, Sjv, sg = kj * js.sum(), abs(kj) * Sj.sum(), abs(kj) * sig.sum()
        vals = torch.stack([ce + jv, ce, jv])
        S = torch.stack([Sce + Sjv, Sce, Sjv])
        named = torch.stack([sg, torch.zeros_like(sg), sg])
        if g0 is None:
            return vals, S, named
        p1, q1, p2, q2 = P['p1'], P['q1'], P['p2'], P['q2']
        r = torch.zeros_like(x)
        Sg, E = torch.zeros_like(x), torch.zeros_like(x)
        r[:h, 0] = g0 * (kc * w * (p1 - t) + kj * p1 * q1 * P['d1'])
        Sg[:h, 0] = abs(g0) * (abs(kc) * w.abs() * (p1 + t) + abs(kj) * p1 * q1 * P['S1'])
        E[:h, 0] = abs(g0) * PROB_ERR * P['b1'] * (abs(kc) * w.abs() + abs(kj) * (P['d1'].abs() + 2.0))
        r[h:, 0] = g0 * kj * p2 * q2 * P['d2']
        Sg[h:, 0] = abs(g0) * abs(kj) * p2 * q2 * P['S2']
        E[h:, 0] = abs(g0) * PROB_ERR * P['b2'] * abs(kj) * (P['d2'].abs() + 2.0)
        return vals, S, named, (r, Sg, E)
    valid = (lab != IGNORE_INDEX) & (lab >= 0) & (lab < C)
    w = torch.where(valid, wsrc if wsrc is not None else torch.ones(h, dtype=torch.float64, device=x.device),
                    torch.zeros(h, dtype=torch.float64, device=x.device))
    ls1, ls2 = torch.log_softmax(x[:h], 1), torch.log_softmax(x[h:], 1)
    p1, p2 = ls1.exp(), ls2.exp()
    # probabilities from expf(x - max) / sum: relative error ~ ulp (1 + |x - max|)
    e1 = PROB_ERR * (1.0 + (x[:h] - x[:h].max(1, keepdim=True)[0]).abs())
    e2 = PROB_ERR * (1.0 + (x[h:] - x[h:].max(1, keepdim=True)[0]).abs())
    li = lab.clamp(0, C - 1).view(-1, 1)
    nll = -ls1.gather(1, li).view(-1)
    ce, Sce = kc * (w * nll).sum(), abs(kc) * (w.abs() * nll.abs()).sum() + abs(kc) * (w.abs() * e1.gather(1, li).view(-1)).sum()
    mr = (p1 + p2) / 2
    m = mr.clamp(1e-7, 1.0)
    lm = torch.log(m)
    t1, s1 = _xlogy_abs(p1, lm)
    t2, s2 = _xlogy_abs(p2, lm)
    js, Sj = ((t1 + t2) / 2).sum(), ((s1 + s2) / 2).sum()
    sg = abs(kj) * (((e1 * p1 * (torch.log(p1.clamp_min(1e-300)).abs() + lm.abs() + 2.0)) +
                     (e2 * p2 * (torch.log(p2.clamp_min(1e-300)).abs() + lm.abs() + 2.0))) / 2).sum()
    vals = torch.stack([ce + kj * js, ce, kj * js])
    S = torch.stack([Sce + abs(kj) * Sj, Sce, abs(kj) * Sj])
    named = torch.stack([sg, torch.zeros_like(sg), sg])
    if g0 is None:
        return vals, S, named
    gd1, sd1 = _dterm(p1, p2, mr, m, lm)
    gd2, sd2 = _dterm(p2, p1, mr, m, lm)
    dot1, sdot1 = (p1 * gd1).sum(1, keepdim=True), (p1 * sd1).sum(1, keepdim=True)
    dot2, sdot2 = (p2 * gd2).sum(1, keepdim=True), (p2 * sd2).sum(1, keepdim=True)
    onehot = torch.zeros_like(p1).scatter_(1, li, 1.0) * valid.view(-1, 1)
    w = w.view(-1, 1)
    r = torch.cat([g0 * (kc * w * (p1 - onehot) + kj * p1 * (gd1 - dot1)), g0 * kj * p2 * (gd2 - dot2)])
    Sg = abs(g0) * torch.cat([abs(kc) * w.abs() * (p1 + onehot) + abs(kj) * p1 * (sd1 + sdot1), abs(kj) * p2 * (sd2 + sdot2)])
    E = abs(g0) * torch.cat([e1 * p1 * (abs(kc) * w.abs() + abs(kj) * ((gd1 - dot1).abs() + 2.0)),
                             e2 * p2 * abs(kj) * ((gd2 - dot2).abs() + 2.0)])
    return vals, S, named, (r, Sg, E)


def roi_reg_expect(bbox_pred, labels, targets, weights, C, reg_limit, beta, avg, lw):
    """fp64 (loss, S) of the RoI box loss: SmoothL1 (beta > 0) / L1 of the class-specific deltas of rows < reg_limit with a
    label in [0, C)"""
    p = bbox_pred.detach().to(torch.float64)
    K, n_reg = p.shape
    lab = labels.view(-1)
    pos = (torch.arange(K, device=p.device) < reg_limit) & (lab >= 0) & (lab < C)
    col = (lab.clamp(0, C - 1) * 4 if n_reg != 4 else torch.zeros_like(lab)).view(-1, 1) + torch.arange(4, device=p.device)
    pr = p.gather(1, col)
    t, w = targets.to(torch.float64), weights.to(torch.float64)
    d = (pr - t).abs()
    e = torch.where(d < beta, 0.5 * d * d / beta, d - 0.5 * beta) if beta > 0 else d
    Se = torch.where(d < beta, 0.5 * (pr.abs() + t.abs()) ** 2 / beta, pr.abs() + t.abs() + 0.5 * beta) if beta > 0 \
        else pr.abs() + t.abs()
    m = pos.to(torch.float64).view(-1, 1)
    return lw * (e * w * m).sum() / avg, abs(lw) * (Se * w.abs() * m).sum() / avg


def roi_reg_grad_expect(bbox_pred, labels, targets, weights, C, reg_limit, beta, avg, lw, g):
    p = bbox_pred.detach().to(torch.float64)
    K, n_reg = p.shape
    lab = labels.view(-1)
    pos = (torch.arange(K, device=p.device) < reg_limit) & (lab >= 0) & (lab < C)
    col = (lab.clamp(0, C - 1) * 4 if n_reg != 4 else torch.zeros_like(lab)).view(-1, 1) + torch.arange(4, device=p.device)
    d = p.gather(1, col) - targets.to(torch.float64)
    de = torch.where(d.abs() < beta, d / beta, torch.sign(d)) if beta > 0 else torch.sign(d)
    v = (g * lw / avg) * weights.to(torch.float64) * de * pos.to(torch.float64).view(-1, 1)
    r = torch.zeros_like(p).scatter_(1, col, v)
    return r, r.abs()


def top1_first(cls_score, labels):
    """(rows whose FIRST maximum is the label - the kernel's strict ``v > best`` scan -, rows whose top two logits tie)"""
    s = cls_score.detach().to(torch.float64)
    lab = labels.view(-1)
    at_max = s == s.max(1, keepdim=True)[0]
    first = at_max & (at_max.cumsum(1) == 1)
    arg = (first * torch.arange(s.shape[1], device=s.device)).sum(1)
    return int((arg == lab).sum()), int((at_max.sum(1) > 1).sum())


def twin_index(B, ori, rp, device):
    """oracle/losses.py twin_index on the device"""
    i = torch.arange(B, device=device)
    t = torch.full((B,), -1, dtype=torch.long, device=device)
    t = torch.where(i < ori, i + ori, t)
    t = torch.where((i >= ori) & (i < 2 * ori), i - ori, t)
    j = i - 2 * ori
    t = torch.where((j >= 0) & (j < rp), i + rp, t)
    t = torch.where((j >= rp) & (j < 2 * rp), i - rp, t)
    return t


def supcon_expect(feats, labels, ori, rp, temper, min_samples, lw, g=None):
    """fp64 supcon (oracle/losses.py supcon on the device): (loss, S) and with ``g`` the gradient (r, S) [B, D]"""
    x = feats.detach().to(torch.float64).clone()
    B = x.shape[0]
    lab = labels.view(-1)
    if lab.numel() != B:
        lab = torch.cat([lab, lab[-1:].repeat(B - lab.numel())])
    bg = lab.max()
    if int((lab != bg).sum()) <= min_samples:
        z = torch.zeros((), dtype=torch.float64, device=x.device)
        return (z, z) if g is None else (z, z, torch.zeros_like(x), torch.zeros_like(x))
    x.requires_grad_(g is not None)
    with torch.enable_grad():
        f = F.normalize(F.normalize(x, dim=1), dim=1)
        Sm = f @ f.t() / temper
        L = Sm - Sm.max(dim=1, keepdim=True)[0].detach()
        eye = torch.eye(B, dtype=torch.bool, device=x.device)
        fg = lab != bg
        same = lab.view(-1, 1) == lab.view(1, -1)
        P = same & fg.view(-1, 1) & fg.view(1, -1) & ~eye
        tw = twin_index(B, ori, rp, x.device)
        twin = torch.zeros(B, B, dtype=torch.bool, device=x.device)
        has = tw >= 0
        twin[torch.arange(B, device=x.device)[has], tw[has]] = True
        P = (P | (twin & (~fg).view(-1, 1) & (~fg).view(1, -1))).to(torch.float64)
        logZ = torch.log((torch.exp(L) * (~eye).to(torch.float64)).sum(1, keepdim=True))
        lp = L - logZ
        npos = P.sum(1)
        per_row = (P * lp).sum(1) / (npos + 1e-8)
        loss = lw * (-per_row).mean()
    with torch.no_grad():
        S_loss = abs(lw) * ((P * (L.abs() + logZ.abs())).sum(1) / (npos + 1e-8)).mean()
    if g is None:
        return loss.detach(), S_loss
    loss.backward(torch.as_tensor(float(g), dtype=torch.float64, device=x.device))
    with torch.no_grad():
        # |d loss / d S_ij| (positives and the softmax), through S = f f^T / T and the two normalisations
        sm = torch.softmax(L.masked_fill(eye, float('-inf')), 1)
        M = abs(lw * float(g)) / B * (P + npos.view(-1, 1) * sm) / (npos.view(-1, 1) + 1e-8)
        fa = f.abs()
        Sf = (M @ fa + M.t() @ fa) / temper
        Sx = 2 * (Sf + fa * (fa * Sf).sum(1, keepdim=True)) / x.detach().norm(dim=1, keepdim=True)
    return loss.detach(), S_loss, x.grad.detach(), Sx


# ----------------------------------------------------------------------------------------------------------- auditor
class Row:
    __slots__ = ('calls', 'shapes', 'worst', 'where')

    def __init__(self):
        self.calls, self.shapes, self.worst, self.where = 0, set(), 0.0, None


class Auditor:
    def __init__(self):
        self.table = {}
        self.wrappers = {}
        self.kernels = set()
        self.failures = []
        self.borderline = {}         # family -> [carved-out elements, elements checked]
        self.info = {}               # path facts of the audited launches (RoIAlign group sizes, bin widths)
        self.lin_src = {}            # data_ptr of a bf16 weight / bias copy -> (fp32 parameter, (C, P) of a permuted one)
        self.lin_acc = {}            # id(parameter) -> [parameter, fp64 gradient, S, rounding terms, calls]

    def hit(self, wrapper):
        self.wrappers[wrapper] = self.wrappers.get(wrapper, 0) + 1

    def count(self, family, carved, total):
        c = self.borderline.setdefault(family, [0, 0])
        c[0] += int(carved)
        c[1] += int(total)

    def record(self, kernel, shape, o, ref, b, check=None, launched=True):
        rt, i = ratio(o, ref, b)
        if launched:
            self.kernels.add(kernel)
        kernel = kernel if check is None else '%s %s' % (kernel, check)
        row = self.table.setdefault(kernel, Row())
        row.calls += 1
        row.shapes.add(tuple(shape))
        if o.numel() and (rt > row.worst or row.where is None):
            row.worst = max(rt, row.worst)
            row.where = (tuple(shape), i, float(o.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(b.reshape(-1)[i]))
        if not rt <= 1.0:
            self.failures.append((kernel, tuple(shape), rt, row.where))
        return rt

    def exact(self, kernel, shape, ok, check=None, launched=True):
        z = torch.zeros(1, dtype=torch.float64)
        return self.record(kernel, shape, z, z + (0.0 if ok else 1.0), torch.full((1,), ALPHA, dtype=torch.float64),
                           check=check, launched=launched)

    def worst(self):
        return max((r.worst for r in self.table.values()), default=0.0)

    def print_table(self, title):
        print('\n== head audit: %s ==' % title)
        print('%-62s %6s %10s  %s' % ('kernel', 'calls', 'err/bound', 'worst element (shape, index, out, ref, bound)'))
        for k in sorted(self.table):
            r = self.table[k]
            print('%-62s %6d %10.4f  %s' % (k, r.calls, r.worst, r.where))
        print('borderline (carved out, checked):', self.borderline)
        print('wrappers:', dict(sorted(self.wrappers.items())))
        print('paths:', self.info)

    # -- installation
    def install_sgd(self, mp, model=None):
        from oadg_amd import _lib, apis
        A = self
        orig = apis.FusedSGD.step
        launches = []
        chk = _lib.check

        def check(rc, what):
            # (FusedSGD.step reports its launch through _lib.check(..., 'oadg_sgd_step_multi'); its fall-back to
            #  torch.optim.SGD.step does not)
            launches.append(what)
            return chk(rc, what)
        mp.setattr(_lib, 'check', check)

        def step(opt, closure=None):
            A.hit('FusedSGD.step')
            snap = A._sgd_snapshot(opt, model)
            del launches[:]
            out = orig(opt, closure)
            torch.cuda.synchronize()
            groups = sum(1 for g in opt.param_groups if any(p.grad is not None for p in g['params']))
            A._check_sgd(opt, snap, model, fused=launches.count('oadg_sgd_step_multi') == groups > 0)
            return out
        mp.setattr(apis.FusedSGD, 'step', step)
        return self

    def install(self, mp, model=None, sgd=True):
        from oadg_amd import hip_ops
        self.ho = hip_ops
        A = self
        sync = torch.cuda.synchronize

        def nograd(fn):
            def g(*a, **k):
                with torch.no_grad(), torch.autocast('cuda', enabled=False):
                    return fn(*a, **k)
            return g

        # RoIAlign
        rf, rb, dep = hip_ops._RoIAlignFPN.forward, hip_ops._RoIAlignFPN.backward, hip_ops._deposit
        captured = []

        def roi_forward(ctx, rois, out_size, scales, finest_scale, sampling_ratio, aligned, tokens, *feats):
            A.hit('_RoIAlignFPN.forward')
            out = rf(ctx, rois, out_size, scales, finest_scale, sampling_ratio, aligned, tokens, *feats)
            sync()
            ctx._audit = nograd(A._check_roi_fwd)(rois, out_size, scales, finest_scale, sampling_ratio, aligned, feats, out)
            return out

        def deposit(tokens, grads):
            captured.append(list(grads))
            return dep(tokens, grads)

        def roi_backward(ctx, gout):
            A.hit('_RoIAlignFPN.backward')
            del captured[:]
            outs = rb(ctx, gout)
            sync()
            nograd(A._check_roi_bwd)(ctx, gout, captured[-1])
            return outs
        mp.setattr(hip_ops._RoIAlignFPN, 'forward', staticmethod(roi_forward))
        mp.setattr(hip_ops._RoIAlignFPN, 'backward', staticmethod(roi_backward))
        mp.setattr(hip_ops, '_deposit', deposit)

        # fused RPN loss
        pf, pb = hip_ops._RpnLoss.forward, hip_ops._RpnLoss.backward

        def rpn_forward(ctx, A_, targets, avg, w_cls, lam, w_box, *ys):
            A.hit('_RpnLoss.forward')
            outs = pf(ctx, A_, targets, avg, w_cls, lam, w_box, *ys)
            sync()
            nograd(A._check_rpn_fwd)(A_, targets, avg, w_cls, lam, w_box, ys, outs)
            return outs

        def rpn_backward(ctx, g_cls, g_box, _g):
            A.hit('_RpnLoss.backward')
            outs = pb(ctx, g_cls, g_box, _g)
            sync()
            nograd(A._check_rpn_bwd)(ctx, g_cls, g_box, outs[6:])
            return outs
        mp.setattr(hip_ops._RpnLoss, 'forward', staticmethod(rpn_forward))
        mp.setattr(hip_ops._RpnLoss, 'backward', staticmethod(rpn_backward))

        # RoI head CE + JSD (and the per-level RPN path when it runs)
        cf, cb = hip_ops._CeJsd.forward, hip_ops._CeJsd.backward

        def ce_forward(ctx, logits, labels, weights, mode, avg, lw, lam):
            A.hit('_CeJsd.forward')
            outs = cf(ctx, logits, labels, weights, mode, avg, lw, lam)
            sync()
            nograd(A._check_ce_fwd)(logits, labels, weights, mode, avg, lw, lam, outs)
            return outs

        def ce_backward(ctx, gout, gp):
            A.hit('_CeJsd.backward')
            outs = cb(ctx, gout, gp)
            sync()
            logits, labels, weights = ctx.saved_tensors
            R, C, mode, avg, lw, lam = ctx.args
            nograd(A._check_ce_bwd)(logits, labels, weights, mode, avg, lw, lam, gout, outs[0])
            return outs
        mp.setattr(hip_ops._CeJsd, 'forward', staticmethod(ce_forward))
        mp.setattr(hip_ops._CeJsd, 'backward', staticmethod(ce_backward))

        # RoI box loss + accuracy
        gf, gbk = hip_ops._RoiRegAcc.forward, hip_ops._RoiRegAcc.backward

        def reg_forward(ctx, bbox_pred, cls_score, labels, targets, weights, C, reg_limit, beta, avg, lw):
            A.hit('_RoiRegAcc.forward')
            outs = gf(ctx, bbox_pred, cls_score, labels, targets, weights, C, reg_limit, beta, avg, lw)
            sync()
            nograd(A._check_reg_fwd)(bbox_pred, cls_score, labels, targets, weights, C, reg_limit, beta, avg, lw, outs)
            return outs

        def reg_backward(ctx, g, gacc):
            A.hit('_RoiRegAcc.backward')
            outs = gbk(ctx, g, gacc)
            sync()
            bp, labels, targets, weights = ctx.saved_tensors
            C, reg_limit, beta, avg, lw, _ = ctx.cfg
            nograd(A._check_reg_bwd)(bp, labels, targets, weights, C, reg_limit, beta, avg, lw, g, outs[0])
            return outs
        mp.setattr(hip_ops._RoiRegAcc, 'forward', staticmethod(reg_forward))
        mp.setattr(hip_ops._RoiRegAcc, 'backward', staticmethod(reg_backward))

        # supcon
        sf, sbk = hip_ops._SupCon.forward, hip_ops._SupCon.backward

        def sc_forward(ctx, feats, labels, n_labels, ori, rp, temper, min_samples, lw):
            A.hit('_SupCon.forward')
            out = sf(ctx, feats, labels, n_labels, ori, rp, temper, min_samples, lw)
            sync()
            ctx._audit_in = (feats.detach().float().contiguous(), labels.detach().view(-1).long(), min_samples)
            nograd(A._check_supcon)(ctx._audit_in[0], ctx._audit_in[1], ori, rp, temper, min_samples, lw, out, None, None)
            return out

        def sc_backward(ctx, gout):
            A.hit('_SupCon.backward')
            outs = sbk(ctx, gout)
            sync()
            feats, labels, min_samples = ctx._audit_in
            B, D, n_labels, ori, rp, temper, lw, _ = ctx.args
            nograd(A._check_supcon)(feats, labels, ori, rp, temper, min_samples, lw, None, gout, outs[0])
            return outs
        mp.setattr(hip_ops._SupCon, 'forward', staticmethod(sc_forward))
        mp.setattr(hip_ops._SupCon, 'backward', staticmethod(sc_backward))

        # _parse_losses
        lf = hip_ops._ParseLosses.forward

        def parse_forward(ctx, name_of, n_names, mask, *vals):
            A.hit('_ParseLosses.forward')
            outs = lf(ctx, name_of, n_names, mask, *vals)
            sync()
            nograd(A._check_parse)(name_of, n_names, mask, vals, outs)
            return outs
        mp.setattr(hip_ops._ParseLosses, 'forward', staticmethod(parse_forward))

        # the RoI head's bf16 casts and column permutation
        kf, kb = hip_ops._CastAll.forward, hip_ops._CastAll.backward

        def cast_forward(ctx, *params):
            A.hit('_CastAll.forward')
            outs = kf(ctx, *params)
            sync()
            for o, p in zip(outs, params):
                A.lin_src[o.data_ptr()] = (p, None)
            ok = all(torch.equal(o, p.detach().to(torch.bfloat16)) for o, p in zip(outs, params))
            A.exact('cast_all_bf16 (foreach copy)', (len(params),), ok, launched=False)
            return outs

        def cast_backward(ctx, *grads):
            A.hit('_CastAll.backward')
            outs = kb(ctx, *grads)
            sync()
            ok = all((g is None and o is None) or torch.equal(o, g.float()) for o, g in zip(outs, grads))
            A.exact('cast_all_bf16 (foreach copy)', (len(grads),), ok, check='backward', launched=False)
            return outs
        mp.setattr(hip_ops._CastAll, 'forward', staticmethod(cast_forward))
        mp.setattr(hip_ops._CastAll, 'backward', staticmethod(cast_backward))
        wf, wb = hip_ops._FcWeightPermute.forward, hip_ops._FcWeightPermute.backward

        def perm_forward(ctx, w, C, P):
            A.hit('_FcWeightPermute.forward')
            out = wf(ctx, w, C, P)
            sync()
            A.lin_src[out.data_ptr()] = (w, (C, P))
            O = w.shape[0]
            ref = w.detach().view(O, C, P).permute(0, 2, 1).reshape(O, P * C).to(torch.bfloat16)
            A.exact('fc_weight_permute_kernel', tuple(w.shape), torch.equal(out, ref))
            return out

        def perm_backward(ctx, g):
            A.hit('_FcWeightPermute.backward')
            outs = wb(ctx, g)
            sync()
            O, C, P = ctx.meta
            ref = g.detach().to(torch.bfloat16).float().view(O, P, C).permute(0, 2, 1).reshape(O, C * P)
            sink = ctx.param is not None and A._in_sink(ctx.param, outs[0])
            A.exact('fc_weight_permute_kernel', (O, C * P), torch.equal(outs[0], ref),
                    check='backward (grad_dest slice)' if sink else 'backward')
            return outs
        mp.setattr(hip_ops._FcWeightPermute, 'forward', staticmethod(perm_forward))
        mp.setattr(hip_ops._FcWeightPermute, 'backward', staticmethod(perm_backward))
        lb = hip_ops.linear_bias_grad

        def linear_bias_grad(x, w, b, relu=False):
            A.hit('linear_bias_grad')
            y = lb(x, w, b, relu)
            if y.requires_grad and not (A.lin_src.get(w.data_ptr()) is None and x.dtype == torch.float32):
                # (an fp32 step casts and permutes nothing: its linears are the library's on the parameters themselves, no
                #  launch of this project's - nothing to map a gradient back through)
                # the operands of this linear's weight / bias gradient: x, and bf16(dy) * (y > 0) - observed by a hook
                # on y, which returns nothing (the gradient flows on unchanged)
                src_w, src_b = A.lin_src.get(w.data_ptr()), A.lin_src.get(b.data_ptr()) if b is not None else None
                xs, ys = x.detach(), y.detach() if relu else None

                def hook(gy):
                    nograd(A._linear_ref)(src_w, src_b, xs, ys, gy)
                y.register_hook(hook)
            return y
        mp.setattr(hip_ops, 'linear_bias_grad', linear_bias_grad)
        if sgd and 'FusedSGD.step' not in self.wrappers:
            self.install_sgd(mp, model)
        return self

    def _in_sink(self, param, t):
        sink = self.ho.GRAD_SINK
        v = sink.get(param) if sink is not None else None
        return v is not None and v.data_ptr() == t.data_ptr()

    # -- per-launch checks
    def _check_roi_fwd(self, rois, out_size, scales, finest_scale, sampling_ratio, aligned, feats, out):
        PH, PW = out_size
        shapes = [tuple(f.shape) for f in feats]
        dt = feats[0].dtype
        rois = rois.detach().float()
        K, C = rois.shape[0], shapes[0][1]
        name = 'roi_align_fwd_rows_kernel<%s>' % ('float' if dt == torch.float32 else 'unsigned short')
        rho = RHO if dt == torch.bfloat16 else 0.0
        lvl, geo, near = roi_setup(rois, shapes, scales, finest_scale, PH, PW, sampling_ratio, aligned)
        o = out.detach().permute(0, 2, 3, 1).to(torch.float64)
        r, S, S4 = roi_align_ref(feats, rois, lvl, geo, PH, PW)
        b = bound(r, S, rho, GAMMA_ROI, POS_ERR * S4)
        chosen = torch.zeros(K, dtype=torch.long, device=rois.device)
        variants = {0: (lvl, geo)}
        if bool(near.any()):
            # borderline RoIs: the other side of each choice; per RoI the variant the launch matches
            best = ((o[near] - r[near]).abs() / b[near]).flatten(1).max(1)[0]
            r0, b0 = r[near].clone(), b[near].clone()
            differ = torch.zeros_like(r0, dtype=torch.bool)
            for s in (-1, 1):
                l2, g2, _ = roi_setup(rois, shapes, scales, finest_scale, PH, PW, sampling_ratio, aligned, s)
                variants[s] = (l2, g2)
                r2, S2, S42 = roi_align_ref(feats, rois, l2, g2, PH, PW, sel=near)
                b2 = bound(r2, S2, rho, GAMMA_ROI, POS_ERR * S42)
                differ |= (r2[near] - r0).abs() > b0
                e2 = ((o[near] - r2[near]).abs() / b2[near]).flatten(1).max(1)[0]
                # the other side only where the fp64 side does not hold
                take = (e2 < best) & (best > 1.0)
                best = torch.where(take, e2, best)
                ni = torch.nonzero(near).view(-1)[take]
                chosen[ni] = s
                r[ni], b[ni] = r2[ni], b2[ni]
            # carved out: the elements of the RoIs that took the other side, where the two sides differ
            used = chosen[near] != 0
            self.count('roi_align', int((differ & used.view(-1, 1, 1, 1)).sum()), o.numel())
            self.info['roi_near'] = self.info.get('roi_near', 0) + int(near.sum())
            self.info['roi_other_side'] = self.info.get('roi_other_side', 0) + int(used.sum())
        else:
            self.count('roi_align', 0, o.numel())
        self.record(name, (K, C, PH, PW) + tuple(s[2] for s in shapes), o, r, b)
        # path facts: the largest (level, image) group and the widest bin
        g = lvl * shapes[0][0] + geo['batch'].clamp(0, shapes[0][0] - 1)
        if K:
            self.info['max_group'] = max(self.info.get('max_group', 0), int(torch.bincount(g).max()))
            self.info['max_bin'] = max(self.info.get('max_bin', 0.0), float(torch.maximum(geo['bh'], geo['bw']).max()))
        return dict(chosen=chosen, variants=variants, name=name)

    def _check_roi_bwd(self, ctx, gout, grads):
        rois, order, rng = ctx.saved_tensors
        shapes, dt, scales, finest_scale, sampling_ratio, aligned, (PH, PW) = ctx.meta
        aud = ctx._audit
        N = shapes[0][0]
        rois = rois.detach().float()
        K = rois.shape[0]
        tiles = rng.numel() > 0 and order.numel() > 0
        if order.numel():
            # the launch's processing order (oadg_roi_order / the key sort): a stable sort of the keys, group boundaries
            ok, klvl, nb = check_order(rois, N, len(shapes), finest_scale, order, rng if rng.numel() else None)
            self.exact('roi_order_rank_kernel' if K <= 8192 else 'roi_order_key_kernel', (K,), ok, check='order / range')
            self.count('roi_order', nb, K)
            if ok:
                self.info['order_level_agrees'] = bool(torch.equal(klvl, self._fwd_levels(aud)))
        name = 'roi_align_bwd_tiles_kernel' if tiles else 'roi_align_bwd_kernel'
        if tiles:
            self.kernels.add('roi_tile_box_kernel')
        rho = RHO if dt == torch.bfloat16 else 0.0
        # per RoI the geometry the forward matched (a borderline level / count / drop is decided once, by the forward)
        lvl = self._fwd_levels(aud)
        geo = dict(aud['variants'][0][1])
        ch = aud['chosen']
        for s in (-1, 1):
            if s in aud['variants']:
                m = ch == s
                g2 = aud['variants'][s][1]
                for k in ('sh', 'sw', 'bh', 'bw', 'gh', 'gw', 'count', 'batch', 'H', 'W'):
                    geo[k] = torch.where(m, g2[k], geo[k])
        # (the shift of a borderline drop follows the chosen variant per RoI: evaluate the two shifted sets separately)
        refs = None
        for s in sorted(set(ch.tolist())):
            sub = dict(geo, shift=s)
            sub['gh'] = torch.where(ch == s, geo['gh'], torch.zeros_like(geo['gh']))      # (only this variant's RoIs)
            part = roi_align_bwd_ref(shapes, rois, lvl, sub, gout, PH, PW)
            refs = part if refs is None else [[a + b_ for a, b_ in zip(x, y)] for x, y in zip(refs, part)]
        for l, (g, (r, S, S4)) in enumerate(zip(grads, refs)):
            o = g.detach().permute(0, 2, 3, 1).to(torch.float64)
            self.record(name, (K,) + tuple(shapes[l]), o, r, bound(r, S, rho, GAMMA_ROI, POS_ERR * S4),
                        check='(level %d)' % l if len(shapes) > 1 else None)

    @staticmethod
    def _fwd_levels(aud):
        lvl = aud['variants'][0][0].clone()
        for s in (-1, 1):
            if s in aud['variants']:
                m = aud['chosen'] == s
                lvl[m] = aud['variants'][s][0][m]
        return lvl

    def _check_rpn_fwd(self, A_, targets, avg, w_cls, lam, w_box, ys, outs):
        vals, S, named = rpn_loss_expect(ys, A_, targets, avg, w_cls, lam, w_box)
        name = self._rpn_kernel(A_, ys, targets[2], targets[3], False)
        self.kernels.add('rpn_loss_fin_kernel')
        parts = outs[2]
        self.record(name, (len(ys),) + tuple(ys[0].shape), parts.double(), vals, bound(vals, S, 0.0, GAMMA_LOSS, named),
                    check='parts')
        got = torch.stack([outs[0], outs[1]]).double()
        ref = torch.stack([vals[0], vals[3]])
        self.record(name, (len(ys),), got, ref, bound(ref, torch.stack([S[0], S[3]]), 0.0, GAMMA_LOSS,
                                                      torch.stack([named[0], named[3]])), check='returned losses')

    @staticmethod
    def _rpn_kernel(A_, ys, bbox_t, bbox_w, bwd):
        """the instantiation csrc oadg_rpn_loss_fwd / _bwd dispatch to for these operands (rpn_loss_fast3, the 16-byte
        alignment of the box targets / weights, and the backward's cooperative-store condition)"""
        bf = ys[0].dtype == torch.bfloat16
        fast3 = A_ == 3 and bf and all(
            y.stride(1) == 1 and y.shape[1] >= 16 and y.stride(0) % 8 == 0 and y.stride(2) % 8 == 0 and
            y.stride(3) % 8 == 0 and y.data_ptr() % 16 == 0 for y in ys) and \
            bbox_t.data_ptr() % 16 == 0 and bbox_w.data_ptr() % 16 == 0
        if not bwd:
            return 'rpn_loss_fwd_kernel<%d>' % (3 if fast3 else 0)
        nz = (5 * A_ + 7) & ~7
        coop = 256 * nz * (2 if bf else 4) <= 48 * 1024 and all(y.shape[1] == ys[0].shape[1] for y in ys)
        return 'rpn_loss_bwd_kernel<%s, %d>' % ('true' if coop else 'false', 3 if coop and fast3 else 0)

    def _check_rpn_bwd(self, ctx, g_cls, g_box, gys):
        labels, label_w, bbox_t, bbox_w, *ys = ctx.saved_tensors
        A_, avg, w_cls, lam, w_box = ctx.args
        gc = float(g_cls) if g_cls is not None else 0.0
        gb = float(g_box) if g_box is not None else 0.0
        refs = rpn_grad_expect(ys, A_, (labels, label_w, bbox_t, bbox_w), avg, w_cls, lam, w_box, gc, gb)
        name = self._rpn_kernel(A_, ys, bbox_t, bbox_w, True)
        rho = RHO if ys[0].dtype == torch.bfloat16 else 0.0
        B2 = ys[0].shape[0] // 2
        for l, (g, (r, S, E)) in enumerate(zip(gys, refs)):
            o = g.detach().permute(0, 2, 3, 1).to(torch.float64)
            self.record(name, tuple(g.shape), o, r, bound(r, S, rho, GAMMA_LOSS, E), check='(level %d)' % l)
            # channels >= 5A and the view-2 delta channels: exactly zero
            z = bool((o[..., 5 * A_:] == 0).all()) and bool((o[B2:, ..., A_:5 * A_] == 0).all())
            self.exact(name, tuple(g.shape), z, check='zero channels')

    def _check_ce_fwd(self, logits, labels, weights, mode, avg, lw, lam, outs):
        vals, S, named = ce_jsd_expect(logits, labels, weights, mode, avg, lw, lam)
        name = 'sig_kernel<false>' if mode == 0 else 'sm_kernel<false>'
        self.kernels.add('cls_fin_kernel')
        self.record(name, tuple(logits.shape), outs[1].double(), vals, bound(vals, S, 0.0, GAMMA_LOSS, named), check='parts')
        self.record(name, tuple(logits.shape), outs[0].double().view(1), vals[:1],
                    bound(vals[:1], S[:1], 0.0, GAMMA_LOSS, named[:1]), check='total')

    def _check_ce_bwd(self, logits, labels, weights, mode, avg, lw, lam, gout, d):
        g0 = float(gout)
        _, _, _, (r, S, E) = ce_jsd_expect(logits, labels, weights, mode, avg, lw, lam, g0)
        name = 'sig_kernel<true>' if mode == 0 else 'sm_kernel<true>'
        self.record(name, tuple(logits.shape), d.double().view(r.shape), r, bound(r, S, 0.0, GAMMA_LOSS, E))

    def _check_reg_fwd(self, bbox_pred, cls_score, labels, targets, weights, C, reg_limit, beta, avg, lw, outs):
        loss, S = roi_reg_expect(bbox_pred, labels, targets, weights, C, reg_limit, beta, avg, lw)
        name = 'roi_reg_acc_fwd_kernel'
        self.record(name, tuple(bbox_pred.shape), outs[0].double().view(1), loss.view(1),
                    bound(loss.view(1), S.view(1), 0.0, GAMMA_LOSS), check='loss')
        if cls_score is not None:
            K = labels.numel()
            hits, ties = top1_first(cls_score, labels)
            # out[1] = (float)hits * (100.0f / (float)K), exactly (bf16 / fp32 logits compare exactly in fp64)
            want = torch.tensor(float(hits), dtype=torch.float32) * (torch.tensor(100.0, dtype=torch.float32) /
                                                                     torch.tensor(float(max(K, 1)), dtype=torch.float32))
            self.exact(name, (K,), float(outs[1].view(-1)[0]) == float(want), check='accuracy')
            self.info['accuracy_ties'] = self.info.get('accuracy_ties', 0) + ties

    def _check_reg_bwd(self, bp, labels, targets, weights, C, reg_limit, beta, avg, lw, g, grad):
        r, S = roi_reg_grad_expect(bp, labels, targets, weights, C, reg_limit, beta, avg, lw, float(g))
        rho = RHO if bp.dtype == torch.bfloat16 else 0.0
        o = grad.double()
        self.record('roi_reg_bwd_kernel', tuple(bp.shape), o, r, bound(r, S, rho, GAMMA_LOSS))
        self.exact('roi_reg_bwd_kernel', tuple(bp.shape), bool((o[r == 0] == 0).all()), check='zeros')

    def _check_supcon(self, feats, labels, ori, rp, temper, min_samples, lw, out, gout, dfeats):
        if gout is None:
            loss, S = supcon_expect(feats, labels, ori, rp, temper, min_samples, lw)
            self.kernels.update({'supcon_prep_kernel', 'supcon_tile_kernel<false>'})
            self.record('supcon_fin_kernel', tuple(feats.shape), out.double().view(1), loss.view(1),
                        bound(loss.view(1), S.view(1), 0.0, GAMMA_LOSS))
        else:
            _, _, r, S = supcon_expect(feats, labels, ori, rp, temper, min_samples, lw, float(gout))
            self.kernels.add('supcon_tile_kernel<true>')
            self.record('supcon_bwd_fin_kernel', tuple(feats.shape), dfeats.double(), r, bound(r, S, 0.0, GAMMA_LOSS))

    def _check_parse(self, name_of, n_names, mask, vals, outs):
        total, packed = outs
        v = torch.stack([x.detach().double().view(-1)[0] for x in vals])
        s = torch.zeros(n_names, dtype=torch.float64, device=v.device)
        Sa = torch.zeros_like(s)
        idx = torch.tensor(list(name_of), dtype=torch.long, device=v.device)
        s.index_add_(0, idx, v)
        Sa.index_add_(0, idx, v.abs())
        m = torch.tensor([(mask >> i) & 1 for i in range(n_names)], dtype=torch.float64, device=v.device)
        tot, St = (s * m).sum().view(1), (Sa * m).sum().view(1)
        ref = torch.cat([s, tot])
        S = torch.cat([Sa, St])
        self.record('parse_losses_kernel', (len(vals), n_names), packed.double(), ref, bound(ref, S, 0.0, GAMMA_LOSS),
                    check='packed')
        self.record('parse_losses_kernel', (len(vals), n_names), total.double().view(1), tot, bound(tot, St, 0.0, GAMMA_LOSS),
                    check='total')

    # -- RoI head parameters
    def _linear_ref(self, src_w, src_b, x, y, gy):
        """fp64 g^T x and column sums of g = bf16(gy) * (y > 0) for one call, accumulated per parameter; the weight gradient
        of a permuted weight (hip_ops._FcWeightPermute: column p C + c) is taken back to the parameter's c P + p order"""
        g = gy.detach().to(torch.bfloat16).to(torch.float64)
        if y is not None:
            g = g * (y > 0)
        x64 = x.reshape(x.shape[0], -1).to(torch.float64)
        for src, ref, S in ((src_w, g.t() @ x64, g.abs().t() @ x64.abs()), (src_b, g.sum(0), g.abs().sum(0))):
            if src is None:
                continue
            p, perm = src
            if perm is not None:
                C, P = perm
                O = ref.shape[0]
                ref = ref.view(O, P, C).permute(0, 2, 1).reshape(O, C * P)
                S = S.view(O, P, C).permute(0, 2, 1).reshape(O, C * P)
            # the library GEMM / bias reduction hands the gradient over in bf16: one rounding per call
            acc = self.lin_acc.get(id(p))
            if acc is None:
                self.lin_acc[id(p)] = [p, ref, S, RHO * ref.abs(), 1]
            else:
                acc[1] += ref
                acc[2] += S
                acc[3] += RHO * ref.abs()
                acc[4] += 1

    def check_linear_params(self, named, prefix='roi_head.'):
        """compare the .grad of every parameter under ``prefix`` that a captured linear produced with the fp64 sum of its
        calls' g^T x / column sums; returns the names checked (the others under ``prefix`` are reported as failures)"""
        seen = set()
        with torch.no_grad():
            for n, p in named:
                if not (n.startswith(prefix) and p.requires_grad):
                    continue
                acc = self.lin_acc.get(id(p))
                if acc is None:
                    self.failures.append(('no linear call captured for', n))
                    continue
                seen.add(n)
                if p.grad is None:
                    self.failures.append(('param .grad missing', n))
                    continue
                _, ref, S, rnd, calls = acc
                extra = rnd + (RHO * ref.abs() if calls > 1 else 0.0)      # (a second call: autograd's bf16 sum)
                self.record('param .grad', (calls,) + tuple(p.shape), p.grad.double(), ref,
                            bound(ref, S, 0.0, GAMMA_GEMM, extra), check='(roi head linear)', launched=False)
        return seen

    # -- SGD
    def _sgd_snapshot(self, opt, model):
        snap = []
        for group in opt.param_groups:
            for p in group['params']:
                st = opt.state.get(p, {})
                b = st.get('momentum_buffer')
                snap.append((p, p.detach().clone(), None if p.grad is None else p.grad.detach().clone(),
                             None if b is None else b.detach().clone(), group))
        frozen = []
        if model is not None:
            frozen = [(n, p, p.detach().clone()) for n, p in model.named_parameters() if not p.requires_grad]
        return snap, frozen

    def _check_sgd(self, opt, snap, model, fused=True):
        """``fused``: the step launched oadg_sgd_step_multi for every group with gradients (else torch's SGD ran: the
        comparison then says nothing about the kernel, and it is recorded as not launched)"""
        entries, frozen = snap
        ok_p = ok_b = True
        n_first = n = 0
        for p, p0, g0, b0, group in entries:
            if g0 is None:
                ok_p &= torch.equal(p.detach(), p0)
                continue
            q = p0.clone().requires_grad_(False)
            ref = torch.optim.SGD([torch.nn.Parameter(q)], lr=group['lr'], momentum=group['momentum'],
                                  weight_decay=group['weight_decay'], dampening=group.get('dampening', 0),
                                  nesterov=group.get('nesterov', False))
            rp = ref.param_groups[0]['params'][0]
            rp.grad = g0.clone()
            if b0 is not None:
                ref.state[rp]['momentum_buffer'] = b0.clone()
            else:
                n_first += 1
            ref.step()
            n += 1
            ok_p &= torch.equal(p.detach(), rp.detach())
            ok_b &= torch.equal(opt.state[p]['momentum_buffer'], ref.state[rp]['momentum_buffer'])
        step = 'first step' if n_first == n else ('later step' if n_first == 0 else 'mixed')
        name = 'sgd_multi_kernel' if fused else 'torch.optim.SGD.step (fall-back)'
        self.exact(name, (n,), ok_p, check='p (%s)' % step, launched=fused)
        self.exact(name, (n,), ok_b, check='momentum (%s)' % step, launched=fused)
        self.info.setdefault('sgd_steps', []).append((step, n, 'fused' if fused else 'fall-back'))
        if model is not None:
            self.exact(name, (len(frozen),), all(torch.equal(p.detach(), p0) for _, p, p0 in frozen),
                       check='frozen unchanged', launched=False)
            names = {id(p): nm for nm, p in model.named_parameters() if p.requires_grad}
            stepped = {id(p) for p, _, g0, _, _ in entries if g0 is not None}
            self.info['sgd_missed'] = sorted(nm for i, nm in names.items() if i not in stepped)
