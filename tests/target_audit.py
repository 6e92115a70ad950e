"""Launch auditor of the integer / index half of a training step - what decides which rows the losses are computed ON:
the RPN's MaxIoU assignment over all anchors, the RandomSampler draws of the RPN (torch's CPU generator, replayed on the
host) and of the RoI head (the same generator replayed on the device), the anchor targets, the RoI proposals at training
settings (nms_pre 2000, padded lists), the RoI assignment with the gts added as proposals, rois / RoI targets and the
OA-Loss random proposals (numpy's global stream).  tests/conv_audit.py and tests/head_audit.py audit the arithmetic half
of the same step; tests/infer_audit.py the proposals at test time - its two wrappers run here unchanged.

Every wrapper takes the exact operands its launch received in the real step and recomputes the result with the pure
reference functions below: numpy / CPU torch restatements of the reference's source lines the kernels cite, NOT the tensor
path of oadg_amd.core.bbox (every other GPU test of these kernels already compares with that).  Everything is compared
bit for bit - IoUs in float32 in the operation order of iou2d_calculator.py, thresholds in float32 on both sides, draws
from a private torch.Generator / numpy RandomState set to the captured state, generator states afterwards - except the
encoded box deltas, where device logf and the divisions need not round as the CPU does::

    |o - r| <= GAMMA_T * S + ALPHA        r = the float64 recomputation, S = the same expression over absolute values

The CPU half of tests/test_target_audit.py ties every function to tests/golden/core_reference.npz and plants errors
(``plant=``: the named wrong answer, for those tests only).
"""
import numpy as np
import torch

import head_audit as HA
import infer_audit as IA

ALPHA = HA.ALPHA
# float32 arithmetic of encode_delta (csrc/targets.hip) and of the tensor path's bbox2delta: the two centres, their
# difference, the width, the division, the mean and the division by std - about six roundings of 2^-24 relative to S, 2^-21
# by derivation; logf and the ratio of widths likewise against (|log| + 1) / std.  Set from measurement against the float64
# reference: at 2^-21 the worst err / bound over the four audited steps and the stress launches of
# tests/test_target_audit.py is 0.287 (roi_targets_kernel in the short-image stress launch; the audited steps: 0.248 the
# host-sampler step at 256 x 512, 0.199 R50-FPN at 1024 x 2048, 0.115 multiscale, 0.122 DC5 - its anchor targets on the
# tensor path; 0.138 in the zero-size stress launch; the reference's own CPU float32 deltas in
# tests/golden/core_reference.npz reach 0.209).  2^-19 puts that worst at 0.072, a margin of 14x.
GAMMA_T = 2.0 ** -19
BORDERLINE_CAP = IA.BORDERLINE_CAP      # no carve-out is used here: Auditor.borderline stays empty

# the C-ABI calls this auditor answers for (closure test of tests/test_target_audit.py)
CLAIMS = {'oadg_max_iou_assign', 'oadg_host_randperm_prefix', 'oadg_sample_select', 'oadg_anchor_targets',
          'oadg_roi_assign_add_gt', 'oadg_roi_sample_device', 'oadg_roi_targets', 'oadg_roi_targets_dev',
          'oadg_np_random_bboxes'}
# encode_delta applies the fork's zero-size guard row by row; the reference pairs rows by position (gy[nan_x] = py[nan_y]).
# The two differ only for a positive with exactly one zero side.  Pinned by test_target_stress_zero_size_positives.
KNOWN_DEVIATION_ENCODE_DELTA = 'encode_delta: row-wise zero-size guard'


def _np(t, dtype=None):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    a = np.asarray(t)
    return a.astype(dtype) if dtype is not None and a.dtype != dtype else a


def same(a, b):
    """exact equality of two arrays (shape, every value; a NaN anywhere is a difference)"""
    a, b = _np(a), _np(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


# ----------------------------------------------------------------------------------------------------------- IoU, assign
def iou_expect(gts, boxes):
    """[G, N] float32 bbox_overlaps(gts, boxes, mode='iou', eps=1e-6) in the operation order of iou2d_calculator.py:
    area1 + area2 - overlap, clamped at eps, overlap / union - numpy float32, no contraction"""
    g, b = _np(gts, np.float32)[:, :4], _np(boxes, np.float32)[:, :4]
    G, N = g.shape[0], b.shape[0]
    if G * N == 0:
        return np.zeros((G, N), np.float32)
    a1 = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
    a2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    zero = np.float32(0)
    w = np.maximum(np.minimum(g[:, None, 2], b[None, :, 2]) - np.maximum(g[:, None, 0], b[None, :, 0]), zero)
    h = np.maximum(np.minimum(g[:, None, 3], b[None, :, 3]) - np.maximum(g[:, None, 1], b[None, :, 1]), zero)
    overlap = w * h
    union = np.maximum(a1[:, None] + a2[None, :] - overlap, np.float32(1e-6))
    return overlap / union


def assign_expect(boxes, valid, gts, labels, pos, neg_lo, neg_hi, min_pos, match_low_quality, plant=None):
    """max_iou_assigner.py:61-213 over the rows of ``boxes`` flagged ``valid`` (None: all) - the reference filters the
    others out before it assigns, so they take part in no maximum: (gt_inds [N] int64 with -1 on invalid rows,
    max_overlaps [N] float32 with NaN on invalid rows, labels [N] or None, (n_pos, n_neg)).  First argmax on ties; the
    low-quality loop runs in gt order, so later gts overwrite."""
    bx = _np(boxes, np.float32)[:, :4]
    g = _np(gts, np.float32).reshape(-1, 4)
    N, G = bx.shape[0], g.shape[0]
    ok = np.ones(N, bool) if valid is None else _np(valid).astype(bool)
    idx = np.nonzero(ok)[0]
    n = idx.size
    gi = np.full(n, -1, np.int64)
    if G == 0 or n == 0:
        mo = np.zeros(n, np.float32)
        if G == 0:
            gi[:] = 0                                                   # :131-134 no gt: everything is background
    else:
        ov = iou_expect(g, bx[idx])
        mo = ov.max(0)
        arg = ov.argmax(0)                                              # numpy: the first maximum
        if plant == 'last argmax':
            arg = G - 1 - ov[::-1].argmax(0)
        gmax = iou_expect(g, bx).max(1) if plant == 'padding row in a gt maximum' else ov.max(1)
        gi[(mo >= np.float32(neg_lo)) & (mo < np.float32(neg_hi))] = 0
        p = mo > np.float32(pos) if plant == '> for >=' else mo >= np.float32(pos)
        gi[p] = arg[p] + 1
        if match_low_quality:
            order = range(G - 1, -1, -1) if plant == 'low quality keeps the first gt' else range(G)
            for i in order:                                             # :195-201
                if gmax[i] >= np.float32(min_pos):
                    gi[ov[i] == gmax[i]] = i + 1
    gt_inds = np.full(N, -1, np.int64)
    gt_inds[idx] = gi
    max_ov = np.full(N, np.nan, np.float32)
    max_ov[idx] = mo
    lab = None
    if labels is not None:
        lab = np.full(N, -1, np.int64)
        gl = _np(labels, np.int64).reshape(-1)
        lab[gt_inds > 0] = gl[gt_inds[gt_inds > 0] - 1]
    return gt_inds, max_ov, lab, (int((gt_inds > 0).sum()), int((gt_inds == 0).sum()))


def add_gt_expect(boxes, gts, gt_labels, gt_inds, max_overlaps, labels, plant=None):
    """base_sampler.py:38-78 + assign_result.py add_gt_: the gts in front of the boxes, self-matched (gt_inds j + 1, their
    label, overlap 1): (boxes [G + N, 4], gt_inds, labels, max_overlaps, gt_flags)"""
    bx, g = _np(boxes, np.float32)[:, :4], _np(gts, np.float32).reshape(-1, 4)
    G = g.shape[0]
    parts = [(g, bx), (np.arange(1, G + 1, dtype=np.int64), _np(gt_inds, np.int64)),
             (_np(gt_labels, np.int64).reshape(-1), _np(labels, np.int64)),
             (np.ones(G, np.float32), _np(max_overlaps, np.float32)),
             (np.ones(G, np.uint8), np.zeros(bx.shape[0], np.uint8))]
    if plant == 'gts behind the proposals':
        parts = [(b, a) for a, b in parts]
    return tuple(np.concatenate(p) for p in parts)


# -------------------------------------------------------------------------------------------------------------- sampling
def sample_expect(gt_inds_list, num, pos_fraction, neg_pos_ub, rng_state, plant=None):
    """random_sampler.py:32-82 / base_sampler.py:79-99 for the images of a batch in order on ONE stream - a private
    torch.Generator set to ``rng_state``: positives first, ``candidates[torch.randperm(n)[:k]]`` only when there are more
    candidates than wanted, ``.unique()`` (sorted).  ([(pos_inds, neg_inds, info)], the generator state afterwards);
    info = candidates and wanted counts of the two draws."""
    g = torch.Generator()
    g.set_state(rng_state.clone())
    out = []

    def choose(cand, k):
        if cand.size <= k:
            return cand
        perm = torch.randperm(int(cand.size), generator=g)[:k].numpy()
        return cand[perm] if plant == 'unsorted' else np.unique(cand[perm])
    for gi in gt_inds_list:
        gi = _np(gi, np.int64)
        num_pos = int(num * pos_fraction)
        cp, cn = np.nonzero(gi > 0)[0], np.nonzero(gi == 0)[0]
        if plant == 'negatives first':
            kp = min(cp.size, num_pos)
            num_neg = num - kp
            if neg_pos_ub >= 0:
                num_neg = min(num_neg, int(neg_pos_ub * max(1, kp)))
            neg = choose(cn, num_neg)
            pos = choose(cp, num_pos)
        else:
            pos = choose(cp, num_pos)
            num_neg = num - pos.size
            if neg_pos_ub >= 0:
                num_neg = min(num_neg, int(neg_pos_ub * max(1, pos.size)))          # a Python (double) product
            neg = choose(cn, num_neg)
        out.append((pos.astype(np.int64), neg.astype(np.int64),
                    dict(n_pos=int(cp.size), want_pos=num_pos, n_neg=int(cn.size), want_neg=int(num_neg))))
    if plant == 'one draw too many':
        torch.randperm(2, generator=g)
    return out, g.get_state()


def sample_matches(got, got_state, exp, exp_state):
    """the checker: [(pos_inds, neg_inds)] per image and the generator state afterwards"""
    return len(got) == len(exp) and all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(got, exp)) and \
        same(got_state, exp_state)


# --------------------------------------------------------------------------------------------------------------- targets
def delta_expect(proposals, gts, means, stds, rule='positional', plant=None):
    """float64 (deltas, S, one-sided rows) of delta_xywh_bbox_coder.py:119-180 with the fork's zero-size guard (:152-160).
    ``rule`` 'positional': the reference's ``gy[nan_x] = py[nan_y]`` - the k-th zero-width row receives py of the k-th
    zero-height row; the reference RAISES when the two counts differ, and so does this.  'rowwise': what encode_delta
    of csrc/targets.hip does (gy = py only where both sides are zero) - KNOWN_DEVIATION_ENCODE_DELTA.  The two agree
    unless a row has exactly one zero side (their count is returned)."""
    p = _np(proposals, np.float32).astype(np.float64).reshape(-1, 4)
    g = _np(gts, np.float32).astype(np.float64).reshape(-1, 4)
    px, py = (p[:, 0] + p[:, 2]) * 0.5, (p[:, 1] + p[:, 3]) * 0.5
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    gx, gy = (g[:, 0] + g[:, 2]) * 0.5, (g[:, 1] + g[:, 3]) * 0.5
    gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    nx, ny = pw == 0, ph == 0
    tiny = float(np.float32(1e-6))
    pw, gw = np.where(nx, tiny, pw), np.where(nx, tiny, gw)
    ph, gh = np.where(ny, tiny, ph), np.where(ny, tiny, gh)
    gx = np.where(nx, px, gx)
    if rule == 'positional':
        if int(nx.sum()) != int(ny.sum()):
            raise ValueError('gy[nan_x] = py[nan_y] with %d zero-width and %d zero-height rows: the reference raises'
                             % (nx.sum(), ny.sum()))
        gy = gy.copy()
        gy[nx] = py[ny]
    else:
        assert rule == 'rowwise'
        gy = np.where(nx & ny, py, gy)
    m, s = np.asarray(means, np.float64), np.asarray(stds, np.float64)
    if plant == 'dw statistics on dx':
        m, s = m[[2, 1, 0, 3]], s[[2, 1, 0, 3]]
    with np.errstate(divide='ignore', invalid='ignore'):
        lw, lh = np.log(gw / pw), np.log(gh / ph)
        d = np.stack([(gx - px) / pw, (gy - py) / ph, lw, lh], 1)
        S = np.stack([(np.abs(gx) + np.abs(px)) / pw, (np.abs(gy) + np.abs(py)) / ph, np.abs(lw) + 1, np.abs(lh) + 1], 1)
    return (d - m) / s, S / np.abs(s) + np.abs(m / s), int((nx ^ ny).sum())


def delta_ratio(o, r, S, gamma=None):
    """worst |o - r| / (gamma S + ALPHA); a non-finite reference value (log of a non-positive width) must be met exactly"""
    o, r, S = _np(o).astype(np.float64).reshape(-1), np.asarray(r).reshape(-1), np.asarray(S).reshape(-1)
    if o.size == 0:
        return 0.0
    fin = np.isfinite(r) & np.isfinite(S)
    with np.errstate(invalid='ignore'):
        e = np.where(fin, np.abs(o - r) / ((GAMMA_T if gamma is None else gamma) * np.where(fin, S, 0.0) + ALPHA), 0.0)
        bad = ~fin & ~((o == r) | (np.isnan(o) & np.isnan(r)))
    e = np.where(np.isnan(e) | bad, np.inf, e)
    return float(e.max())


def _deltas_of(p, g, means, stds, plant=None):
    """positional where the reference is defined, else row-wise; the one-sided rows are counted either way"""
    pw, ph = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
    rule = 'positional' if int((pw == 0).sum()) == int((ph == 0).sum()) else 'rowwise'
    return delta_expect(p, g, means, stds, rule, plant)


def anchor_targets_expect(anchors, images, num_classes, pos_weight, means, stds, plant=None):
    """anchor_head.py:201-297 per image on shared anchors.  ``images``: dicts of gts [G, 4], gt_inds [A], pos_inds,
    neg_inds, gt_labels (None: RPN, foreground is class 0).  Exact: labels, label_weights, bbox_weights [B, A(, 4)];
    float64 deltas / S of the positive rows per image (every other row of bbox_targets is exactly 0)."""
    an = _np(anchors, np.float32)[:, :4]
    A, B = an.shape[0], len(images)
    labels = np.full((B, A), 0 if plant == 'label fill 0' else num_classes, np.int64)
    lw = np.zeros((B, A), np.float32)
    bw = np.zeros((B, A, 4), np.float32)
    deltas, one_sided = [], 0
    for b, im in enumerate(images):
        pos, neg = _np(im['pos_inds'], np.int64), _np(im['neg_inds'], np.int64)
        gi = _np(im['gt_inds'], np.int64)
        g = _np(im['gts'], np.float32).reshape(-1, 4)
        d, S, n1 = _deltas_of(an[pos], g[gi[pos] - 1], means, stds, plant)
        one_sided += n1
        deltas.append((pos, d, S))
        bw[b, pos] = 1.0
        gl = im.get('gt_labels')
        labels[b, pos] = 0 if gl is None else _np(gl, np.int64)[gi[pos] - 1]
        lw[b, pos] = 1.0 if pos_weight <= 0 or plant == 'pos_weight ignored' else pos_weight
        lw[b, neg] = 1.0
    return dict(labels=labels, label_weights=lw, bbox_weights=bw, deltas=deltas, one_sided=one_sided)


def roi_targets_expect(entries, num_classes, pos_weight, means, stds, extra=(), plant=None):
    """bbox_head.py:190-257 + transforms.py:75-94 (bbox2roi) + the fork's ``absolute`` output, entry by entry: the sampled
    positives, then the negatives; ``extra`` box lists (the random proposals) appended as rois with their own list
    position as batch index.  ``entries``: dicts of bboxes [n, >= 4], gts [G, 4], gt_inds [n], labels [n], pos_inds,
    neg_inds and optionally cap (a fixed row capacity: rows past the sampled ones are padding, ``live`` False).  Exact:
    rois, labels, label_weights, bbox_weights, absolute; float64 deltas / S [K, 4]."""
    rois, labels, lw, bw, ab, d_all, S_all, live = [], [], [], [], [], [], [], []
    one_sided, n_pos = 0, []
    for i, e in enumerate(entries):
        bx = _np(e['bboxes'], np.float32)[:, :4]
        g = _np(e['gts'], np.float32).reshape(-1, 4)
        gi, lab = _np(e['gt_inds'], np.int64), _np(e['labels'], np.int64)
        pos, neg = _np(e['pos_inds'], np.int64), _np(e['neg_inds'], np.int64)
        kp, kn = pos.size, neg.size
        rows = int(e['cap']) if e.get('cap') is not None else kp + kn
        pad = rows - kp - kn
        assert pad >= 0
        pb, pg = bx[pos], g[gi[pos] - 1]
        r = np.zeros((rows, 5), np.float32)
        r[:, 0] = i
        r[:kp, 1:], r[kp:kp + kn, 1:] = pb, bx[neg]
        rois.append(r)
        l = np.full(rows, 0 if plant == 'label fill 0' else num_classes, np.int64)
        l[:kp] = lab[pos]
        labels.append(l)
        w = np.ones(rows, np.float32)
        if kp:
            w[:kp] = 1.0 if pos_weight <= 0 or plant == 'pos_weight ignored' else pos_weight
        lw.append(w)
        b4 = np.zeros((rows, 4), np.float32)
        b4[:kp] = 1.0
        bw.append(b4)
        a4 = np.zeros((rows, 4), np.float32)
        a4[:kp] = pb if plant == 'absolute from the proposal' else pg
        ab.append(a4)
        d, S, n1 = _deltas_of(pb, pg, means, stds, plant)
        one_sided += n1
        n_pos.append(kp)
        d_all.append(np.concatenate([d, np.zeros((rows - kp, 4))]))
        S_all.append(np.concatenate([S, np.zeros((rows - kp, 4))]))
        live.append(np.arange(rows) < kp + kn)
    K = sum(x.shape[0] for x in labels)
    base = len(entries) if plant == 'extra rois continue the batch index' else 0
    for j, b in enumerate(extra):
        b = _np(b, np.float32)[:, :4]
        rois.append(np.concatenate([np.full((b.shape[0], 1), base + j, np.float32), b], 1))
    cat = np.concatenate
    live = cat(live) if live else np.zeros(0, bool)
    n_all = sum(x.shape[0] for x in rois)
    return dict(rois=cat(rois), K=K, labels=cat(labels), label_weights=cat(lw), bbox_weights=cat(bw), absolute=cat(ab),
                deltas=cat(d_all), S=cat(S_all), live=live, live_all=cat([live, np.ones(n_all - K, bool)]),
                one_sided=one_sided, n_pos=n_pos)


def roi_targets_match(got, exp, gamma=None):
    """the checker: ({field: ok} of the exact fields over the live rows, worst err / bound of the deltas).  ``got``:
    rois, K, labels, label_weights, bbox_targets, bbox_weights, absolute"""
    lv, la = exp['live'], exp['live_all']
    ok = {'K': int(got['K']) == exp['K'], 'rois': _np(got['rois']).shape == exp['rois'].shape and
          same(_np(got['rois'])[la], exp['rois'][la])}
    for k in ('labels', 'label_weights', 'bbox_weights', 'absolute'):
        ok[k] = _np(got[k]).shape == exp[k].shape and same(_np(got[k])[lv], exp[k][lv])
    bt = _np(got['bbox_targets'])
    if bt.shape != exp['deltas'].shape:
        return ok, float('inf')
    return ok, delta_ratio(bt[lv], exp['deltas'][lv], exp['S'][lv], gamma)


def anchor_targets_match(got, exp, gamma=None):
    """the checker of the anchor targets: ``got`` = labels, label_weights, bbox_targets, bbox_weights [B, A(, 4)]"""
    ok = {k: same(got[k], exp[k]) for k in ('labels', 'label_weights', 'bbox_weights')}
    bt = _np(got['bbox_targets'])
    worst, rest = 0.0, np.ones(bt.shape[:2], bool)
    for b, (pos, d, S) in enumerate(exp['deltas']):
        worst = max(worst, delta_ratio(bt[b, pos], d, S, gamma))
        rest[b, pos] = False
    ok['bbox_targets of unsampled rows are 0'] = not bool(np.any(bt[rest] != 0))
    return ok, worst


# ------------------------------------------------------------------------------------------------------ random proposals
def random_bboxes_expect(np_state, img_size, num_bboxes, bboxes_xy=None, **kw):
    """the trial loop of two_stage.py:389-419 (oadg_amd.detectors' Python form, which tests/test_core_reference.py ties to
    the golden's rand_boxes* / rand_rng*) drawing from ``np_state``: (boxes, numpy's global state afterwards).  The
    caller's global numpy state is left as it was."""
    from oadg_amd import detectors
    keep = np.random.get_state()
    native = detectors.NATIVE_RANDOM_BBOXES
    try:
        detectors.NATIVE_RANDOM_BBOXES = False
        np.random.set_state(np_state)
        fn = getattr(detectors.generate_random_bboxes_xy, '_audit_orig', detectors.generate_random_bboxes_xy)
        out = fn(img_size, num_bboxes, bboxes_xy=bboxes_xy, **kw)
        return out, np.random.get_state()
    finally:
        detectors.NATIVE_RANDOM_BBOXES = native
        np.random.set_state(keep)


def np_state_same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


# --------------------------------------------------------------------------------------------------------------- auditor
class Auditor(IA.ProposalAudit, HA.Auditor):
    """rows / failures / kernels / wrappers as tests/head_audit.py's Auditor; ``labels`` = the ``what`` of every C-ABI call
    that reported through a ``check`` while installed, ``checked`` = those a wrapper verified"""

    def __init__(self):
        super().__init__()
        self.quiet = 0
        self.labels = []
        self.checked = set()
        self.draws = []              # per sampled image: branch, candidate / wanted counts, k_pos, k_neg
        self.n_pos = {'rpn': [], 'roi': []}
        self.one_sided = 0           # sampled positives with exactly one zero side (KNOWN_DEVIATION_ENCODE_DELTA)
        self.worst_delta = 0.0
        self.end_state = None        # the CPU generator state the device sampler's draws must leave (after sync_host)
        self.declined = []

    def print_table(self, title):
        super().print_table(title)
        print('n_pos per image:', self.n_pos)
        print('draws:', self.draws)
        print('worst err / bound of the deltas (GAMMA_T = 2^%d): %.4f' % (int(np.log2(GAMMA_T)), self.worst_delta))
        print('sampled positives with exactly one zero side:', self.one_sided)
        print('declined (tensor path):', self.declined)
        print('labels checked:', sorted(self.checked))

    def _claim(self, ran, mine):
        self.checked.update(set(ran) & set(mine))

    def check_end_state(self):
        """after the step's sync_host: torch's CPU generator holds what the replayed draws leave"""
        if self.end_state is not None:
            self.exact('roi_sample_kernel', (0,), same(torch.get_rng_state(), self.end_state),
                       check='CPU generator state after sync_host')
        return self.end_state is not None

    def install(self, mp, det=None):
        from oadg_amd import _lib, dense_heads, detectors, device_rng, hip_conv, hip_ops, roi_heads
        from oadg_amd.core import bbox as BB
        A = self
        sync = torch.cuda.synchronize
        self.install_proposals(mp)                      # RPNHead.get_bboxes, hip_ops.nms_sorted_batched, _lib.check
        labels = self.labels
        for mod in (_lib, hip_ops, hip_conv):           # (hip_ops / hip_conv bound ``check`` by name at import)
            def check(rc, what, _c=mod.check):
                labels.append(what)
                return _c(rc, what)
            mp.setattr(mod, 'check', check)

        def ran_since(n0):
            return labels[n0:]

        # the RPN's assignment (and the RoI head's, when roi_assign_sample_begin declines)
        am = BB.MaxIoUAssigner.assign_many

        def assign_many(asg, boxes, valids, gt_bboxes_list, gt_labels_list=None):
            A.hit('MaxIoUAssigner.assign_many')
            n0 = len(labels)
            out = am(asg, boxes, valids, gt_bboxes_list, gt_labels_list)
            sync()
            if out is None:
                A.declined.append('assign_many')
                return out
            A._claim(ran_since(n0), ['oadg_max_iou_assign'])
            with torch.no_grad():
                A._check_assign(asg, boxes, valids, gt_bboxes_list, gt_labels_list, out)
            return out
        mp.setattr(BB.MaxIoUAssigner, 'assign_many', assign_many)

        # the RoI head's assignment with the gts added as proposals
        rb = BB.roi_assign_sample_begin

        def roi_assign_sample_begin(assigner, sampler, proposals, gt_bboxes_list, gt_labels_list):
            A.hit('roi_assign_sample_begin')
            n0 = len(labels)
            pend = rb(assigner, sampler, proposals, gt_bboxes_list, gt_labels_list)
            sync()
            if pend is None:
                A.declined.append('roi_assign_sample_begin')
                return pend
            A._claim(ran_since(n0), ['oadg_roi_assign_add_gt'])
            with torch.no_grad():
                A._check_roi_assign(assigner, proposals, gt_bboxes_list, gt_labels_list, pend)
            return pend
        mp.setattr(BB, 'roi_assign_sample_begin', roi_assign_sample_begin)
        mp.setattr(roi_heads, 'roi_assign_sample_begin', roi_assign_sample_begin)

        # the draws: host branch (oadg_host_randperm_prefix + oadg_sample_select) and device branch
        rp = BB.randperm_prefix

        def randperm_prefix(n, k):
            if n >= 4096:
                A.hit('randperm_prefix (oadg_host_randperm_prefix)')
                A.checked.add('oadg_host_randperm_prefix')      # judged by the indices and the end state of finish()
            return rp(n, k)
        mp.setattr(BB, 'randperm_prefix', randperm_prefix)
        fin = BB.PendingSampling.finish

        def finish(p):
            if p.results is not None or not p.prepared:
                return fin(p)
            A.hit('PendingSampling.finish')
            dev = p.prepared[0][1].device
            if BB._SPEC is not None and dev.type == 'cuda':
                gen = device_rng.generator(dev)                 # what _finish_device does before it uploads the state
                if gen.pending():
                    gen.sync_host()
            state0 = torch.get_rng_state()
            n0 = len(labels)
            res = fin(p)
            sync()
            A._claim(ran_since(n0), ['oadg_sample_select', 'oadg_roi_sample_device'])
            with torch.no_grad():
                A._check_sampling(p, res, state0, ran_since(n0))
            return res
        mp.setattr(BB.PendingSampling, 'finish', finish)

        # anchor targets
        ft = dense_heads.AnchorHead._fused_targets

        def _fused_targets(head, pend, srs, num_level_anchors, gt_labels_list, unmap_outputs):
            A.hit('AnchorHead._fused_targets')
            n0 = len(labels)
            out = ft(head, pend, srs, num_level_anchors, gt_labels_list, unmap_outputs)
            sync()
            # the kernel's domain: every anchor inside the padded image and no border filter (allowed_border < 0)
            in_domain = bool(head._all_anchors_valid and head.train_cfg.allowed_border < 0)
            A.exact('targets_scatter_kernel', (len(srs),), (out is not None) == in_domain,
                    check='fused path taken where the config is in its domain')
            A.info['anchor_targets'] = 'fused' if out is not None else 'tensor path'
            if out is not None:
                A._claim(ran_since(n0), ['oadg_anchor_targets'])
                with torch.no_grad():
                    A._check_anchor_targets(head, pend, srs, num_level_anchors, out, head._whole_targets)
            else:
                stash[:] = [(pend, srs, num_level_anchors)]
            return out
        mp.setattr(dense_heads.AnchorHead, '_fused_targets', _fused_targets)
        gt_ = dense_heads.AnchorHead.get_targets
        stash = []

        def get_targets(head, *a, **k):
            del stash[:]
            out = gt_(head, *a, **k)
            if stash and out is not None:                       # the tensor path ran on the batch assignment: same check
                sync()
                pend, srs, nla = stash.pop()
                if getattr(pend.prepared[0][0], 'batch', None) is not None and pend.prepared[0][0].batch['boxes'] is not None:
                    with torch.no_grad():
                        A._check_anchor_targets(head, pend, srs, nla, out, [torch.cat(list(lvl), 1) for lvl in out[:4]],
                                                name='anchor targets (tensor path)')
            return out
        mp.setattr(dense_heads.AnchorHead, 'get_targets', get_targets)

        # rois + RoI targets
        rt = roi_heads.BBoxHead.rois_and_targets

        def rois_and_targets(head, sampling_results, rcnn_train_cfg, extra=()):
            A.hit('BBoxHead.rois_and_targets')
            n0 = len(labels)
            out = rt(head, sampling_results, rcnn_train_cfg, extra)
            sync()
            A.exact('roi_targets_kernel', (len(sampling_results), len(extra)), out is not None, check='fused path taken')
            if out is not None:
                A._claim(ran_since(n0), ['oadg_roi_targets', 'oadg_roi_targets_dev'])
                with torch.no_grad():
                    A._check_roi_targets(head, sampling_results, rcnn_train_cfg, extra, out, ran_since(n0))
            return out
        mp.setattr(roi_heads.BBoxHead, 'rois_and_targets', rois_and_targets)

        # OA-Loss random proposals (numpy's global stream)
        gen_boxes = detectors.generate_random_bboxes_xy
        nat = detectors._random_bboxes_native
        native_calls = []

        def _random_bboxes_native(*a, **k):
            out = nat(*a, **k)
            native_calls.append(out is not None)
            return out
        mp.setattr(detectors, '_random_bboxes_native', _random_bboxes_native)

        def generate_random_bboxes_xy(img_size, num_bboxes, bboxes_xy=None, **kw):
            A.hit('generate_random_bboxes_xy')
            state0 = np.random.get_state()
            del native_calls[:]
            out = gen_boxes(img_size, num_bboxes, bboxes_xy=bboxes_xy, **kw)
            state1 = np.random.get_state()
            ref, ref_state = random_bboxes_expect(state0, img_size, num_bboxes, bboxes_xy, **kw)
            native = native_calls == [True]
            A.exact('oadg_np_random_bboxes (host)', (len(out),), native, check='native path taken', launched=False)
            if native:
                A.checked.add('oadg_np_random_bboxes')
            A.exact('oadg_np_random_bboxes (host)', (len(out),), same(out, ref) and np.asarray(out).dtype == ref.dtype,
                    check='boxes', launched=False)
            A.exact('oadg_np_random_bboxes (host)', (len(out),), np_state_same(state1, ref_state) and
                    np_state_same(np.random.get_state(), state1), check="numpy's global state afterwards", launched=False)
            return out
        generate_random_bboxes_xy._audit_orig = gen_boxes
        mp.setattr(detectors, 'generate_random_bboxes_xy', generate_random_bboxes_xy)
        return self

    # -- per-call checks
    def after_proposals(self, head, cfg, padded, out, nms_counts):
        self._claim(self.labels, IA.CLAIMS)             # (verified by the two shared wrappers)
        if not padded:
            return
        cnt = nms_counts.cpu().tolist() if nms_counts is not None else [None] * len(out)
        for i, d in enumerate(out):
            d = _np(d)
            live = d[:, 4] >= 0
            k = int(live.sum())
            ok = d.shape == (int(cfg.max_per_img), 5) and bool(live[:k].all()) and \
                same(d[k:], np.tile(np.array([0, 0, 0, 0, -1], np.float32), (d.shape[0] - k, 1))) and \
                (cnt[i] is None or k == min(int(cnt[i]), d.shape[0]))
            self.exact('rpn_gather_kernel', d.shape, ok, check='padded to max_per_img with (0, 0, 0, 0, -1) rows')
            self.info.setdefault('proposals_kept', []).append(k)

    def _check_assign(self, asg, boxes, valids, gts_list, labels_list, out):
        res, counts = out
        cnt = counts.cpu().tolist()
        lo, hi = (0.0, asg.neg_iou_thr) if isinstance(asg.neg_iou_thr, float) else asg.neg_iou_thr
        shared = isinstance(boxes, torch.Tensor)
        bx_shared = _np(boxes) if shared else None
        self.kernels.update({'assign_gtmax_kernel', 'assign_kernel'})
        for i, ar in enumerate(res):
            bx = bx_shared if shared else _np(boxes[i])
            v = None if valids is None or valids[i] is None else _np(valids[i]).astype(bool)
            gl = None if labels_list is None or labels_list[i] is None else labels_list[i]
            gi, mo, lab, (n_pos, n_neg) = assign_expect(bx, v, gts_list[i], gl, asg.pos_iou_thr, lo, hi, asg.min_pos_iou,
                                                        asg.match_low_quality)
            ok = np.ones(bx.shape[0], bool) if v is None else v
            shape = (len(res), bx.shape[0], int(_np(gts_list[i]).reshape(-1, 4).shape[0]))
            self.exact('assign_kernel', shape, same(ar.gt_inds, gi), check='gt_inds')
            self.exact('assign_kernel', shape, same(_np(ar.max_overlaps)[ok], mo[ok]), check='max_overlaps')
            self.exact('assign_kernel', shape, tuple(cnt[i]) == (n_pos, n_neg), check='counts')
            if lab is not None:
                self.exact('assign_kernel', shape, ar.labels is not None and same(ar.labels, lab), check='labels')
            if shared:
                self.n_pos['rpn'].append(n_pos)

    def _check_roi_assign(self, asg, proposals, gts_list, labels_list, pend):
        lo, hi = (0.0, asg.neg_iou_thr) if isinstance(asg.neg_iou_thr, float) else asg.neg_iou_thr
        self.event_wait(pend)
        cnt = pend.counts.tolist()
        self.kernels.update({'roi_assign_prep_kernel', 'assign_gtmax_kernel', 'assign_kernel'})
        for i, (ar, boxes, G, _, _) in enumerate(pend.prepared):
            p = _np(proposals[i])
            v = p[:, 4] >= 0 if p.shape[1] == 5 else np.ones(p.shape[0], bool)
            gi, mo, lab, (n_pos, n_neg) = assign_expect(p, v, gts_list[i], labels_list[i], asg.pos_iou_thr, lo, hi,
                                                        asg.min_pos_iou, asg.match_low_quality)
            eb, egi, elab, emo, _ = add_gt_expect(p, gts_list[i], labels_list[i], gi, mo, lab)
            ok = np.concatenate([np.ones(G, bool), v])
            shape = (len(pend.prepared), p.shape[0], G)
            self.exact('roi_assign_prep_kernel', shape, G == _np(gts_list[i]).reshape(-1, 4).shape[0] and same(boxes, eb),
                       check='boxes, gts in front')
            self.exact('assign_kernel', shape, same(ar.gt_inds, egi), check='gt_inds (RoI form, padding rows -1)')
            self.exact('assign_kernel', shape, same(ar.labels, elab), check='labels (RoI form)')
            self.exact('assign_kernel', shape, _np(ar.max_overlaps).shape == emo.shape and
                       same(_np(ar.max_overlaps)[ok], emo[ok]), check='max_overlaps (RoI form)')
            self.exact('assign_kernel', shape, tuple(cnt[i]) == (n_pos, n_neg), check='counts (RoI form)')
            self.n_pos['roi'].append(n_pos + G)
            self.info.setdefault('roi_padding_rows', []).append(int((~v).sum()))

    @staticmethod
    def event_wait(pend):
        if pend.event is not None:
            pend.event.synchronize()

    def _check_sampling(self, p, res, state0, ran):
        from oadg_amd.core import bbox as BB
        s = p.sampler
        gis = [prep[0].gt_inds for prep in p.prepared]
        exp, exp_state = sample_expect(gis, s.num, s.pos_fraction, s.neg_pos_ub, state0)
        B = len(res)
        device = isinstance(res[0], BB.DeviceSamplingResult)
        branch = 'device' if device else 'host'
        kind = 'roi' if getattr(s, 'add_gt_as_proposals', True) else 'rpn'      # (the RPN's sampler adds no gts)
        if device:
            self.kernels.add('roi_sample_kernel')
            name = 'roi_sample_kernel'
            meta = BB._SPEC[-1]['meta'].numpy().copy()           # counts [B][2] | flags [B] (the copy has landed: sync)
            got = []
            for i, r in enumerate(res):
                kp, kn = (int(v) for v in r.cnt.cpu().tolist())
                sel = _np(r.sel)
                got.append((sel[:kp], sel[kp:kp + kn]))
                e = exp[i]
                self.exact(name, (B, gis[i].numel()), (kp, kn) == (e[0].size, e[1].size) and
                           tuple(meta[2 * i:2 * i + 2]) == (kp, kn), check='counts')
                self.exact(name, (B, gis[i].numel()), int(meta[2 * B + i]) == int(e[0].size + e[1].size != s.num),
                           check='flags')
            self.exact(name, (B,), all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(got, exp)),
                       check='sel (positives, then negatives, sorted)')
            self.end_state = exp_state                           # compared after the step's sync_host
            self.exact(name, (B,), same(torch.get_rng_state(), state0), check='host generator untouched until sync_host')
            self.info.setdefault('flags', []).append(meta[2 * B:].tolist())
        else:
            self.kernels.update({'sel_count_kernel', 'sel_locate_kernel'} if 'oadg_sample_select' in ran else set())
            name = 'sel_locate_kernel'
            got = [(r.pos_inds, r.neg_inds) for r in res]
            self.exact(name, (B, kind), all(same(a[0], b[0]) and same(a[1], b[1]) for a, b in zip(got, exp)),
                       check='pos_inds / neg_inds (%s)' % kind)
            self.exact(name, (B, kind), same(torch.get_rng_state(), exp_state), check='CPU generator state (%s)' % kind)
        for i, e in enumerate(exp):
            self.draws.append(dict(kind=kind, branch=branch, image=i, k_pos=int(e[0].size), k_neg=int(e[1].size), **e[2]))

    def _check_anchor_targets(self, head, pend, srs, num_level_anchors, out, whole, name='targets_scatter_kernel'):
        batch = pend.prepared[0][0].batch
        B = len(srs)
        counts = [int(prep[0].num_gts) for prep in pend.prepared]
        images = [dict(gts=batch['gts'][i][:counts[i]] if counts[i] else np.zeros((0, 4), np.float32),
                       gt_inds=batch['gt_inds'][i], pos_inds=srs[i].pos_inds, neg_inds=srs[i].neg_inds) for i in range(B)]
        coder = head.bbox_coder
        exp = anchor_targets_expect(batch['boxes'], images, head.num_classes, head.train_cfg.pos_weight, coder.means,
                                    coder.stds)
        lab, lw, bt, bw = whole
        fused = name == 'targets_scatter_kernel'
        ok, worst = anchor_targets_match(dict(labels=lab, label_weights=lw, bbox_targets=bt, bbox_weights=bw), exp)
        shape = tuple(lab.shape)
        if fused:
            self.kernels.update({'targets_fill_kernel', 'targets_scatter_kernel'})
        for k, v in ok.items():
            self.exact(name, shape, v, check=k, launched=fused)
        self._delta_row(name, shape, worst, launched=fused)
        self.one_sided += exp['one_sided']
        # images_to_levels: the per-level views and the two totals
        cat = [torch.cat([t for t in lvl], 1) for lvl in out[:4]]
        self.exact(name, shape, all(torch.equal(a, b) for a, b in zip(cat, (lab, lw, bt, bw))) and
                   [t.shape[1] for t in out[0]] == list(num_level_anchors), check='per-level views', launched=False)
        tot = (sum(max(_np(r.pos_inds).size, 1) for r in srs), sum(max(_np(r.neg_inds).size, 1) for r in srs))
        self.exact(name, shape, tuple(out[4:6]) == tot, check='num_total_pos / neg', launched=False)

    def _delta_row(self, kernel, shape, worst, launched=True):
        self.worst_delta = max(self.worst_delta, worst)
        z = torch.zeros(1, dtype=torch.float64)
        self.record(kernel, shape, z + worst, z, z + 1.0, check='deltas (err / bound, GAMMA_T)', launched=launched)

    def _check_roi_targets(self, head, sampling_results, cfg, extra, out, ran):
        from oadg_amd.core import bbox as BB
        entries = []
        for r in sampling_results:
            bboxes, gtb, ar, _ = r._src
            e = dict(bboxes=bboxes, gts=gtb, gt_inds=ar.gt_inds, labels=ar.labels)
            if isinstance(r, BB.DeviceSamplingResult):
                kp, kn = (int(v) for v in r.cnt.cpu().tolist())
                sel = _np(r.sel)
                e.update(pos_inds=sel[:kp], neg_inds=sel[kp:kp + kn], cap=r.cap)
            else:
                e.update(pos_inds=r.pos_inds, neg_inds=r.neg_inds)
            entries.append(e)
        coder = head.bbox_coder
        exp = roi_targets_expect(entries, head.num_classes, cfg.pos_weight, coder.means, coder.stds, extra)
        rois, K, (lab, lw, bt, bw, ab) = out
        ok, worst = roi_targets_match(dict(rois=rois, K=K, labels=lab, label_weights=lw, bbox_targets=bt, bbox_weights=bw,
                                           absolute=ab), exp)
        shape = (len(sampling_results), len(extra), int(rois.shape[0]))
        self.kernels.add('roi_targets_kernel')
        entry = 'oadg_roi_targets_dev' if 'oadg_roi_targets_dev' in ran else 'oadg_roi_targets'
        for k, v in ok.items():
            self.exact('roi_targets_kernel', shape, v, check='%s (%s)' % (k, entry))
        self._delta_row('roi_targets_kernel', shape, worst)
        self.one_sided += exp['one_sided']
        self.info.setdefault('roi_targets_entry', []).append(entry)
        self.info.setdefault('roi_sampled_pos', []).append(exp['n_pos'])
