"""Launch auditor of the parts of bf16 test-time inference that no training audit checks: the fused RPN proposals and every
NMS launch (a training step makes its RoI proposals on the same kernels: tests/target_audit.py runs the same two wrappers
there, at nms_pre = 2000 with padded lists), the forward outputs of the RoI head's linears on autocast's casts, any
convolution that reaches the library's F.conv2d (a row per layer shape - none is expected) and the detector's
post-processing.  The MFMA convolutions, the weight preparation and RoIAlign of the same forward pass
are audited by tests/conv_audit.py and tests/head_audit.py, installed beside this one.

Bounds in the form of tests/conv_audit.py (``|o - r| <= RHO |r| + GAMMA S + ALPHA``); exact operations are compared bit
for bit: the fused proposals against RPNHead.get_bboxes' tensor path on the same head outputs, every NMS keep list and
count against oracle/nms.py on the sorted, class-offset boxes the launch received, fc_weight_permute (tests/head_audit.py).

The post-processing (softmax, delta2bbox clamped to img_shape, rescale, score threshold, greedy NMS, max_per_img,
bbox2result) is recomputed on the host in float64 from the fp32 rois / cls_score / bbox_pred the head produced.  Every
returned detection must be a candidate of ITS class within fp32 rounding of the fp64 box and score.  The kept set may
differ from the fp64 one only where a score or an IoU lies within fp32 rounding of its threshold (and through what such a
difference suppresses or pushes past max_per_img): those detections are counted in ``Auditor.borderline`` and the GPU
tests cap the count; any other difference is a failure.
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_audit as CA
import head_audit as HA

RHO, ALPHA, GAMMA_GEMM, PROB_ERR = HA.RHO, HA.ALPHA, HA.GAMMA_GEMM, HA.PROB_ERR
# relative fp32 error of a decoded, clamped and rescaled box coordinate: delta * std + mean, the centre and size products,
# expf, the half-size sum / difference and the division by the scale factor - under ten roundings of quantities no larger
# than |centre| + |size| of the box
BOX_ERR = 2.0 ** -20
# absolute fp32 error of an IoU beyond what the coordinates' errors explain (the division and the area products)
IOU_ERR = 2.0 ** -20
# detections of the post-processing that differ from the fp64 selection through a decision within fp32 rounding, per
# candidate above the score threshold: the RoIAlign carve-out cap of tests/test_head_audit.py (measured: 0 on every workload
# of tests/test_inference_audit.py)
BORDERLINE_CAP = 1e-4


# ------------------------------------------------------------------------------------------------------- fp64 references
def linear_expect(x, w, b, low):
    """(r, bound) of F.linear(x, w, b) whose operands autocast rounds to ``low`` (None: fp32 operands, fp32 output)"""
    c = (lambda t: t.detach().to(low).to(torch.float64)) if low is not None else (lambda t: t.detach().to(torch.float64))
    x64, w64 = c(x).reshape(-1, x.shape[-1]), c(w)
    r = x64 @ w64.t()
    S = x64.abs() @ w64.abs().t()
    if b is not None:
        b64 = c(b)
        r, S = r + b64, S + b64.abs()
    return r, (RHO if low is not None else 0.0) * r.abs() + GAMMA_GEMM * S + ALPHA


def nms_expect(boxes, count, iou_thr, max_keep):
    """oracle/nms.py on the first ``count`` rows of one image's sorted, class-offset boxes: the kept rows, ascending"""
    from oracle import nms as ONMS
    return ONMS.nms_sorted(boxes[:count].detach().cpu().numpy(), iou_thr, max_keep=max_keep)


def decode_expect(rois, cls_score, bbox_pred, img_shape, scale_factor, means, stds, flip=False,
                  wh_ratio_clip=16 / 1000):
    """fp64 (boxes [n, C, 4], their tolerance, scores [n, C + 1], their tolerance) of ConvFCBBoxHead.get_bboxes before
    the NMS: softmax, delta2bbox against rois[:, 1:] clamped to img_shape, then (aug_test's merge) the horizontal flip back
    and the division by the scale factor"""
    r = torch.as_tensor(rois).detach().cpu().to(torch.float64)[:, 1:5]
    x = torch.as_tensor(cls_score).detach().cpu().to(torch.float64)
    n = x.shape[0]
    p = torch.softmax(x, 1)
    # expf(x - max) / sum in fp32: relative error ~ ulp (1 + |x - max|) (tests/head_audit.py ce_jsd_expect)
    stol = PROB_ERR * (1.0 + (x - x.max(1, keepdim=True)[0]).abs()) * p + ALPHA
    d = torch.as_tensor(bbox_pred).detach().cpu().to(torch.float64).view(n, -1, 4)
    d = d * torch.tensor(stds, dtype=torch.float64) + torch.tensor(means, dtype=torch.float64)
    pxy = ((r[:, :2] + r[:, 2:]) * 0.5).view(n, 1, 2)
    pwh = (r[:, 2:] - r[:, :2]).view(n, 1, 2)
    mr = float(np.abs(np.log(wh_ratio_clip)))
    gxy = pxy + pwh * d[..., :2]
    gwh = pwh * d[..., 2:].clamp(-mr, mr).exp()
    b = torch.cat([gxy - gwh * 0.5, gxy + gwh * 0.5], -1)
    mag = (gxy.abs() + gwh.abs()).repeat(1, 1, 2)
    H, W = float(img_shape[0]), float(img_shape[1])
    b[..., 0::2] = b[..., 0::2].clamp(0, W)
    b[..., 1::2] = b[..., 1::2].clamp(0, H)
    if flip:
        b = torch.stack([W - b[..., 2], b[..., 1], W - b[..., 0], b[..., 3]], -1)
        mag = mag + W
    sf = torch.as_tensor(np.asarray(scale_factor, dtype=np.float32)).to(torch.float64)
    b = b / sf
    btol = BOX_ERR * (mag / sf + b.abs()) + ALPHA
    return b, btol, p, stol


def merge_expect(parts):
    """aug_test's merge (core merge_aug_bboxes) of per-augmentation decode_expect results: boxes and scores averaged"""
    k = len(parts)
    b = sum(q[0] for q in parts) / k
    bt = sum(q[1] for q in parts) / k + BOX_ERR * b.abs()
    s = sum(q[2] for q in parts) / k
    st = sum(q[3] for q in parts) / k + PROB_ERR * s
    return b, bt, s, st


def multiclass_expect(boxes, scores, score_thr, iou_thr, max_num):
    """the fp64 selection of multiclass_nms: kept candidates (flat index i * C + c) in output order - score > score_thr,
    stable descending sort, greedy NMS per class (oracle/nms.py), the first max_num"""
    from oracle import nms as ONMS
    n, C = boxes.shape[:2]
    s = scores[:, :C].reshape(-1)
    b = boxes.reshape(-1, 4)
    idx = torch.nonzero(s > score_thr).view(-1)
    order = idx[torch.sort(s[idx], descending=True, stable=True)[1]]
    rank = torch.full((n * C,), -1, dtype=torch.long)
    rank[order] = torch.arange(order.numel())
    kept = []
    for c in range(C):
        sub = order[order % C == c]
        if sub.numel():
            kept.append(sub[torch.as_tensor(ONMS.nms_sorted(b[sub].numpy(), iou_thr), dtype=torch.long)])
    if not kept:
        return torch.zeros(0, dtype=torch.long)
    kept = torch.cat(kept)
    kept = kept[torch.argsort(rank[kept])]
    return kept[:max_num] if max_num > 0 else kept


def _iou(a, b):
    lt = torch.maximum(a[:2], b[:2])
    rb = torch.minimum(a[2:], b[2:])
    inter = (rb - lt).clamp_min(0).prod()
    union = (a[2:] - a[:2]).prod() + (b[2:] - b[:2]).prod() - inter
    return float(inter / union) if union > 0 else 0.0, float(union)


def compare_detections(result, boxes, btol, scores, stol, score_thr, iou_thr, max_num):
    """(failures, borderline detections, candidates above the threshold) of the detector's per-class arrays ``result``
    against the fp64 candidates"""
    n, C = boxes.shape[:2]
    fb, ft = boxes.reshape(-1, 4), btol.reshape(-1, 4)
    fs, fst = scores[:, :C].reshape(-1), stol[:, :C].reshape(-1)
    fails = []
    got = []
    if len(result) != C:
        return [('classes', len(result), C)], 0, 0
    for c in range(C):
        a = np.asarray(result[c])
        if a.size == 0:
            continue
        if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 5:
            fails.append(('result array', c, a.dtype, a.shape))
            continue
        g = torch.from_numpy(a).to(torch.float64)
        cand = torch.arange(c, n * C, C)
        ok = ((g[:, None, :4] - fb[cand][None]).abs() <= ft[cand][None]).all(-1) & \
            ((g[:, None, 4] - fs[cand][None]).abs() <= fst[cand][None])
        used = set()
        for j in range(g.shape[0]):
            hits = [int(cand[h]) for h in torch.nonzero(ok[j]).view(-1).tolist() if int(cand[h]) not in used]
            if not hits:
                fails.append(('detection matches no candidate of its class', c, j, a[j].tolist()))
                continue
            used.add(hits[0])
            got.append(hits[0])
    ref = multiclass_expect(boxes, scores, score_thr, iou_thr, max_num).tolist()
    total = int((fs > score_thr).sum())
    G, R = set(got), set(ref)
    D = sorted(G ^ R)
    if not D:
        return fails, 0, total
    mx = float(fb.abs().max()) if fb.numel() else 0.0
    shift = 2.0 ** -23 * C * (mx + 1)          # batched NMS: every class offset by (max coordinate + 1), rounded to fp32

    def near_iou(d, e):
        v, u = _iou(fb[d], fb[e])
        eps = float(ft[d].max() + ft[e].max()) + shift
        side = float((fb[d, 2:] - fb[d, :2]).sum() + (fb[e, 2:] - fb[e, :2]).sum())
        return v, 4 * eps * side / max(u, 1e-30) + IOU_ERR

    roots = set()
    for d in D:
        if abs(float(fs[d]) - score_thr) <= float(fst[d]):
            roots.add(d)                                       # score threshold
            continue
        for e in G | R:
            if e == d or e % C != d % C:
                continue
            v, tol = near_iou(d, e)
            if abs(v - iou_thr) <= tol or (v > iou_thr - tol and abs(float(fs[d] - fs[e])) <= float(fst[d] + fst[e])):
                roots.add(d)                                   # an IoU at the threshold, or two overlapping equal scores
                break
    ok = set(roots)
    grew = True
    while grew:                                                # what a borderline difference suppresses in turn
        grew = False
        for d in D:
            if d in ok:
                continue
            for e in ok:
                if e % C == d % C and e != d:
                    v, tol = near_iou(d, e)
                    if v > iou_thr - tol:
                        ok.add(d)
                        grew = True
                        break
    if ok and max_num > 0:                                     # ... or pushes past max_per_img
        # each explained difference moves the cut by at most one place: only the last len(ok) places of either list
        tail = max_num - len(ok)
        # (``got`` is collected class by class: the detector's output order is descending score, stable in candidate order)
        by_score = sorted(got, key=lambda d: (-float(fs[d]), d))
        for lst in (by_score, ref):
            if len(lst) == max_num:
                for k, d in enumerate(lst):
                    if k >= tail and d in D:
                        ok.add(d)
    for d in D:
        if d not in ok:
            fails.append(('kept set differs from the fp64 selection', 'kept' if d in G else 'dropped', d // C, d % C,
                          float(fs[d]), fb[d].tolist()))
    return fails, len(D), total


# ----------------------------------------------------------------------------------------------------------- auditor
# the C-ABI calls this auditor answers for (tests/test_target_audit.py's closure over the call sites): the proposal and NMS
# launches, at test-time settings here and at training settings through tests/target_audit.py
CLAIMS = {'oadg_rpn_topk', 'oadg_rpn_decode', 'oadg_rpn_order', 'oadg_rpn_gather', 'oadg_nms_batched'}


class ProposalAudit:
    """the two wrappers of the RoI proposals, shared with tests/target_audit.py (the training step makes its proposals on
    the same kernels): every NMS launch against oracle/nms.py, RPNHead.get_bboxes' fused path against its tensor path.
    Needs ``self.quiet`` (> 0 while a reference path runs) beside tests/head_audit.py's Auditor."""

    def after_proposals(self, head, cfg, padded, out, nms_counts):
        """hook: the proposal lists ``out`` of one get_bboxes call and the kept counts of its NMS launch"""

    def install_proposals(self, mp):
        from oadg_amd import _lib, dense_heads, hip_ops
        A = self
        sync = torch.cuda.synchronize
        launches = []
        chk = _lib.check
        last_nms = []

        def check(rc, what):
            launches.append(what)
            return chk(rc, what)
        mp.setattr(_lib, 'check', check)

        # every NMS launch: keep list and count against the oracle on the exact boxes
        nms = hip_ops.nms_sorted_batched

        def nms_sorted_batched(boxes, counts, iou_thr, max_keep=-1):
            keep, cnt = nms(boxes, counts, iou_thr, max_keep)
            if A.quiet:
                return keep, cnt
            A.hit('nms_sorted_batched')
            sync()
            with torch.no_grad():
                A._check_nms(boxes, counts, iou_thr, max_keep, keep, cnt)
            last_nms[:] = [cnt]
            return keep, cnt
        mp.setattr(hip_ops, 'nms_sorted_batched', nms_sorted_batched)

        # the fused proposals against the tensor path on the same head outputs
        gb = dense_heads.RPNHead.get_bboxes

        def get_bboxes(head, cls_scores, bbox_preds, img_metas=None, cfg=None, num_imgs=None, padded=False, **kw):
            A.hit('RPNHead.get_bboxes')
            del launches[:]
            out = gb(head, cls_scores, bbox_preds, img_metas=img_metas, cfg=cfg, num_imgs=num_imgs, padded=padded, **kw)
            sync()
            ran = list(launches)
            A.quiet += 1
            saved = (head.FUSED_PROPOSALS, head.FUSED_TOPK)
            try:
                head.FUSED_PROPOSALS = head.FUSED_TOPK = False
                ref = gb(head, cls_scores, bbox_preds, img_metas=img_metas, cfg=cfg, num_imgs=num_imgs, padded=padded, **kw)
            finally:
                del head.FUSED_PROPOSALS, head.FUSED_TOPK
                A.quiet -= 1
            assert (head.FUSED_PROPOSALS, head.FUSED_TOPK) == saved
            A._check_proposals(ran, out, ref)
            A.after_proposals(head, head.test_cfg if cfg is None else cfg, padded, out, last_nms[0] if last_nms else None)
            return out
        mp.setattr(dense_heads.RPNHead, 'get_bboxes', get_bboxes)
        return self

    def _check_nms(self, boxes, counts, iou_thr, max_keep, keep, cnt):
        n_img, M = boxes.shape[:2]
        mk = max_keep if 0 < max_keep <= M else M
        words = (M + 63) // 64
        self.kernels.add('nms_mask_kernel')
        name = 'nms_scan_kernel<3, 2>' if words <= 64 * 3 else 'nms_scan_kernel<MAX_WORDS_PER_LANE, 1>'
        c = counts.cpu().tolist()
        k = cnt.cpu().tolist()
        for i in range(n_img):
            ref = nms_expect(boxes[i].float(), int(c[i]), float(iou_thr), mk)
            got = keep[i, :int(k[i])].cpu().numpy().astype(np.int64)
            self.exact(name, (n_img, M, int(c[i])), int(k[i]) == len(ref) and np.array_equal(got, ref), check='keep list')

    def _check_proposals(self, ran, out, ref):
        fused = 'oadg_rpn_gather' in ran
        if fused:
            self.kernels.update({'rpn_decode_kernel', 'rpn_order_kernel', 'rpn_gather_kernel'})
            if 'oadg_rpn_topk' in ran:
                self.kernels.update({'sel_score_kernel', 'sel_refine_kernel<1>', 'sel_refine_kernel<2>', 'sel_count_kernel2',
                                     'sel_scatter_kernel', 'sel_sort_kernel'})
        self.info['proposals'] = 'fused' if fused else 'tensor path'
        ok = len(out) == len(ref) and all(a.shape == b.shape and torch.equal(a, b) for a, b in zip(out, ref))
        self.exact('rpn proposals (fused vs tensor path)', (len(out),) + tuple(out[0].shape), ok, launched=False)
        self.info['proposals_per_img'] = [int(a.shape[0]) for a in out]


class Auditor(ProposalAudit, HA.Auditor):
    """rows / failures / kernels / borderline as tests/head_audit.py's Auditor"""

    def __init__(self):
        super().__init__()
        self.quiet = 0               # >0 while a reference path runs (its NMS launches are not the product's)
        self.post = []               # per forward: the captured (rois, cls_score, bbox_pred, metas) of the RoI head
        self.results = []            # per forward: what the detector returned

    def install(self, mp, det):
        self.install_proposals(mp)
        A = self
        sync = torch.cuda.synchronize

        # the RoI head's linears (autocast's casts, the library GEMM) and the RPN's library convolutions
        lin = F.linear

        def linear(x, w, b=None):
            y = lin(x, w, b)
            if not A.quiet and y.is_cuda:
                sync()
                with torch.no_grad(), torch.autocast('cuda', enabled=False):
                    low = y.dtype if y.dtype != torch.float32 else None
                    A.hit('F.linear')
                    r, bd = linear_expect(x, w, b, low)
                    A.record('F.linear (library GEMM)', (x.shape[0], w.shape[1], w.shape[0]),
                             y.detach().reshape(-1, y.shape[-1]).to(torch.float64), r, bd)
            return y
        mp.setattr(F, 'linear', linear)
        cv = F.conv2d

        def conv2d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
            y = cv(x, w, b, stride, padding, dilation, groups)
            if not A.quiet and y.is_cuda and groups == 1:
                sync()
                with torch.no_grad(), torch.autocast('cuda', enabled=False):
                    A.hit('F.conv2d')
                    t = (lambda v: v.to(y.dtype)) if y.dtype != torch.float32 else (lambda v: v)   # noqa: E731
                    st, pd, dl = (v[0] if isinstance(v, (tuple, list)) else v for v in (stride, padding, dilation))
                    r, bd = CA.forward_expect(t(x), t(w), t(b) if b is not None else None, None, st, pd, dl, False)
                    if y.dtype == torch.float32:
                        bd = bd - RHO * r.abs()
                    # (keyed by layer: any test-time convolution that reaches the library adds a row to the kernel set)
                    A.record('F.conv2d (library) %d->%d %dx%d' % (w.shape[1], w.shape[0], w.shape[2], w.shape[3]),
                             tuple(x.shape) + tuple(w.shape), CA._nhwc64(y), r, bd)
            return y
        mp.setattr(F, 'conv2d', conv2d)

        # the RoI head's outputs and the detector's per-class arrays
        rh = det.roi_head
        st_ = type(rh).simple_test_bboxes
        at_ = type(rh).aug_test_bboxes
        bh = type(rh.bbox_head).get_bboxes

        def simple_test_bboxes(head, x, img_metas, proposals, rcnn_test_cfg, rescale=False):
            out = st_(head, x, img_metas, proposals, rcnn_test_cfg, rescale=rescale)
            res = head.bbox_results
            A.post.append(('simple', [p.detach().float().clone() for p in proposals], res['cls_score'].detach().float(),
                           res['bbox_pred'].detach().float(), img_metas, rescale, rcnn_test_cfg))
            return out
        mp.setattr(type(rh), 'simple_test_bboxes', simple_test_bboxes)
        augs = []

        def bbox_get_bboxes(head, rois, cls_score, bbox_pred, img_shape, scale_factor, rescale=False, cfg=None):
            if cfg is None:
                augs.append((rois.detach().float().clone(), cls_score.detach().float(), bbox_pred.detach().float()))
            return bh(head, rois, cls_score, bbox_pred, img_shape, scale_factor, rescale=rescale, cfg=cfg)
        mp.setattr(type(rh.bbox_head), 'get_bboxes', bbox_get_bboxes)

        def aug_test_bboxes(head, feats, img_metas, proposal_list, rcnn_test_cfg):
            del augs[:]
            out = at_(head, feats, img_metas, proposal_list, rcnn_test_cfg)
            A.post.append(('aug', list(augs), None, None, img_metas, True, rcnn_test_cfg))
            return out
        mp.setattr(type(rh), 'aug_test_bboxes', aug_test_bboxes)
        return self

    # -- per-forward check
    def check_results(self, det, fwd, results):
        """the post-processing of forward ``fwd`` (its entry of ``self.post``) against the detector's ``results``"""
        kind, props, cls_score, bbox_pred, metas, rescale, cfg = self.post[fwd]
        coder = det.roi_head.bbox_head.bbox_coder
        means, stds = coder.means, coder.stds
        nms_thr = cfg.nms.get('iou_threshold', cfg.nms.get('iou_thr'))
        if kind == 'simple':
            cuts = np.cumsum([0] + [len(p) for p in props])
            per_img = []
            for i, p in enumerate(props):
                rois = torch.cat([torch.full((len(p), 1), float(i)), p[:, :4].cpu()], 1)
                sl = slice(int(cuts[i]), int(cuts[i + 1]))
                m = metas[i]
                per_img.append(decode_expect(rois, cls_score[sl], bbox_pred[sl], m['img_shape'],
                                             m['scale_factor'] if rescale else np.ones(4, np.float32), means, stds))
        else:
            parts = []
            for (rois, cs, bp), meta in zip(props, metas):
                m = meta[0]
                parts.append(decode_expect(rois, cs, bp, m['img_shape'], m['scale_factor'], means, stds,
                                           flip=bool(m['flip'])))
            per_img = [merge_expect(parts)]
        assert len(per_img) == len(results)
        for i, (b, bt, s, st) in enumerate(per_img):
            fails, border, total = compare_detections(results[i], b, bt, s, st, cfg.score_thr, nms_thr, cfg.max_per_img)
            self.count('post-processing', border, total)
            self.exact('post-processing (fp64 host reference)', (i, total), not fails, launched=False)
            self.failures.extend(fails[:10])
            self.info.setdefault('detections', []).append(int(sum(len(r) for r in results[i])))


def within_cap(carved, total):
    return carved <= BORDERLINE_CAP * max(total, 1)
