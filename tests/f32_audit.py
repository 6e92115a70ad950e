"""Launch auditor of the fp32 parity path's convolutions (csrc/conv_f32.hip through oadg_amd/hip_conv_f32.py): every launch
of an fp32 training step - forward, transposed-gather data gradient, weight gradient + split reduce - checked elementwise
against a float64 recomputation from the exact operands it received (teacher forcing), in the form of tests/conv_audit.py::

    |o - r| <= GAMMA_F32 * S + ALPHA                (outputs are fp32: no RHO term)

``S`` is the same computation over absolute values (plus |bias|).  Where ``S`` is zero - a border pixel no tap reaches, a
zero-padded channel, a parity class of a strided data gradient that receives nothing - the bound is ALPHA: the output must
be zero.

``Auditor.install(monkeypatch, det)`` wraps hip_conv_f32's ``_conv`` / ``_wgrad`` (the level at which the kernels' real
operands are visible: padded NHWC tensors, [K][R][S][C4] weights), ``_Conv2dF32.forward`` / ``backward`` (channel slicing,
the bias gradient, ``needs_input_grad``) and ``conv2d_f32`` (which parameter a call belongs to).  ``check_params`` compares
every trainable convolution parameter's ``.grad`` with the fp64 BN-fold chain rule applied to the fp64 weight / bias
gradients of the operands each launch received.  The pure functions are what tests/test_f32_audit.py's CPU half exercises.
"""
import numpy as np
import torch

import conv_audit as CA
from conv_audit import conv_ref, ratio, wgrad_ref  # noqa: F401

U = 2.0 ** -24           # unit roundoff of fp32 (round to nearest)
ALPHA = 1e-30
# The two constants are set from measurement on the MI355X over the three audited steps and every stress launch of
# tests/test_f32_audit.py: the smallest power of two that is at least twice the worst err / S (the kernels are deterministic -
# fixed split order, no atomics -, so the margin covers other inputs only).  MEASURED: worst err / (2^-24 S) per family and
# the launch it occurred in.
MEASURED = {
    'conv': (34.072, 'stress, same-signed operands: conv_f32_kernel transposed 3x3 s1 d2, dy [2, 2048, 48, 96] x W [2048][3][3]'
                     '[2048] - 18432 non-negative products per element'),
    'wgrad': (39.762, 'r50_fpn_f32 step: conv_wgrad_f32_kernel + reduce 3x3 s1 d1, x [8, 256, 256, 512], K 256 - 8 splits of '
                      '131072 pixels, 2048 chains of 64 per split'),
}
# conv_f32_kernel, forward and transposed gather: 32 products chained per stage, one add per stage into the running sum.
# Worst 34.07 x 2^-24 = 2^-18.91 S (the same-signed stress launch above; the three audited steps, whose weights are signed,
# reach 6.9 / 6.8 / 9.1, the other stress launches 4.4): a margin of 3.76x.  A-priori bound of the tree at the longest audited
# reduction (18432 products): 610 x 2^-24.  The numpy emulation of the two orders on 18432 same-signed products puts the
# blocked sums at 23 units and one long chain at 163: this constant separates them (tests/test_f32_audit.py).  On SIGNED
# products it cannot: there the emulation gives 0.8 (blocked) against 3 - 4 (one chain), both far below a constant that has
# to admit the same-signed launch.  Measured once on the kernel itself, rebuilt with one running accumulator instead of the
# blocked sums: the same-signed stress launch 207 units (rejected, 1.6x the bound); the audited R101-DC5 step 9.1 -> 26.6
# units (a factor 2.9, accepted).
GAMMA_F32_CONV = 2.0 ** -17
# conv_wgrad_f32_kernel + wgrad_f32_reduce_kernel: 64 pixels chained per block, blocks chained per split, splits chained.
# Worst 39.76 x 2^-24 = 2^-18.69 S (the bench step's 3x3 layer at 256 x 512 above: post-ReLU activations against signed
# gradients, 2048 block sums chained per split; the other steps reach 37.1 - 512 splits with empty trailing ones - and 26.0,
# the same-signed one-split stress launch 16.5): a margin of 3.22x.  A-priori bound at that launch: (64 + 2048 + 8 + 2) x
# 2^-24; at the 512 splits of 2048 pixels of the head gradients: 610 x 2^-24.  Same remark on signed operands as above.
GAMMA_F32_WGRAD = 2.0 ** -17
# torch's own fp32 arithmetic around the kernels - ``gy.sum((0, 2, 3))``, the BN fold's tensor expressions and their
# autograd (layers.conv_bn: products with gamma * rsqrt(var + eps), sums over C R S), the sum of a shared parameter's
# per-level gradients: not this project's kernels, bounded a priori.  A torch reduction chains a few elements per thread
# and sums the threads' partials in a tree: under 64 roundings for every reduction of these steps (2^22 pixels:
# 4 x 4 unrolled chains of <= 16 + a tree of depth <= 22), the elementwise part of the fold is 5 roundings.
TORCH_F32 = 64 * U
# the C-ABI calls this auditor answers for (tests/test_target_audit.py's closure over the call sites of oa-dg_amd/)
CLAIMS = {'oadg_conv2d_f32', 'oadg_conv2d_wgrad_f32'}


# ---------------------------------------------------------------------------------------------------- fp64 references
def _nhwc64(t):
    return t.detach().permute(0, 2, 3, 1).to(torch.float64)


def out_size(H, R, stride, pad, dil):
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1


def dgrad_ref(gy, w, H, W, stride, pad, dil):
    """(dx, S) [N,H,W,C] fp64 of the data gradient of y = conv(x, w) for the output gradient gy [N,K,Ho,Wo], w [K,C,R,S] -
    the adjoint of the forward gather, from the definition
    dx[n, oh stride - pad + r dil, ow stride - pad + s dil, c] += gy[n, oh, ow, k] w[k, c, r, s]  (any stride / dil / pad;
    ``(H, W)`` may exceed what the forward reads: rows the forward never read get nothing)"""
    N, K, Ho, Wo = gy.shape
    _, C, R, S_ = w.shape
    w64 = w.detach().to(torch.float64)
    Hp = max(H + 2 * pad, (R - 1) * dil + stride * (Ho - 1) + 1)
    Wp = max(W + 2 * pad, (S_ - 1) * dil + stride * (Wo - 1) + 1)
    dx = torch.zeros((N, Hp, Wp, C), dtype=torch.float64, device=gy.device)
    a = torch.zeros_like(dx)
    for n in range(N):
        g = _nhwc64(gy[n:n + 1]).reshape(-1, K)
        ga = g.abs()
        for i in range(R):
            for j in range(S_):
                wk = w64[:, :, i, j]
                h0, w0 = i * dil, j * dil
                dx[n, h0:h0 + stride * (Ho - 1) + 1:stride, w0:w0 + stride * (Wo - 1) + 1:stride].add_(
                    (g @ wk).view(Ho, Wo, C))
                a[n, h0:h0 + stride * (Ho - 1) + 1:stride, w0:w0 + stride * (Wo - 1) + 1:stride].add_(
                    (ga @ wk.abs()).view(Ho, Wo, C))
    return dx[:, pad:pad + H, pad:pad + W].contiguous(), a[:, pad:pad + H, pad:pad + W].contiguous()


def sample(x, hi, wi, okh=None, okw=None):
    """x [N,H,W,C] -> [N, len(hi), len(wi), C]: x[:, hi, wi] with zeros where an index is out of range (or not ok)"""
    H, W = x.shape[1], x.shape[2]
    mh = (hi >= 0) & (hi < H) if okh is None else okh & (hi >= 0) & (hi < H)
    mw = (wi >= 0) & (wi < W) if okw is None else okw & (wi >= 0) & (wi < W)
    v = x[:, hi.clamp(0, H - 1)][:, :, wi.clamp(0, W - 1)]
    return v * (mh.view(-1, 1) & mw.view(1, -1)).view(1, len(hi), len(wi), 1).to(x.dtype)


def gather_conv(x, w, stride, pad, dil, Ho, Wo, plant=None):
    """the forward in the kernel's gather form, [N,Ho,Wo,K] fp64: y[oh, ow] = sum_rs x[oh stride - pad + r dil, ...] w[r, s].
    ``plant``: 'dil and stride swapped'"""
    x64, w64 = _nhwc64(x), w.detach().to(torch.float64)
    K, C, R, S_ = w.shape
    a, b = (dil, stride) if plant == 'dil and stride swapped' else (stride, dil)
    oh, ow = torch.arange(Ho), torch.arange(Wo)
    y = torch.zeros((x.shape[0], Ho, Wo, K), dtype=torch.float64)
    for r in range(R):
        for s in range(S_):
            y += sample(x64, oh * a - pad + r * b, ow * a - pad + s * b) @ w64[:, :, r, s].t()
    return y


def gather_dgrad(gy, w, H, W, stride, pad, dil, plant=None):
    """the data gradient in the kernel's transposed gather form, [N,H,W,C] fp64: pixel (oh, ow) of dx takes, for every tap,
    source pixel ((oh + pad - r dil) / stride, (ow + pad - s dil) / stride) when both divisions are exact and in range.
    ``plant``: 'no divisibility test' (every source pixel floored)"""
    g64, w64 = _nhwc64(gy), w.detach().to(torch.float64)
    K, C, R, S_ = w.shape
    oh, ow = torch.arange(H), torch.arange(W)
    dx = torch.zeros((gy.shape[0], H, W, C), dtype=torch.float64)
    for r in range(R):
        for s in range(S_):
            nh, nw = oh + pad - r * dil, ow + pad - s * dil
            hi, wi = torch.div(nh, stride, rounding_mode='floor'), torch.div(nw, stride, rounding_mode='floor')
            okh, okw = nh >= 0, nw >= 0
            if plant != 'no divisibility test':
                okh, okw = okh & (hi * stride == nh), okw & (wi * stride == nw)
            dx += sample(g64, hi, wi, okh, okw) @ w64[:, :, r, s]
    return dx


def wgrad_plan(N, Ho, Wo, C, K, R, S_):
    """(splits, per_split) of csrc oadg_conv2d_wgrad_f32_splits / oadg_conv2d_wgrad_f32, restated"""
    P = N * Ho * Wo
    tiles = ((K + 31) // 32) * ((C + 31) // 32) * R * S_
    s = (4096 + tiles - 1) // tiles
    s = max(1, min(s, (P + 511) // 512, 1024))
    return s, ((P + s - 1) // s + 7) // 8 * 8


def empty_trailing_splits(P, splits, per_split):
    """splits whose pixel range starts at or behind P (per_split is rounded up to a multiple of 8)"""
    return sum(1 for k in range(splits) if k * per_split >= P)


def conv_tree_bound(R, S_, C):
    """a-priori rounding bound (in S) of conv_f32_kernel's documented summation tree: a chain of 32 products, one add per
    stage into the running sum, bias add, the product roundings"""
    return (32 + -(-R * S_ * C // 32) + 2) * U


def wgrad_tree_bound(per_split, splits):
    return (64 + -(-per_split // 64) + splits + 2) * U


# ------------------------------------------------------------------------------------ numpy emulation of the sum orders
def blocked_sum_f32(prod, block):
    """rows of products [n, L] (L a multiple of ``block``) summed in float32 as the kernels do: a sequential chain inside a
    block from zero, then one add of the block's sum to the running sum"""
    p = np.asarray(prod, np.float32)
    n, L = p.shape
    parts = np.add.accumulate(p.reshape(n, L // block, block), axis=2, dtype=np.float32)[:, :, -1]
    return np.add.accumulate(parts, axis=1, dtype=np.float32)[:, -1]


def chain_sum_f32(prod):
    """the same rows as ONE sequential float32 chain"""
    return np.add.accumulate(np.asarray(prod, np.float32), axis=1, dtype=np.float32)[:, -1]


def sum_units(got, prod):
    """error of float32 row sums against the float64 sum, in units of 2^-24 S"""
    p = np.asarray(prod, np.float64)
    return np.abs(got.astype(np.float64) - p.sum(1)) / (np.abs(p).sum(1) * U)


def bound(S, gamma, *extra):
    b = gamma * S + ALPHA
    for e in extra:
        b = b + e
    return b


# ----------------------------------------------------------------------------------------------------------- auditor
class Row:
    __slots__ = ('calls', 'shapes', 'worst', 'where')

    def __init__(self):
        self.calls, self.shapes, self.worst, self.where = 0, set(), 0.0, None


def _tags(C, K):
    return (' C%d' % C if C % 32 else '') + (' K%d' % K if K % 32 else '')


def conv_label(transposed, R, S_, stride, dil, C, K):
    """what distinguishes launches of conv_f32_kernel: mode, filter, stride, dilation, ragged channel counts (C: the
    reduction's channels, a last 32-chunk with dead 16-byte pieces; K: output channels, a partly live 64-channel tile)"""
    return 'conv_f32_kernel %s %dx%d s%d d%d%s' % ('transposed' if transposed else 'forward', R, S_, stride, dil,
                                                 (' C%d' % C if C % 32 else '') + (' K%d' % K if K % 64 else ''))


def wgrad_label(R, S_, stride, dil, C, K, P, splits, per_split):
    how = '1 split' if splits == 1 else ('%d splits' % splits if splits >= 512 else 'splits')
    if empty_trailing_splits(P, splits, per_split):
        how += ' (empty trailing)'
    return 'conv_wgrad_f32_kernel + reduce %dx%d s%d d%d%s, %s' % (R, S_, stride, dil, _tags(C, K), how)


class Auditor:
    def __init__(self):
        self.table = {}
        self.wrappers = {}
        self.kernels = set()         # the launch labels audited
        self.failures = []
        self.labels = []             # the ``what`` of every check() of hip_conv_f32 while installed
        self.checked = set()         # those a wrapper verified
        self.params = {}             # id(weight parameter) -> [weight, bias, bn, dWf, S, db, S_db, calls]
        self.declined = 0
        self.units = {'conv': [0.0, None], 'wgrad': [0.0, None]}     # worst err / (2^-24 S) per family and its launch
        self.longest = {'conv': 0, 'wgrad': (0, 0)}                  # longest audited reduction (R S C; per_split, splits)

    # -- bookkeeping
    def hit(self, wrapper):
        self.wrappers[wrapper] = self.wrappers.get(wrapper, 0) + 1

    def record(self, kernel, shape, o, ref, b, check=None, launched=True, S=None, family=None):
        rt, i = ratio(o, ref, b)
        if launched:
            self.kernels.add(kernel)
        name = kernel if check is None else '%s %s' % (kernel, check)
        row = self.table.setdefault(name, Row())
        row.calls += 1
        row.shapes.add(tuple(shape))
        if rt > row.worst or row.where is None:
            row.worst = max(rt, row.worst)
            row.where = (tuple(shape), i, float(o.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(b.reshape(-1)[i]))
        if not rt <= 1.0:
            self.failures.append((name, tuple(shape), rt, row.where))
        if family is not None and S is not None:
            live = S > 0
            if bool(live.any()):
                u = ((o.to(torch.float64) - ref).abs()[live] / (S[live] * U)).max().item()
                if u > self.units[family][0]:
                    self.units[family] = [u, (name, tuple(shape))]
        return rt

    def exact(self, kernel, shape, ok, check=None, launched=True):
        z = torch.zeros(1, dtype=torch.float64)
        return self.record(kernel, shape, z, z + (0.0 if ok else 1.0), torch.full((1,), ALPHA, dtype=torch.float64),
                           check=check, launched=launched)

    def worst(self):
        return max((r.worst for r in self.table.values()), default=0.0)

    def print_table(self, title):
        print('\n== f32 audit: %s ==' % title)
        print('%-78s %6s %10s  %s' % ('launch', 'calls', 'err/bound', 'worst element (shape, index, out, ref, bound)'))
        for k in sorted(self.table):
            r = self.table[k]
            print('%-78s %6d %10.4f  %s' % (k, r.calls, r.worst, r.where))
        print('wrappers:', dict(sorted(self.wrappers.items())))
        for fam, g in (('conv', GAMMA_F32_CONV), ('wgrad', GAMMA_F32_WGRAD)):
            u, where = self.units[fam]
            print('worst err / S, %s: %.3f x 2^-24 = 2^%.2f (constant 2^%d: margin %.2fx) in %s; longest reduction %s' % (
                fam, u, np.log2(max(u, 1e-9) * U), int(np.log2(g)), g / max(u * U, 1e-300), where, self.longest[fam]))
        print('labels checked:', sorted(self.checked), 'declined calls:', self.declined)

    # -- installation
    def install(self, mp, det=None):
        from oadg_amd import backbones, hip_conv_f32 as HF, layers
        A = self
        sync = torch.cuda.synchronize
        L = HF._lib.lib()
        labels = self.labels

        def check(rc, what, _c=HF.check):
            labels.append(what)
            return _c(rc, what)
        mp.setattr(HF, 'check', check)

        def nograd(fn):
            def g(*a, **k):
                with torch.no_grad(), torch.autocast('cuda', enabled=False):
                    return fn(*a, **k)
            return g

        by_ptr = {}
        bn_of = {}
        if det is not None:
            for n, p in det.named_parameters():
                by_ptr[p.data_ptr()] = p
        context = []                 # (conv, bn) of the layers.conv_bn call in progress
        pending = []                 # source of the conv2d_f32 call in progress: (weight parameter, bias parameter, bn)
        last = {}                    # what the launches of the _Conv2dF32.backward in progress produced

        cbn = layers.conv_bn

        def conv_bn(x, conv, bn, *a, **k):
            context.append((conv, bn))
            try:
                return cbn(x, conv, bn, *a, **k)
            finally:
                context.pop()
        mp.setattr(layers, 'conv_bn', conv_bn)
        mp.setattr(backbones, 'conv_bn', conv_bn)

        c2d = HF.conv2d_f32

        def conv2d_f32(x, weight, bias, stride, padding, dilation):
            A.hit('conv2d_f32')
            src = None
            p = by_ptr.get(weight.data_ptr())
            if p is not None and p.shape == weight.shape:
                src = (p, by_ptr.get(bias.data_ptr()) if bias is not None else None, None)
            elif context and tuple(weight.shape) == tuple(context[-1][0].weight.shape):
                src = (context[-1][0].weight, None, context[-1][1])      # the folded weight of this conv + BN pair
            pending[:] = [src]
            n0 = len(labels)
            y = c2d(x, weight, bias, stride, padding, dilation)
            if y is None:
                A.declined += 1
                A.exact('conv2d_f32 (dispatcher)', tuple(weight.shape), not labels[n0:], check='declined: nothing launched',
                        launched=False)
            return y
        mp.setattr(HF, 'conv2d_f32', conv2d_f32)

        conv, wgrad = HF._conv, HF._wgrad

        def _conv(x4, w_krsc, bias, stride, pad, dil, transposed=False, out_hw=(0, 0)):
            A.hit('_conv transposed' if transposed else '_conv')
            n0 = len(labels)
            y = conv(x4, w_krsc, bias, stride, pad, dil, transposed, out_hw)
            sync()
            if labels[n0:] == ['oadg_conv2d_f32']:
                A.checked.add('oadg_conv2d_f32')
            nograd(A._check_conv)(x4, w_krsc, bias, stride, pad, dil, transposed, out_hw, y)
            last['conv'] = y
            return y

        def _wgrad(x4, g4, R, S_, stride, pad, dil):
            A.hit('_wgrad')
            n0 = len(labels)
            dw = wgrad(x4, g4, R, S_, stride, pad, dil)
            sync()
            if labels[n0:] == ['oadg_conv2d_wgrad_f32']:
                A.checked.add('oadg_conv2d_wgrad_f32')
            last['wgrad'] = nograd(A._check_wgrad)(L, x4, g4, R, S_, stride, pad, dil, dw)
            return dw
        mp.setattr(HF, '_conv', _conv)
        mp.setattr(HF, '_wgrad', _wgrad)

        ff, fb = HF._Conv2dF32.forward, HF._Conv2dF32.backward

        def forward(ctx, x, w, bias, stride, pad, dil):
            A.hit('_Conv2dF32.forward')
            ctx._audit_src = pending[0] if pending else None
            del pending[:]
            return ff(ctx, x, w, bias, stride, pad, dil)

        def backward(ctx, gy):
            A.hit('_Conv2dF32.backward')
            last.clear()
            outs = fb(ctx, gy)
            sync()
            nograd(A._check_backward)(ctx, gy, outs, dict(last))
            last.clear()
            return outs
        mp.setattr(HF._Conv2dF32, 'forward', staticmethod(forward))
        mp.setattr(HF._Conv2dF32, 'backward', staticmethod(backward))
        return self

    # -- per-launch checks
    def _check_conv(self, x4, w_krsc, bias, stride, pad, dil, transposed, out_hw, y):
        N, C, H, W = x4.shape
        K, R, S_, _ = w_krsc.shape
        if transposed:
            r, S = dgrad_ref(x4, w_krsc.permute(3, 0, 1, 2), out_hw[0], out_hw[1], stride, pad, dil)
        else:
            r, S = conv_ref(x4, w_krsc.permute(0, 3, 1, 2), stride, pad, dil)
            if bias is not None:
                b64 = bias.detach().to(torch.float64)
                r += b64
                S += b64.abs()
        name = conv_label(transposed, R, S_, stride, dil, C, K)
        shape = tuple(x4.shape) + tuple(w_krsc.shape) + (stride, pad, dil)
        o = _nhwc64(y)
        self.exact(name, shape, tuple(o.shape) == tuple(r.shape) and y.dtype == torch.float32, check='shape / dtype')
        self.record(name, shape, o, r, bound(S, GAMMA_F32_CONV), S=S, family='conv')
        dead = S == 0
        self.exact(name, shape, bool((o[dead] == 0).all()), check='exactly zero where nothing is summed (%s)' % (
            'some' if bool(dead.any()) else 'none'))
        self.longest['conv'] = max(self.longest['conv'], R * S_ * C)

    def _check_wgrad(self, L, x4, g4, R, S_, stride, pad, dil, dw):
        N, C, H, W = x4.shape
        K, Ho, Wo = g4.shape[1], g4.shape[2], g4.shape[3]
        P = N * Ho * Wo
        splits, per_split = wgrad_plan(N, Ho, Wo, C, K, R, S_)
        name = wgrad_label(R, S_, stride, dil, C, K, P, splits, per_split)
        shape = tuple(x4.shape) + (K, R, S_, stride, pad, dil, splits)
        self.exact(name, shape, splits == int(L.oadg_conv2d_wgrad_f32_splits(N, Ho, Wo, C, K, R, S_)),
                   check='split plan as restated')
        r, S = wgrad_ref(x4, g4, R, S_, stride, pad, dil)                  # [K, C, R, S]
        o = dw.detach().permute(0, 3, 1, 2).to(torch.float64)
        self.record(name, shape, o, r, bound(S, GAMMA_F32_WGRAD), S=S, family='wgrad')
        dead = S == 0
        self.exact(name, shape, bool((o[dead] == 0).all()), check='exactly zero where nothing is summed (%s)' % (
            'some' if bool(dead.any()) else 'none'))
        if self.longest['wgrad'] == (0, 0) or wgrad_tree_bound(per_split, splits) > wgrad_tree_bound(*self.longest['wgrad']):
            self.longest['wgrad'] = (per_split, splits)
        return name, r, S

    def _check_backward(self, ctx, gy, outs, last):
        x4, w = ctx.saved_tensors
        stride, pad, dil, has_bias, C = ctx.cfg
        K, _, R, S_ = w.shape
        gx, gw, gb = outs[:3]
        need = ctx.needs_input_grad
        shape = tuple(x4.shape) + tuple(w.shape)
        self.exact('_Conv2dF32.backward', shape, (gx is not None) == bool(need[0]) and (gw is not None) == bool(need[1]) and
                   (gb is not None) == bool(has_bias and need[2]) and ('conv' in last) == bool(need[0]) and
                   ('wgrad' in last) == bool(need[1]) and all(o is None for o in outs[3:]),
                   check='launches and outputs follow needs_input_grad', launched=False)
        if gx is not None:
            y = last['conv']
            self.exact('_Conv2dF32.backward', shape, gx.shape[1] == C and tuple(gx.shape[2:]) == tuple(x4.shape[2:]) and
                       torch.equal(gx, y[:, :C]), check='dx = the launch\'s first C channels', launched=False)
        g64 = _nhwc64(gy).reshape(-1, K)
        db, Sdb = g64.sum(0), g64.abs().sum(0)
        if gb is not None:
            self.record('gy.sum((0, 2, 3)) (torch)', tuple(gy.shape), gb.double(), db, bound(Sdb, TORCH_F32), launched=False)
        if gw is not None:
            name, r, S = last['wgrad']
            r, S = r[:K, :C], S[:K, :C]
            self.record(name, shape, gw.double(), r, bound(S, GAMMA_F32_WGRAD), check='returned dW [:K, :C]')
            src = getattr(ctx, '_audit_src', None)
            if src is not None:
                acc = self.params.get(id(src[0]))
                if acc is None:
                    self.params[id(src[0])] = [src[0], src[1], src[2], r.clone(), S.clone(), db, Sdb, 1]
                else:
                    acc[3] += r
                    acc[4] += S
                    acc[5] = acc[5] + db
                    acc[6] = acc[6] + Sdb
                    acc[7] += 1

    # -- parameter level
    def check_params(self, named):
        """compare every audited parameter's .grad with its fp64 reference (summed over the step's calls of a shared
        convolution); returns the set of parameter names checked"""
        names = {id(p): n for n, p in named}
        seen = set()
        with torch.no_grad():
            for wp, bp, bn, dwf, S, db, Sdb, calls in self.params.values():
                # autograd adds a shared parameter's per-call gradients in fp32: one rounding of the partial sum per add
                acc = (calls - 1) * U
                if bn is None:
                    checks = [(wp, dwf, S, GAMMA_F32_WGRAD + acc, '(conv)')]
                    if bp is not None:
                        checks.append((bp, db, Sdb, TORCH_F32 + acc, '(bias)'))
                else:
                    dW, SdW, dg, Sdg = CA.bn_chain_expect(dwf, S, db, Sdb, wp, bn.weight, bn.running_mean, bn.running_var,
                                                          bn.eps)
                    g = GAMMA_F32_WGRAD + TORCH_F32 + acc
                    checks = [(wp, dW, SdW, g, '(conv, BN fold)'), (bn.weight, dg, Sdg, g, '(bn weight)'),
                              (bn.bias, db, Sdb, TORCH_F32 + acc, '(bn bias)')]
                for p, ref, Sref, gamma, what in checks:
                    if p is None or not p.requires_grad:
                        continue
                    n = names.get(id(p), '?')
                    seen.add(n)
                    if p.grad is None:
                        self.failures.append(('param .grad missing', n))
                        continue
                    self.record('param .grad', (calls,) + tuple(p.shape), p.grad.double(), ref, bound(Sref, gamma),
                                check=what, launched=False)
        return seen
