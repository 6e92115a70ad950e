"""Launch auditor of the convolution family: every launch of a real training step checked elementwise against a float64
recomputation from the exact operands it received ("teacher forcing": independent of the bf16 drift through the network
and of discrete decisions such as top-k, NMS and sampling).

Bound per element, with ``r`` the fp64 value (before ReLU), ``S`` the same computation over absolute values plus the
absolute epilogue terms, and ``o`` the kernel's output::

    |o - r| <= RHO * |r| + GAMMA * S + ALPHA          (RHO = 0 for fp32 outputs)

ReLU and the masks are 1-Lipschitz, so the bound carries through them.  Where the product deliberately rounds an
intermediate to bf16, one more RHO term of that intermediate is added and named at the place it is added.

``Auditor.install(monkeypatch)`` wraps the Python entry points of hip_conv / hip_ops; ``Auditor.check_params`` compares every
trainable parameter's gradient after ``hip_conv.end_backward()`` with the fp64 BN-fold chain rule applied to the fp64
weight / bias gradients of the operands each layer's backward received.  The pure reference functions below are also what
tests/test_conv_audit.py's CPU self-tests exercise.
"""
import torch
import torch.nn.functional as F

RHO = 2.0 ** -8          # one bf16 rounding (8 significant bits, round to nearest even)
# fp32 accumulation.  One constant for every launch, set from measurement: the worst err / bound over the fp32 outputs of the three
# audited GPU workloads of tests/test_conv_audit.py is 0.277 (configs[1]: a grouped weight-gradient element of a 1024 -> 256
# layer, 65536 same-signed bf16 products summed in fp32 - about sqrt(n) units of 2^-24), i.e. an error of 2^-15.85 S: a
# margin of 3.6x.  (2^-20 would reject correct fp32 sums: that element needs 2^-15.85.)
GAMMA = 2.0 ** -14
ALPHA = 1e-30            # absolute floor (values that flush to zero as fp32 / bf16 denormals)
# the C-ABI calls this auditor answers for (tests/test_target_audit.py's closure over the call sites of oa-dg_amd/): every
# launch of hip_conv.py, the stem, the fused max-pool and the FPN top-down pair
CLAIMS = {
    'oadg_conv2d_nhwc_bf16_ex', 'oadg_conv2d_nhwc_bf16_scatter', 'oadg_conv2d_dgrad_s2_nhwc_bf16', 'oadg_conv2d_wgrad_nhwc_bf16',
    'oadg_conv2d_wgrad_parts_nhwc_bf16', 'oadg_conv2d_wgrad_multi', 'oadg_colsum_reduce', 'oadg_colsum_reduce_multi',
    'oadg_relu_bias_bwd', 'oadg_prep_conv_weights', 'oadg_prep_conv_weights_multi', 'oadg_prep_conv_weights_bwd',
    'oadg_prep_conv_weights_bwd_parts', 'oadg_prep_conv_weights_bwd_parts_multi', 'oadg_bottleneck_frozen_256',
    'oadg_bottleneck_frozen_first_64', 'oadg_conv1x1_n16_fwd', 'oadg_conv1x1_n16_dgrad', 'oadg_conv1x1_n16_wgrad',
    'oadg_stem_conv7x7s2_nhwc_bf16',
    'oadg_bias_relu_maxpool_nhwc_bf16', 'oadg_fpn_topdown_fwd', 'oadg_fpn_topdown_bwd',
}


# ---------------------------------------------------------------------------------------------------- fp64 references
def _nhwc64(t):
    return t.detach().permute(0, 2, 3, 1).to(torch.float64)


def _taps(x, R, S, stride, pad, dil, Ho, Wo):
    """x [N,H,W,C] fp64 -> iterator of ((r, s), view [N,Ho,Wo,C]) of the zero-padded input under tap (r, s)"""
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    for r in range(R):
        for s in range(S):
            h0, w0 = r * dil, s * dil
            yield (r, s), xp[:, h0:h0 + stride * (Ho - 1) + 1:stride, w0:w0 + stride * (Wo - 1) + 1:stride, :]


def conv_ref(x, w, stride, pad, dil):
    """(r, S) [N,Ho,Wo,K] fp64 of conv(x, w) and of conv(|x|, |w|): per-tap fp64 GEMMs, one image at a time"""
    N, C, H, W = x.shape
    K, _, R, S_ = w.shape
    Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
    Wo = (W + 2 * pad - dil * (S_ - 1) - 1) // stride + 1
    w64 = w.detach().to(torch.float64)
    r = torch.zeros((N, Ho, Wo, K), dtype=torch.float64, device=x.device)
    a = torch.zeros_like(r)
    for n in range(N):
        xn = _nhwc64(x[n:n + 1])
        for (i, j), v in _taps(xn, R, S_, stride, pad, dil, Ho, Wo):
            m = v.reshape(-1, C)
            wk = w64[:, :, i, j].t()
            r[n].view(-1, K).addmm_(m, wk)
            a[n].view(-1, K).addmm_(m.abs(), wk.abs())
    return r, a


def wgrad_ref(x, gy, R, S_, stride, pad, dil):
    """(dW, S) [K,C,R,S] fp64 of the weight gradient of y = conv(x, W) for the output gradient gy (and over |x|, |gy|)"""
    N, C, H, W = x.shape
    K, Ho, Wo = gy.shape[1], gy.shape[2], gy.shape[3]
    dw = torch.zeros((K, C, R, S_), dtype=torch.float64, device=x.device)
    a = torch.zeros_like(dw)
    for n in range(N):
        xn = _nhwc64(x[n:n + 1])
        g = _nhwc64(gy[n:n + 1]).reshape(-1, K)
        for (i, j), v in _taps(xn, R, S_, stride, pad, dil, Ho, Wo):
            m = v.reshape(-1, C)
            dw[:, :, i, j] += g.t() @ m
            a[:, :, i, j] += g.abs().t() @ m.abs()
    return dw, a


def dgrad_s2_ref(gy, w, H, W, pad):
    """(dx, S) [N,H,W,C] fp64 of a stride-2 convolution's data gradient: dx[n, 2p + r - pad, 2q + s - pad] += gy[n,p,q] W[r,s]"""
    N, K, Ho, Wo = gy.shape
    _, C, R, S_ = w.shape
    w64 = w.detach().to(torch.float64)
    dx = torch.zeros((N, H + 2 * pad + 2, W + 2 * pad + 2, C), dtype=torch.float64, device=gy.device)
    a = torch.zeros_like(dx)
    for n in range(N):
        g = _nhwc64(gy[n:n + 1]).reshape(-1, K)
        for i in range(R):
            for j in range(S_):
                wk = w64[:, :, i, j]
                dx[n, i:i + 2 * Ho:2, j:j + 2 * Wo:2].add_((g @ wk).view(Ho, Wo, C))
                a[n, i:i + 2 * Ho:2, j:j + 2 * Wo:2].add_((g.abs() @ wk.abs()).view(Ho, Wo, C))
    return dx[:, pad:pad + H, pad:pad + W].contiguous(), a[:, pad:pad + H, pad:pad + W].contiguous()


def s2_filters(wt, K, C, R):
    """the forward filters W [K,C,R,R] of a stride-2 layer from its data-gradient parity-class filters (csrc
    prep_weights_channel, wt_mode 2: class blocks [C][taps][K] in the order (0,0) (0,1) (1,0) (1,1) at block offsets
    0, 1, 3, 5 x C K; 3x3 / pad 1: parity 0 uses the centre tap, parity 1 the taps 2 then 0)"""
    flat = wt.detach().permute(0, 2, 3, 1).reshape(-1)      # memory order of the channels_last [C,K,R,R] tensor
    w = torch.empty((K, C, R, R), dtype=wt.dtype, device=wt.device)
    if R == 1:
        w[:, :, 0, 0] = flat[:C * K].view(C, K).t()
        return w
    for r in range(3):
        for q in range(3):
            ph, pw = int(r != 1), int(q != 1)
            tr, tq = int(r == 0), int(q == 0)
            sc = 2 if pw else 1
            T = (2 if ph else 1) * sc
            off = (0, 1, 3, 5)[2 * ph + pw]
            blk = flat[off * C * K:(off + T) * C * K].view(C, T, K)
            w[:, :, r, q] = blk[:, tr * sc + tq, :].t()
    return w


def pack_bits(pos):
    """[N,H,W,K] bool -> uint8 [N*H*W*K/8]: bit e of byte j = element 8 j + e of the NHWC order (csrc ConvArgs.bits_in)"""
    b = pos.reshape(-1, 8).to(torch.int32) << torch.arange(8, device=pos.device, dtype=torch.int32)
    return b.sum(1).to(torch.uint8)


def unpack_bits(bits, shape):
    v = bits.reshape(-1, 1).to(torch.int32) >> torch.arange(8, device=bits.device, dtype=torch.int32)
    return (v & 1).bool().reshape(shape)


def _nearest(n_out, n_in, device):
    """source index of every destination index of F.interpolate(mode='nearest') from n_in to n_out"""
    src = torch.arange(n_in, dtype=torch.float64, device=device).view(1, 1, n_in)
    return F.interpolate(src, size=n_out, mode='nearest').view(-1).long()


def bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


def bound(r, S, rho, *extra):
    """elementwise bound; ``extra``: additional named terms already in absolute units"""
    b = rho * r.abs() + GAMMA * S + ALPHA
    for e in extra:
        b = b + e
    return b


def ratio(o, ref, b):
    """(worst err / bound, flat index of the worst element)"""
    e = (o.to(torch.float64) - ref).abs() / b
    e = torch.where(torch.isnan(e), torch.full_like(e, float('inf')), e)
    i = int(e.reshape(-1).argmax())
    return float(e.reshape(-1)[i]), i


def forward_expect(x, w, bias, residual, stride, pad, dil, relu, mask=None, mask_bits=None, res_up=False):
    """(expected y [N,Ho,Wo,K] fp64, bound) of conv_forward's contract: y = [relu](conv(x, w) + bias [+ residual |
    up2(residual)]) * (mask > 0) * bits, stored in bf16"""
    r, S = conv_ref(x, w, stride, pad, dil)
    if bias is not None:
        b64 = bias.detach().to(torch.float64)
        r += b64
        S += b64.abs()
    extra = []
    if residual is not None:
        # csrc finish_piece: the tile is rounded to bf16 BEFORE the residual is added (conv_mfma.hip: `v` comes from the
        # bf16 epilogue tile; the sum is rounded again on the store): one more rounding of conv + bias
        extra.append(RHO * r.abs())
        res = _nhwc64(residual)
        if res_up:
            res = res.repeat_interleave(2, 1).repeat_interleave(2, 2)
        r = r + res
        S = S + res.abs()
    b = bound(r, S, RHO, *extra)
    if relu:
        r = r.clamp_min(0)
    keep = None
    if mask is not None:
        keep = _nhwc64(mask) > 0
    if mask_bits is not None:
        kb = unpack_bits(mask_bits, r.shape)
        keep = kb if keep is None else keep & kb
    if keep is not None:
        r = r * keep
    return r, b


def colsum_expect(y_nhwc):
    """(sum over the pixels of the STORED output, S) per channel"""
    y = y_nhwc.to(torch.float64).reshape(-1, y_nhwc.shape[-1])
    return y.sum(0), y.abs().sum(0)


# ------------------------------------------------------------------------------------------- the integer-exact regime
# Operands that are small integers stored in bf16 (bias: fp32 integers): every product is exact in fp32 and so is every
# partial sum in ANY order while S - the same computation over absolute values - stays below 2^24.  A kernel then has
# exactly one admissible output: the fp64 integer for fp32 outputs, its round-to-nearest-even bf16 value for bf16 ones
# (tests/test_conv_stress.py).  The roundings are restated on the bit pattern, not taken from torch's cast.
EXACT_LIMIT = 2.0 ** 24


def _bits(t):
    """int32 bit patterns of fp64 values that are exact in fp32 (asserted)"""
    f = t.to(torch.float32)
    assert torch.equal(f.to(torch.float64), t.to(torch.float64)), 'value not exact in fp32'
    return f.contiguous().view(torch.int32)


def _unbits(b):
    return b.view(torch.float32).to(torch.float64)


def bf16_rne(t):
    """fp64 (exact in fp32) -> fp64 of its bf16 value, round to nearest, ties to even: bits + 0x7fff + (bit 16)"""
    b = _bits(t)
    return _unbits((b + 0x7fff + ((b >> 16) & 1)) & -65536)


def bf16_trunc(t):
    """the conversion that drops the low 16 bits (round towards zero): what RHO = 2^-8 would still admit"""
    return _unbits(_bits(t) & -65536)


def bf16_half_away(t):
    """round to nearest, ties away from zero: bits + 0x8000"""
    return _unbits((_bits(t) + 0x8000) & -65536)


def bf16_ties(t, live=None):
    """(down, up): how many elements are exact bf16 ties (low 16 bits 0x8000) that nearest-even rounds down / up in
    magnitude, among the ``live`` elements (those whose rounding reaches the stored output)"""
    b = _bits(t)
    tie = (b & 0xffff) == 0x8000
    if live is not None:
        tie = tie & live
    odd = ((b >> 16) & 1) == 1
    return int((tie & ~odd).sum()), int((tie & odd).sum())


def _keep(shape, mask, mask_bits):
    keep = None
    if mask is not None:
        keep = _nhwc64(mask) > 0
    if mask_bits is not None:
        kb = unpack_bits(mask_bits, shape)
        keep = kb if keep is None else keep & kb
    return keep


def forward_exact(x, w, bias, residual, stride, pad, dil, relu, mask=None, mask_bits=None, res_up=False):
    """conv_forward's contract on integer operands: (y [N,Ho,Wo,K] fp64 - the ONE admissible stored output, S, first, live).
    ``first`` = conv + bias, the fp32 value of the first rounding; without a residual y = relu(rne(first)), with one
    y = rne(relu(rne(first) + res)) (csrc finish_piece: the bf16 tile, then the sum rounded again); then mask and bits.
    ``live``: the elements whose first rounding reaches the output (not masked, not cut by the ReLU)."""
    r, S = conv_ref(x, w, stride, pad, dil)
    if bias is not None:
        b64 = bias.detach().to(torch.float64)
        r = r + b64
        S = S + b64.abs()
    first = r
    y = bf16_rne(r)
    if residual is not None:
        res = _nhwc64(residual)
        if res_up:
            res = res.repeat_interleave(2, 1).repeat_interleave(2, 2)
        S = S + res.abs()
        t = y + res
        y = bf16_rne(t.clamp_min(0) if relu else t)
    elif relu:
        y = y.clamp_min(0)
    live = (y != 0) if relu else torch.ones_like(y, dtype=torch.bool)
    keep = _keep(y.shape, mask, mask_bits)
    if keep is not None:
        y = y * keep
        live = live & keep
    return y, S, first, live


def dgrad_s2_exact(gy, w, H, W, pad, acc0=None, mask=None, mask_bits=None):
    """conv_dgrad_s2's contract on integer operands: (dx [N,H,W,C] fp64, S, first, live); ``acc0``: the deposit the launch
    adds in place (rne(rne(conv) + acc0))"""
    r, S = dgrad_s2_ref(gy, w, H, W, pad)
    first = r
    y = bf16_rne(r)
    if acc0 is not None:
        a = _nhwc64(acc0)
        S = S + a.abs()
        y = bf16_rne(y + a)
    live = torch.ones_like(y, dtype=torch.bool)
    keep = _keep(y.shape, mask, mask_bits)
    if keep is not None:
        y = y * keep
        live = keep
    return y, S, first, live


def wgrad_split_geometry(L, N, Ho, Wo, C, K, R, S_, splits):
    """pixels per split of a single-layer weight-gradient launch that returned ``splits`` partials: csrc wgrad_launch -
    ``chunks_per_split = ceil(nchunks / splits)`` 64-pixel chunks (conv_mfma.hip, `a.chunks_per_split = ...`), and for
    the 256-tile kernel on filters with taps and Wo % 64 == 0 whole output rows (wgrad_strip: per = ceil(N Ho / splits0)
    rows, splits = ceil(N Ho / per), splits0 = max(1, 256 / weight tiles) from wgrad256_splits).  Split s owns the pixels
    [s p, min((s + 1) p, P)) of the (n, ho, wo) order; a split past P owns none and must hold zeros."""
    P = N * Ho * Wo
    nchunks = (P + 63) // 64
    if L.oadg_conv2d_wgrad_variant(N, Ho, Wo, C, K, R, S_) == 256:
        s0 = max(1, 256 // ((K // 256) * (C // 256) * R * S_))
        rows = N * Ho
        if R * S_ > 1 and Wo % 64 == 0 and rows >= s0:
            per = -(-rows // s0)
            assert splits == -(-rows // per), (splits, rows, per)
            return per * Wo
        assert splits == s0, (splits, s0)
    return -(-nchunks // splits) * 64


def wgrad_parts_exact(x, gy, R, S_, stride, pad, dil, splits, pix):
    """(parts [splits][K][R*S][C] fp64, S [K][R*S][C]): the weight gradient over each split's pixel range
    [s pix, (s + 1) pix) on its own, in the layout of the fp32 workspace, and the sum over |x| |gy| of all pixels"""
    N, C, H, W = x.shape
    K, Ho, Wo = gy.shape[1], gy.shape[2], gy.shape[3]
    P = N * Ho * Wo
    g = torch.zeros((splits * pix, K), dtype=torch.float64, device=x.device)
    g[:P] = _nhwc64(gy).reshape(-1, K)[:splits * pix]
    assert P <= splits * pix
    g = g.view(splits, pix, K).transpose(1, 2)
    parts = torch.zeros((splits, K, R * S_, C), dtype=torch.float64, device=x.device)
    a = torch.zeros((K, R * S_, C), dtype=torch.float64, device=x.device)
    for (i, j), v in _taps(_nhwc64(x), R, S_, stride, pad, dil, Ho, Wo):
        m = torch.zeros((splits * pix, C), dtype=torch.float64, device=x.device)
        m[:P] = v.reshape(-1, C)
        m = m.view(splits, pix, C)
        parts[:, :, i * S_ + j, :] = torch.bmm(g, m)
        a[:, i * S_ + j, :] = torch.bmm(g.abs(), m.abs()).sum(0)
    return parts, a


def frozen_block_exact(x, ws, bs, downsample):
    """csrc bottleneck_frozen.hip on integer operands, rounded as frozen_block_expect documents: (y fp64, [S of every
    stage], first, live)"""
    def stage(inp, w, b, pad):
        r, S = conv_ref(inp, w, 1, pad, 1)
        b64 = b.detach().to(torch.float64)
        return r + b64, S + b64.abs()
    r1, S1 = stage(x, ws[0], bs[0], 0)
    t1 = bf16_rne(r1.clamp_min(0))
    r2, S2 = stage(t1.permute(0, 3, 1, 2), ws[1], bs[1], 1)
    t2 = bf16_rne(r2.clamp_min(0))
    r3, S3 = stage(t2.permute(0, 3, 1, 2), ws[2], bs[2], 0)
    Ss = [S1, S2, S3]
    if downsample:
        rd, Sd = stage(x, ws[3], bs[3], 0)
        Ss.append(Sd)
        s = bf16_rne(rd)
    else:
        s = _nhwc64(x)
    t = bf16_rne(r3) + s
    y = bf16_rne(t.clamp_min(0))
    return y, Ss, (r1, r2, r3), y != 0


def tile_width(M, K):
    """output channels per workgroup of the 128-pixel tile family (variants 1 and 3): csrc conv_launch,
    `const int tbn = (K % BN == 0 && m_tiles * (K / BN) > tbn64_max) ? BN : 64` with BN = 128, m_tiles = ceil(M / 128) and
    tbn64_max = 256 - the 64-wide tile whenever 128-wide tiles would leave compute units without a workgroup"""
    return 128 if (K % 128 == 0 and -(-M // 128) * (K // 128) > 256) else 64


def frozen_block_expect(x, ws, bs, downsample):
    """csrc bottleneck_frozen.hip: y = relu(bf16(conv3(t2) + b3) + s), t2 = bf16(relu(conv2(t1) + b2)),
    t1 = bf16(relu(conv1(x) + b1)), s = x (identity block) or bf16(convd(x) + bd).  Errors of the rounded intermediates
    propagate through the later convolutions as conv(|W|, error bound)."""
    def stage(inp, w, b, pad, e_in):
        r, S = conv_ref(inp, w, 1, pad, 1)
        b64 = b.detach().to(torch.float64)
        r, S = r + b64, S + b64.abs()
        e = GAMMA * S + ALPHA
        if e_in is not None:
            # the input's own error bound carried through this convolution
            ec, _ = conv_ref(e_in.permute(0, 3, 1, 2), w.detach().to(torch.float64).abs(), 1, pad, 1)
            e = e + ec
        return r, e
    # stage 1 / 2: bf16 rounding of the ReLU output in LDS (bottleneck_frozen.hip, `pack2(fmaxf(acc + b, 0))`)
    r1, e1 = stage(x, ws[0], bs[0], 0, None)
    t1 = r1.clamp_min(0)
    e1 = e1 + RHO * t1
    x1 = bf16(t1).permute(0, 3, 1, 2)
    r2, e2 = stage(x1, ws[1], bs[1], 1, e1)
    t2 = r2.clamp_min(0)
    e2 = e2 + RHO * t2
    r3, e3 = stage(bf16(t2).permute(0, 3, 1, 2), ws[2], bs[2], 0, e2)
    e3 = e3 + RHO * r3.abs()      # `bf16_to_f32(f32_to_bf16(acc + b3))` before the shortcut add
    if downsample:
        rd, ed = stage(x, ws[3], bs[3], 0, None)
        e3 = e3 + ed + RHO * rd.abs()       # `bf16_to_f32(f32_to_bf16(accd + bd))`
        s = rd
    else:
        s = _nhwc64(x)
    r = r3 + s
    b = RHO * r.abs() + e3
    return r.clamp_min(0), b


def bn_fold_expect(w, gamma, beta, mean, var, eps, bias_in):
    """fp64 (Wf, b, scale) of the BN fold Wf = W g / sqrt(v + eps), b = beta - mean g / sqrt(v + eps)"""
    w64 = w.detach().to(torch.float64)
    K = w64.shape[0]
    if gamma is None:
        b = bias_in.detach().to(torch.float64) if bias_in is not None else None
        return w64, b, torch.ones(K, dtype=torch.float64, device=w64.device)
    sc = gamma.detach().to(torch.float64) / torch.sqrt(var.detach().to(torch.float64) + eps)
    b = beta.detach().to(torch.float64) - mean.detach().to(torch.float64) * sc
    return w64 * sc.view(-1, 1, 1, 1), b, sc


def bn_chain_expect(dwf, s_dwf, db, s_db, w, gamma, mean, var, eps):
    """fp64 (dW, S_dW, dgamma, S_dgamma) of the BN fold's chain rule: dW = dWf g / sqrt(v + eps),
    dgamma = (sum dWf W - db mean) / sqrt(v + eps)  (dbeta = db)"""
    w64 = w.detach().to(torch.float64)
    inv = 1.0 / torch.sqrt(var.detach().to(torch.float64) + eps)
    sc = gamma.detach().to(torch.float64) * inv
    m = mean.detach().to(torch.float64)
    dW = dwf * sc.view(-1, 1, 1, 1)
    SdW = s_dwf * sc.abs().view(-1, 1, 1, 1)
    dg = ((dwf * w64).sum((1, 2, 3)) - db * m) * inv
    Sdg = ((s_dwf * w64.abs()).sum((1, 2, 3)) + s_db * m.abs()) * inv
    return dW, SdW, dg, Sdg


# ----------------------------------------------------------------------------------------------------------- auditor
class Row:
    __slots__ = ('calls', 'shapes', 'worst', 'where')

    def __init__(self):
        self.calls, self.shapes, self.worst, self.where = 0, set(), 0.0, None


class Auditor:
    def __init__(self):
        self.table = {}
        self.wrappers = {}           # wrapper name -> calls
        self.params = {}             # id(param) -> [param, kind, ref, S, handover-rounding term or None]
        self.bf16_handover = set()   # bank entries whose weight gradient reached the BN-fold chain rule in bf16
        self.narrow = None           # [dW, S, db, S_db] fp64 of the narrow RPN head's weight / bias over the step's calls
        self.kernels = set()         # the kernel instantiations whose launches were audited
        self.last = None             # the instantiation of the latest audited launch
        self.regime = None           # tests/test_conv_stress.py: the operand regime, kept apart in the table's rows
        self.failures = []

    # -- bookkeeping
    def hit(self, wrapper):
        self.wrappers[wrapper] = self.wrappers.get(wrapper, 0) + 1

    def record(self, kernel, shape, o, ref, b, check=None, launched=True):
        """one row per (kernel, check): ``check`` names a further output of the launch (its bits, column sums, bias,
        layouts) or a value the kernel wrote earlier; ``launched``: ``kernel`` ran in this audited call"""
        rt, i = ratio(o, ref, b)
        if launched:
            self.kernels.add(kernel)
            self.last = kernel
        if self.regime is not None:
            check = '[%s]' % self.regime if check is None else '[%s] %s' % (self.regime, check)
        kernel = kernel if check is None else '%s %s' % (kernel, check)
        row = self.table.setdefault(kernel, Row())
        row.calls += 1
        row.shapes.add(tuple(shape))
        if rt > row.worst or row.where is None:
            row.worst = max(rt, row.worst)
            row.where = (tuple(shape), i, float(o.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(b.reshape(-1)[i]))
        if not rt <= 1.0:
            self.failures.append((kernel, tuple(shape), rt, row.where))
        return rt

    def exact(self, kernel, shape, o, ref, check='exact integers'):
        """``o`` must EQUAL ``ref`` (torch.equal: the integer-exact regime has one admissible output); booked as a row whose
        bound, the absolute floor, makes any difference a failure"""
        o64, r64 = o.detach().to(torch.float64), ref.detach().to(torch.float64)
        same = o64.shape == r64.shape and torch.equal(o64, r64)
        if o64.shape != r64.shape:
            self.failures.append(('%s %s' % (kernel, check), tuple(shape), 'shape', (tuple(o64.shape), tuple(r64.shape))))
            return False
        rt = self.record(kernel, shape, o64, r64, torch.full_like(r64, ALPHA), check=check, launched=False)
        assert same == (rt == 0.0), (kernel, check, same, rt)
        return same

    def worst(self):
        return max((r.worst for r in self.table.values()), default=0.0)

    def print_table(self, title):
        print('\n== conv audit: %s ==' % title)
        print('%-62s %6s %10s  %s' % ('kernel', 'calls', 'err/bound', 'worst element (shape, index, out, ref, bound)'))
        for k in sorted(self.table):
            r = self.table[k]
            print('%-62s %6d %10.4f  %s' % (k, r.calls, r.worst, r.where))
        print('wrappers:', dict(sorted(self.wrappers.items())))

    # -- installation
    def install(self, mp):
        from oadg_amd import hip_conv, hip_ops
        self.hc, self.ho = hip_conv, hip_ops
        L = hip_conv._lib.lib()
        A = self

        def sync():
            torch.cuda.synchronize()

        def nograd(fn):
            def g(*a, **k):
                with torch.no_grad(), torch.autocast('cuda', enabled=False):
                    return fn(*a, **k)
            return g

        orig = {n: getattr(hip_conv, n) for n in ('conv_forward', 'conv_dgrad_s2', 'conv_wgrad', 'conv_wgrad_parts',
                                                  'wgrad_multi', 'relu_bias_bwd', '_colsum', 'resolve_colsum',
                                                  'flush_colsums', 'frozen_bottleneck')}
        last_part = []

        def _colsum(part, K):
            A.hit('_colsum')
            last_part.append(part)
            return orig['_colsum'](part, K)

        def conv_forward(x, w, bias, residual, stride, pad, dil, relu, variant=0, mask=None, want_colsum=False,
                         mask_bits=None, bits_out=None, res_up=False):
            A.hit('conv_forward')
            N, C, H, W = x.shape
            K, _, R, S_ = w.shape
            v = int(variant) or L.oadg_conv2d_auto_variant(N, H, W, C, K, R, S_, stride, pad, dil)
            if v == 4 and (mask is not None or (mask_bits is not None and bits_out is not None)):
                v = 3
            name = hip_conv.kernel_name(v, C, K, R, S_, stride, pad, residual is not None, mask is not None,
                                        mask_bits is not None, bits_out is not None)
            if v in (1, 3):
                # hip_conv.kernel_name knows the tile width by K % 128 only; conv_launch also takes the 64-wide tile on
                # small maps (tile_width restates its rule): book the launch under the instantiation that ran
                Ho = (H + 2 * pad - dil * (R - 1) - 1) // stride + 1
                Wo = (W + 2 * pad - dil * (S_ - 1) - 1) // stride + 1
                name = name.replace('conv_igemm_kernel<%d,' % (128 if K % 128 == 0 else 64),
                                    'conv_igemm_kernel<%d,' % tile_width(N * Ho * Wo, K), 1)
            mb = mask_bits.clone() if mask_bits is not None else None
            del last_part[:]
            out = orig['conv_forward'](x, w, bias, residual, stride, pad, dil, relu, variant, mask, want_colsum, mask_bits,
                                       bits_out, res_up)
            sync()
            y = out[0] if want_colsum else out
            nograd(A._check_forward)(name, x, w, bias, residual, stride, pad, dil, relu, mask, mb, bits_out, res_up, y,
                                     last_part[-1] if want_colsum else None)
            return out

        def conv_dgrad_s2(gy, wt, xshape, R, mask=None, want_colsum=False, mask_bits=None, accumulate=None):
            A.hit('conv_dgrad_s2')
            C = xshape[1]
            post = accumulate is not None or mask is not None or mask_bits is not None
            name = 'conv_igemm_s2_kernel<%d, %s>' % (128 if C % 128 == 0 else 64, 'true' if post else 'false')
            acc0 = accumulate.clone() if accumulate is not None else None
            del last_part[:]
            out = orig['conv_dgrad_s2'](gy, wt, xshape, R, mask, want_colsum, mask_bits, accumulate)
            sync()
            gx = out[0] if want_colsum else out
            nograd(A._check_dgrad_s2)(name, gy, wt, xshape, R, mask, mask_bits, acc0, gx,
                                      last_part[-1] if want_colsum else None)
            return out

        def conv_wgrad(x16, gy16, K, R, S_, stride, pad, dil):
            A.hit('conv_wgrad')
            dw = orig['conv_wgrad'](x16, gy16, K, R, S_, stride, pad, dil)
            sync()
            nograd(A._check_wgrad)(A._wgrad_name(L, x16, gy16, K, R, S_) + ' (+reduce)', x16, gy16, K, R, S_, stride, pad,
                                   dil, dw.permute(0, 2, 3, 1).reshape(1, -1))
            return dw

        def conv_wgrad_parts(x16, gy16, K, R, S_, stride, pad, dil):
            A.hit('conv_wgrad_parts')
            ws, splits = orig['conv_wgrad_parts'](x16, gy16, K, R, S_, stride, pad, dil)
            sync()
            C = x16.shape[1]
            parts = ws[:splits * K * R * S_ * C * 4].view(torch.float32).view(splits, -1)
            nograd(A._check_wgrad)(A._wgrad_name(L, x16, gy16, K, R, S_), x16, gy16, K, R, S_, stride, pad, dil, parts)
            return ws, splits

        def wgrad_multi(jobs, target_blocks=256):
            A.hit('wgrad_multi')
            ws, parts = orig['wgrad_multi'](jobs, target_blocks)
            sync()
            base = ws.data_ptr()
            for (x16, gy16, K, R, S_, stride, pad, dil), (p, splits) in zip(jobs, parts):
                C = x16.shape[1]
                n = splits * K * R * S_ * C
                off = p - base
                pt = ws[off:off + 4 * n].view(torch.float32).view(splits, -1)
                nograd(A._check_wgrad)('conv_wgrad256_multi_kernel', x16, gy16, K, R, S_, stride, pad, dil, pt)
            return ws, parts

        def relu_bias_bwd(gy, y, want_bias):
            A.hit('relu_bias_bwd')
            g, db = orig['relu_bias_bwd'](gy, y, want_bias)
            sync()
            nograd(A._check_relu_bias)(gy, y, g, db)
            return g, db

        def resolve_colsum(t):
            A.hit('resolve_colsum')
            ent = hip_conv.pending_colsum(t)
            part = ent.part if ent is not None else None
            out = orig['resolve_colsum'](t)
            if part is not None:
                sync()
                nograd(A._check_reduce)('colsum_reduce_kernel', part, ent.out)
            return out

        def flush_colsums():
            A.hit('flush_colsums')
            pend = [(e.part, e.out, None if e.fix is None else (e.fix[0].clone(),) + tuple(e.fix)) for e in hip_conv._PENDING]
            n = orig['flush_colsums']()
            sync()
            for part, out, fix in pend:
                nograd(A._check_reduce)('colsum_reduce_multi_kernel', part, out, fix)
            return n

        def frozen_bottleneck(x, block):
            A.hit('frozen_bottleneck')
            y = orig['frozen_bottleneck'](x, block)
            if y is not None:
                sync()
                nograd(A._check_frozen)(x, block, y)
            return y

        for n, f in (('conv_forward', conv_forward), ('conv_dgrad_s2', conv_dgrad_s2), ('conv_wgrad', conv_wgrad),
                     ('conv_wgrad_parts', conv_wgrad_parts), ('wgrad_multi', wgrad_multi),
                     ('relu_bias_bwd', relu_bias_bwd), ('_colsum', _colsum), ('resolve_colsum', resolve_colsum),
                     ('flush_colsums', flush_colsums), ('frozen_bottleneck', frozen_bottleneck)):
            mp.setattr(hip_conv, n, f)

        # _PrepWeights forward / backward, the bank refresh
        pw_fwd, pw_bwd = hip_conv._PrepWeights.forward, hip_conv._PrepWeights.backward

        def prep_forward(ctx, w, gamma, beta, mean, var, eps, bias_in, want_wt, wtoken=None, entry=None):
            A.hit('_PrepWeights.forward')
            served = entry is not None and entry.valid      # prepared by an earlier refresh / forward: nothing launches
            outs = pw_fwd(ctx, w, gamma, beta, mean, var, eps, bias_in, want_wt, wtoken, entry)
            sync()
            nograd(A._check_prep)('prep_weights_multi_kernel' if served else 'prep_weights_kernel', w, gamma, beta, mean, var, eps, bias_in, int(want_wt),
                                  outs[0], outs[1] if outs[1].numel() else None, outs[2] if outs[2].numel() else None,
                                  launched=not served, what='(served from the bank)' if served else None)
            return outs

        def prep_backward(ctx, gwf, gbias, gwt):
            A.hit('_PrepWeights.backward')
            tok = ctx.wtoken
            if gwf is not None and (tok is None or tok.parts is None) and gwf.stride() != (0, 0, 0, 0):
                # the weight gradient arrives as a tensor and is handed to oadg_prep_conv_weights_bwd in bf16
                # (hip_conv._PrepWeights.backward: `gwf = gwf.to(torch.bfloat16)`)
                A.bf16_handover.add(id(ctx.entry) if ctx.entry is not None else id(tok))
            return pw_bwd(ctx, gwf, gbias, gwt)

        mp.setattr(hip_conv._PrepWeights, 'forward', staticmethod(prep_forward))
        mp.setattr(hip_conv._PrepWeights, 'backward', staticmethod(prep_backward))
        refresh = hip_conv._Bank.refresh

        def bank_refresh(bank):
            A.hit('_Bank.refresh')
            n = refresh(bank)
            sync()
            for e in list(bank.entries):
                if e.args is None or e.versions is None:
                    continue
                w, g_, b_, m_, v_, eps, bi_, K, C, R, S_, krsc, want_wt = e.args
                wsrc = e.src[0]
                nograd(A._check_prep)('prep_weights_multi_kernel', wsrc, g_, b_, m_, v_, eps, bi_, want_wt, e.wf, e.bias,
                                      e.wt)
            return n
        mp.setattr(hip_conv._Bank, 'refresh', bank_refresh)

        # the layers' backward: parameter-level references (fp64 dWf, db of the operands each weight gradient received)
        cb = hip_conv._Conv2dMFMA.backward

        def conv_backward(ctx, gy):
            A.hit('_Conv2dMFMA.backward')
            x16, wf, wt, y = ctx.saved_tensors
            stride, pad, dil, has_bias = ctx.cfg[:4]
            ent = ctx.wtoken.entry if ctx.wtoken is not None else None
            if ctx.wtoken is not None and ctx.needs_input_grad[1]:
                # (no bank entry: a weight built by autograd ops each step - the fused RPN head's [rpn_cls; rpn_reg; 0]
                #  of dense_heads.py - keyed by its weight-gradient token, mapped to its parameters by check_params)
                nograd(A._param_ref)(ent if ent is not None else ctx.wtoken, x16, wf, y, gy, stride, pad, dil)
            outs = cb(ctx, gy)
            if ctx.res_up is not None and outs[3] is not None:
                # the fused FPN top-down add's backward, launched inline (oadg_fpn_topdown_bwd): the coarser level's
                # gradient = the 2 x 2 sums of bf16(gy)
                A.hit('_Conv2dMFMA.backward res_up')
                sync()
                nograd(A._check_topdown_bwd)(gy, outs[3], '(lateral res_up)')
            return outs
        mp.setattr(hip_conv._Conv2dMFMA, 'backward', staticmethod(conv_backward))

        # the narrow RPN head
        nf, nb = hip_conv._NarrowHead.forward, hip_conv._NarrowHead.backward

        def narrow_forward(ctx, w_cat, b_cat, w16, wt16, b16, toks, *xs):
            A.hit('_NarrowHead.forward')
            ys = nf(ctx, w_cat, b_cat, w16, wt16, b16, toks, *xs)
            sync()
            for x, y in zip(xs, ys):
                C = x.shape[1]
                r, b = nograd(forward_expect)(hip_conv._nhwc_bf16(x), w16.view(16, C, 1, 1), b16, None, 1, 0, 1, False)
                A.record('n16_fwd_kernel<%d>' % C, x.shape, nograd(_nhwc64)(y), r, b)
            return ys

        def narrow_backward(ctx, *gys):
            A.hit('_NarrowHead.backward')
            wt16, *xs16 = ctx.saved_tensors
            state = [(tok.bits if tok is not None else None, tok is not None and tok.masked,
                      tok.extra.clone() if (tok is not None and tok.extra is not None) else None) for tok in ctx.toks]
            outs = nb(ctx, *gys)
            sync()
            nograd(A._check_narrow_bwd)(ctx, wt16, xs16, gys, state, outs)
            return outs
        mp.setattr(hip_conv._NarrowHead, 'forward', staticmethod(narrow_forward))
        mp.setattr(hip_conv._NarrowHead, 'backward', staticmethod(narrow_backward))

        # hip_ops: stem, bias + ReLU + max-pool, FPN top-down add
        so, bm = hip_ops.stem_conv, hip_ops.bias_relu_maxpool

        def stem_conv(x, wp):
            A.hit('stem_conv')
            y = so(x, wp)
            sync()
            w = wp[:, :, 1:, :3].permute(0, 3, 1, 2)          # hip_ops.stem_weights: [64][7][8][4], pixel 0 / channel 3 zero
            r, b = nograd(forward_expect)(x, w, None, None, 2, 3, 1, False)
            A.record('stem_conv7x7s2_kernel', x.shape, nograd(_nhwc64)(y), r, b)
            return y

        def bias_relu_maxpool(x, bias):
            A.hit('bias_relu_maxpool')
            y = bm(x, bias)
            sync()
            with torch.no_grad():
                # csrc bias_relu_maxpool_kernel casts the bias to bf16 as autocast would (`bf16_to_f32(f32_to_bf16(bias))`):
                # the operand the sum receives
                t = x.detach().double() + (bf16(bias.detach().double()).view(1, -1, 1, 1) if bias is not None else 0)
                r = F.max_pool2d(t.clamp_min(0), 3, 2, 1)
                A.record('bias_relu_maxpool_kernel', x.shape, _nhwc64(y), _nhwc64(r), bound(_nhwc64(r), 0, RHO))
            return y
        mp.setattr(hip_ops, 'stem_conv', stem_conv)
        mp.setattr(hip_ops, 'bias_relu_maxpool', bias_relu_maxpool)
        tf, tb = hip_ops._FpnTopDown.forward, hip_ops._FpnTopDown.backward

        def td_forward(ctx, lat, top):
            A.hit('_FpnTopDown.forward')
            out = tf(ctx, lat, top)
            sync()
            with torch.no_grad():
                ih, iw = _nearest(lat.shape[2], top.shape[2], lat.device), _nearest(lat.shape[3], top.shape[3], lat.device)
                r = _nhwc64(lat) + _nhwc64(top)[:, ih][:, :, iw]
                A.record('fpn_topdown_fwd_kernel', lat.shape, _nhwc64(out), r, bound(r, 0, RHO))
            return out

        def td_backward(ctx, g):
            A.hit('_FpnTopDown.backward')
            outs = tb(ctx, g)
            sync()
            if outs[1] is not None:
                nograd(A._check_topdown_bwd)(g, outs[1], None)
            return outs
        mp.setattr(hip_ops._FpnTopDown, 'forward', staticmethod(td_forward))
        mp.setattr(hip_ops._FpnTopDown, 'backward', staticmethod(td_backward))
        return self

    # -- per-launch checks
    @staticmethod
    def _wgrad_name(L, x16, gy16, K, R, S_):
        v = L.oadg_conv2d_wgrad_variant(x16.shape[0], gy16.shape[2], gy16.shape[3], x16.shape[1], K, R, S_)
        return 'conv_wgrad256_kernel' if v == 256 else 'conv_wgrad_kernel<%d>' % v

    def _check_topdown_bwd(self, g, dtop, check):
        """d top[n, h, w] = sum of bf16(g) over the destination pixels whose nearest source is (h, w)"""
        g16 = bf16(_nhwc64(g))
        N, H, W, C = g16.shape
        Ht, Wt = dtop.shape[2], dtop.shape[3]
        ih, iw = _nearest(H, Ht, g.device), _nearest(W, Wt, g.device)
        r = torch.zeros((N, Ht, W, C), dtype=torch.float64, device=g.device).index_add_(1, ih, g16)
        Sa = torch.zeros_like(r).index_add_(1, ih, g16.abs())
        r = torch.zeros((N, Ht, Wt, C), dtype=torch.float64, device=g.device).index_add_(2, iw, r)
        Sa = torch.zeros_like(r).index_add_(2, iw, Sa)
        self.record('fpn_topdown_bwd_kernel', g.shape, _nhwc64(dtop), r, bound(r, Sa, RHO), check=check)

    def _check_forward(self, name, x, w, bias, residual, stride, pad, dil, relu, mask, mask_bits, bits_out, res_up, y,
                       part):
        r, b = forward_expect(x, w, bias, residual, stride, pad, dil, relu, mask, mask_bits, res_up)
        o = _nhwc64(y)
        self.record(name, tuple(x.shape) + tuple(w.shape), o, r, b)
        if bits_out is not None:
            ok = torch.equal(bits_out, pack_bits(o > 0))
            self.record(name, x.shape, torch.zeros(1, device=o.device, dtype=torch.float64),
                        torch.zeros(1, device=o.device, dtype=torch.float64) + (0.0 if ok else 1.0),
                        torch.full((1,), ALPHA, device=o.device, dtype=torch.float64), check='bits_out')
        if part is not None:
            cs, S = colsum_expect(o)
            self.record(name, x.shape, part.to(torch.float64).sum(0), cs, bound(cs, S, 0.0), check='colsum')
        del r, b, o

    def _check_dgrad_s2(self, name, gy, wt, xshape, R, mask, mask_bits, acc0, gx, part):
        N, C, H, W = xshape
        K = gy.shape[1]
        w = s2_filters(wt, K, C, R)
        r, S = dgrad_s2_ref(gy, w, H, W, 1 if R == 3 else 0)
        extra = []
        if acc0 is not None:
            # the deposit is read from bf16 and the sum stored in bf16; the convolution's own value is rounded first
            # (finish_piece: bf16 tile + residual)
            extra.append(RHO * r.abs())
            a = _nhwc64(acc0)
            r, S = r + a, S + a.abs()
        b = bound(r, S, RHO, *extra)
        keep = None
        if mask is not None:
            keep = _nhwc64(mask) > 0
        if mask_bits is not None:
            kb = unpack_bits(mask_bits, r.shape)
            keep = kb if keep is None else keep & kb
        if keep is not None:
            r = r * keep
        o = _nhwc64(gx)
        self.record(name, tuple(gy.shape) + (C, R), o, r, b)
        if part is not None:
            cs, Sc = colsum_expect(o)
            self.record(name, gy.shape, part.to(torch.float64).sum(0), cs, bound(cs, Sc, 0.0), check='colsum')

    def _check_wgrad(self, name, x16, gy16, K, R, S_, stride, pad, dil, parts):
        dw, S = wgrad_ref(x16, gy16, R, S_, stride, pad, dil)
        got = parts.to(torch.float64).sum(0).view(K, R, S_, -1).permute(0, 3, 1, 2)
        self.record(name, tuple(x16.shape) + (K, R, stride, dil), got, dw, bound(dw, S, 0.0))

    def _check_relu_bias(self, gy, y, g, db):
        g0 = bf16(_nhwc64(gy))
        if y is not None:
            g0 = g0 * (_nhwc64(y) > 0)
        # the reference IS the rounded value: bf16(gy) * (y > 0) must come out exactly (a truncating cast would not)
        self.record('relu_bias_bwd_kernel', gy.shape, _nhwc64(g), g0, bound(g0, 0, 0.0))
        if db is not None:
            o = _nhwc64(g).reshape(-1, g.shape[1])
            self.record('relu_bias_bwd_kernel', gy.shape, db, o.sum(0), bound(o.sum(0), o.abs().sum(0), 0.0), check='colsum')

    def _check_reduce(self, name, part, out, fix=None):
        p = part.to(torch.float64)
        r, S = p.sum(0), p.abs().sum(0)
        self.record(name, part.shape, out, r, bound(r, S, 0.0))
        if fix is not None:
            raw, dg, mean, var, eps = fix
            inv = 1.0 / torch.sqrt(var.double() + eps)
            ref = (raw.double() - out.double() * mean.double()) * inv
            Sg = (raw.double().abs() + out.double().abs() * mean.double().abs()) * inv
            self.record(name, part.shape, dg, ref, bound(ref, Sg, 0.0), check='dgamma')

    def _check_frozen(self, x, block, y):
        hc = self.hc
        convs, bns = [block.conv1, block.conv2, block.conv3], [block.bn1, block.bn2, block.bn3]
        ds = block.downsample is not None
        if ds:
            convs.append(block.downsample[0])
            bns.append(block.downsample[1])
        ws, bs = [], []
        for c, bn in zip(convs, bns):
            wf, b, _ = hc.prepared(c.weight, bn, None, 0, c)     # the cached bf16 operands the launch received
            # (folded once, when the block first ran, and cached on the module: checked here against its source)
            self._check_prep('prep_weights_kernel', c.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps,
                             None, 0, wf, b, None, launched=False, what='(cached frozen fold)')
            ws.append(wf)
            bs.append(b)
        r, b = frozen_block_expect(x, ws, bs, ds)
        self.record('bottleneck_frozen_first_kernel' if ds else 'bottleneck_frozen_kernel', x.shape, _nhwc64(y), r, b)

    def _check_prep(self, name, w, gamma, beta, mean, var, eps, bias_in, want_wt, wf, bias, wt, launched=True, what=None):
        """``what``: the prepared tensors were written earlier (a bank refresh, a cached frozen fold), not by this call"""
        wf64, b64, sc = bn_fold_expect(w, gamma, beta, mean, var, eps, bias_in)
        K, C, R, S_ = wf64.shape
        sub = lambda c: c if what is None else '%s %s' % (what, c)  # noqa: E731
        # scale = g * rsqrtf(v + eps) in fp32 before the product is rounded: GAMMA |Wf|
        self.record(name, wf64.shape, wf.double(), wf64, bound(wf64, wf64.abs(), RHO), check=what, launched=launched)
        if b64 is not None:
            Sb = (beta.double().abs() + (mean.double() * sc).abs()) if gamma is not None else b64.abs()
            self.record(name, wf64.shape, bias.double(), b64, bound(b64, Sb, 0.0), check=sub('bias'), launched=launched)
        if wt is not None:
            if want_wt == 2:
                back = s2_filters(wt, K, C, R)
            else:     # [C][R][S][K] flipped / transposed
                back = wt.detach().permute(1, 0, 2, 3).flip(2, 3)
            exact = torch.zeros(1, dtype=torch.float64, device=wf.device) + float(not torch.equal(back, wf.detach()))
            self.record(name, wf64.shape, torch.zeros_like(exact), exact,
                        torch.full((1,), ALPHA, dtype=torch.float64, device=wf.device), check=sub('wt(mode %d)' % want_wt),
                        launched=launched)

    def _check_narrow_bwd(self, ctx, wt16, xs16, gys, state, outs):
        C = xs16[0].shape[1]
        KN = ctx.meta[0]
        w = wt16.t().contiguous().view(16, C)
        dw = S = db = Sdb = None
        for l, (x16, gy, (bits, masked, extra)) in enumerate(zip(xs16, gys, state)):
            g = torch.zeros((x16.shape[0], 16) + tuple(x16.shape[2:]), dtype=torch.bfloat16, device=x16.device) \
                if gy is None else gy
            g64 = bf16(_nhwc64(g))
            gx = outs[6 + l]
            if gx is not None:
                r = (g64.reshape(-1, 16) @ w.double()).view(g64.shape[:3] + (C,))
                Sa = (g64.abs().reshape(-1, 16) @ w.double().abs()).view(r.shape)
                if extra is None:
                    b = bound(r, Sa, RHO)
                    if masked and bits is not None:
                        r = r * unpack_bits(bits, r.shape)
                else:
                    # gx + extra in torch: the launch's bf16 output rounded, then the bf16 sum (two roundings)
                    e = _nhwc64(extra)
                    b = bound(r + e, Sa + e.abs(), RHO, RHO * r.abs())
                    r = r + e
                self.record('n16_dgrad_kernel<%d>' % C, x16.shape, _nhwc64(gx), r, b)
            x64 = _nhwc64(x16).reshape(-1, C)
            gg = g64.reshape(-1, 16)
            d, s_ = gg.t() @ x64, gg.abs().t() @ x64.abs()
            dw, S = (d, s_) if dw is None else (dw + d, S + s_)
            db = gg.sum(0) if db is None else db + gg.sum(0)
            Sdb = gg.abs().sum(0) if Sdb is None else Sdb + gg.abs().sum(0)
        if outs[0] is not None:
            self.record('n16_wgrad_kernel<%d>' % C, xs16[0].shape, outs[0].reshape(KN, C), dw[:KN], bound(dw[:KN], S[:KN], 0.0))
        if outs[1] is not None:
            self.record('n16_wgrad_kernel<%d>' % C, xs16[0].shape, outs[1], db[:KN], bound(db[:KN], Sdb[:KN], 0.0),
                        check='bias')
        # parameter level: the [rpn_cls; rpn_reg] rows, summed over the step's calls (check_params)
        if self.narrow is None:
            self.narrow = [dw[:KN], S[:KN], db[:KN], Sdb[:KN]]
        else:
            for a, v in zip(self.narrow, (dw[:KN], S[:KN], db[:KN], Sdb[:KN])):
                a += v

    # -- parameter level
    def _param_ref(self, ent, x16, wf, y, gy, stride, pad, dil):
        """fp64 dWf / db of this call (g = bf16(gy) * (y > 0): what the weight-gradient launch and the bias reduction
        receive), summed per bank entry over the calls of the step"""
        g = gy.detach().to(torch.bfloat16)
        if y is not None:
            g = g * (y > 0)
        K, C, R, S_ = wf.shape
        dwf, S = wgrad_ref(x16, g, R, S_, stride, pad, dil)
        g64 = _nhwc64(g).reshape(-1, K)
        db, Sdb = g64.sum(0), g64.abs().sum(0)
        acc = self.params.get(id(ent))
        if acc is None:
            self.params[id(ent)] = [ent, dwf, S, db, Sdb, 1]
        else:
            acc[1] += dwf
            acc[2] += S
            acc[3] += db
            acc[4] += Sdb
            acc[5] += 1

    def head_rows(self):
        """(fp64 [dW, S, db, S_db] of the RPN head's output rows [rpn_cls; rpn_reg; zero padding], how it ran) - from the
        narrow head, or from the one unbanked 1x1 convolution (the fused 128-channel head), or None"""
        if self.narrow is not None:
            return self.narrow, '(narrow head)'
        fused = [v for v in self.params.values() if not hasattr(v[0], 'src') and v[1].shape[2:] == (1, 1)]
        if len(fused) == 1:
            _, dwf, S, db, Sdb, _ = fused[0]
            return [dwf.flatten(1), S.flatten(1), db, Sdb], '(fused head)'
        return None, None

    def check_params(self, named, head_convs=()):
        """compare every audited parameter's .grad with its fp64 reference; returns the set of parameter names checked.
        ``head_convs``: the 1x1 convolutions whose weights / biases make up the RPN head's rows, in order (dense_heads.py
        _narrow_head_params / _fused_head_params: [rpn_cls; rpn_reg], the fused head zero-padded to 128 rows)"""
        names = {id(p): n for n, p in named}
        seen = set()
        rows, how = self.head_rows()
        with torch.no_grad():
            if rows is not None and head_convs:
                dw, S, db, Sdb = rows
                k0 = 0
                for conv in head_convs:
                    k1 = k0 + conv.weight.shape[0]
                    for p, ref, Sref in ((conv.weight, dw[k0:k1].view(conv.weight.shape), S[k0:k1].view(conv.weight.shape)),
                                         (conv.bias, db[k0:k1], Sdb[k0:k1])):
                        n = names.get(id(p), '?')
                        seen.add(n)
                        if p.grad is None:
                            self.failures.append(('param .grad missing', n))
                            continue
                        self.record('param .grad', tuple(p.shape), p.grad.double(), ref, bound(ref, Sref, 0.0),
                                    check=how, launched=False)
                    k0 = k1
                assert k0 <= dw.shape[0], (k0, dw.shape)
            for key, (ent, dwf, S, db, Sdb, calls) in self.params.items():
                if not hasattr(ent, 'src'):      # an unbanked weight (a WeightGradToken): the head rows above
                    continue
                src = ent.src
                w = src[0]
                # bf16 hand-over of the weight gradient into the chain rule (hip_conv._PrepWeights.backward, `gwf.to(
                # torch.bfloat16)`): one more rounding of dWf
                rho_h = RHO if key in self.bf16_handover else 0.0
                if len(src) == 5:
                    gamma, beta, mean, var = src[1:]
                    eps = ent.args[5] if ent.args is not None else 1e-5
                    dW, SdW, dg, Sdg = bn_chain_expect(dwf, S, db, Sdb, w, gamma, mean, var, eps)
                    hand_w = rho_h * dW.abs()
                    hand_g = rho_h * (dwf.abs() * w.double().abs()).sum((1, 2, 3)) / torch.sqrt(var.double() + eps)
                    checks = [(w, dW, SdW, hand_w), (gamma, dg, Sdg, hand_g), (beta, db, Sdb, 0.0)]
                else:
                    checks = [(w, dwf, S, rho_h * dwf.abs())] + ([(src[1], db, Sdb, 0.0)] if len(src) == 2 else [])
                for p, ref, Sref, hand in checks:
                    if not p.requires_grad:         # (frozen norm parameters, e.g. the caffe-style BN of R101-DC5)
                        continue
                    n = names.get(id(p), '?')
                    seen.add(n)
                    if p.grad is None:
                        self.failures.append(('param .grad missing', n))
                        continue
                    self.record('param .grad', (calls,) + tuple(p.shape), p.grad.double(), ref, bound(ref, Sref, 0.0, hand),
                                check='(conv)' if p is w else '(bn / bias)', launched=False)
        return seen
